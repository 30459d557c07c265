"""GPU: the segmental metrics on the device (prego_segmental_scores, csrc/segmental.hip) word for word against the host model
(prego_amd/segmental.py, which tests/test_segmental_cpu.py holds to hand-computed cases and to the sequential fp64 form): the hand cases,
random video sets, video boundaries around the kernel's chunk size, the Levenshtein table around the LDS cap, the Epic-tent-O fixture,
`Evaluate` under cfg['eval_segmental'], every refusal, and the allocation / host-wait counters of the debug library."""
import ctypes as C
import gzip
import json
import logging
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import _lib                                                     # noqa: E402
from prego_amd._lib import PregoError, SEGMENTAL_CHUNK, SEGMENTAL_LDS_SEGMENTS    # noqa: E402
from prego_amd.segmental import (segmental_records, segmental_report, segmental_scores_device, voted_frames)      # noqa: E402
from tests.helpers.segmental_cases import HAND_CASES, concat, random_videos    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
DEV = "cuda:0"
CAP = SEGMENTAL_LDS_SEGMENTS


def _device_records(P, Gt, bg=(), overlaps=None, misalign=False):
    """the kernel's records of host videos; misalign: pred and gt start 4 bytes behind a 16-byte boundary (the scalar load path)"""
    pf, off = concat(P)
    gf, _ = concat(Gt)
    pad = 1 if misalign else 0
    pd = torch.from_numpy(np.concatenate((np.zeros(pad, np.int32), pf))).to(DEV)[pad:]
    gd = torch.from_numpy(np.concatenate((np.zeros(pad, np.int32), gf))).to(DEV)[pad:]
    assert (pd.data_ptr() % 16 != 0) == (misalign and pf.size > 0) or pf.size == 0
    kw = {} if overlaps is None else {"overlaps": overlaps}
    rec = segmental_scores_device(pd, gd, torch.from_numpy(off).to(DEV), bg=bg, raw=True, **kw)
    return torch.from_numpy(rec)


def _check(P, Gt, bg=(), overlaps=None, misalign=False):
    kw = {} if overlaps is None else {"overlaps": overlaps}
    want = torch.from_numpy(segmental_records(P, Gt, bg, **kw))
    got = _device_records(P, Gt, bg, overlaps, misalign)
    assert got.dtype == torch.int32 and got.shape == want.shape
    if not torch.equal(got, want):
        bad = (got != want).any(1).nonzero().flatten().tolist()
        raise AssertionError(f"videos {bad[:5]} of {len(P)}: device {got[bad[:5]].tolist()} host {want[bad[:5]].tolist()}")
    return want


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_cases(name):
    case = HAND_CASES[name]
    got = _device_records(case["pred"], case["gt"], case.get("bg", ()))
    assert torch.equal(got, torch.tensor(case["records"], dtype=torch.int32)), (name, got.tolist())


# V 300 and 1100: more videos than one wave of workgroups / than the grid (1024 workgroups), which then strides
@pytest.mark.parametrize("V,max_len,alphabet,oor,mask,misalign", [
    (1, 5000, 12, False, "none", False), (1, 5000, 86, True, "some", True), (3, 5000, 1, False, "none", False),
    (3, 5000, 128, True, "all", False), (3, 5000, 12, False, "all", True), (64, 1500, 86, False, "some", False),
    (64, 1500, 128, True, "none", True), (300, 400, 12, True, "some", False), (300, 400, 1, False, "none", True),
    (1100, 60, 12, False, "some", False)])
def test_random_sets(V, max_len, alphabet, oor, mask, misalign):
    rng = np.random.default_rng(V * 1000 + alphabet + max_len)
    P, Gt, bg = random_videos(rng, V, max_len, alphabet, oor, mask, lengths=[max_len] if V == 1 else None)
    _check(P, Gt, bg, misalign=misalign)


def test_other_overlaps():
    rng = np.random.default_rng(5)
    P, Gt, bg = random_videos(rng, 40, 700, 6, False, "none")
    a = _check(P, Gt, bg, overlaps=((1, 3), (32767, 32768), (1, 1)))
    b = _check(P, Gt, bg, overlaps=((1, 32768), (2, 3), (3, 4)))
    assert (a[:, 5] >= a[:, 6]).all() and (a[:, 6] >= a[:, 7]).all() and (b[:, 5] >= a[:, 5]).all()


@pytest.mark.parametrize("misalign", [False, True])
def test_video_boundaries_around_the_chunk_size(misalign):
    """video boundaries at and next to every multiple of the chunk size (of the axis and of the video), equal labels across them"""
    K = SEGMENTAL_CHUNK
    lens = [K - 1, 1, 1, 1, K - 3, K, K + 1, K - 1, 2 * K, 2 * K - 1, 2 * K + 1, 3, K - 3, 4 * K, 2, K - 2, K + 2, 5]
    n = sum(lens)
    cuts = np.cumsum(lens)[:-1]
    flat_p = np.full(n, 5, np.int32)                               # one label everywhere: every boundary splits a run
    flat_g = ((np.arange(n) // 512) % 2 + 5).astype(np.int32)      # runs of 512 that cross the boundaries
    P, Gt = np.split(flat_p, cuts), np.split(flat_g, cuts)
    want = _check(P, Gt, misalign=misalign)
    assert want[:, 2].tolist() == [1] * len(lens)
    rng = np.random.default_rng(77)
    P, Gt, bg = random_videos(rng, len(lens), alphabet=4, mask="some", lengths=lens)
    _check(P, Gt, bg, misalign=misalign)
    for v in range(len(lens) - 1):                                 # the same label on both sides of every boundary
        if len(P[v]) and len(P[v + 1]):
            P[v + 1][0] = P[v][-1]
            Gt[v + 1][0] = Gt[v][-1]
    _check(P, Gt, bg, misalign=misalign)


def _alternating(k, period):
    return (np.arange(k) % period).astype(np.int32)


def test_table_sizes_around_the_lds_cap():
    """min(m, n) in {0, 1, 63, 64, 65, 1023, 1024, 1025, cap - 1, cap, cap + 1}: one-frame runs, so a video of k frames has k segments on
    both sides (labels of period 2 against period 3: a distance that is neither 0 nor k); above the cap the diagonals live in the
    workspace.  Then one side much longer than the other AT the cap, both ways: which side is the short one."""
    sizes = [0, 1, 63, 64, 65, 1023, 1024, 1025, CAP - 1, CAP, CAP + 1]
    P = [_alternating(k, 2) for k in sizes]
    Gt = [_alternating(k, 3) for k in sizes]
    long_, short = _alternating(3 * CAP, 2), np.repeat(_alternating(CAP, 3), 3)
    P += [long_, short, _alternating(3 * (CAP + 1), 2), np.repeat(_alternating(CAP + 1, 3), 3)]
    Gt += [short, long_, np.repeat(_alternating(CAP + 1, 3), 3), _alternating(3 * (CAP + 1), 2)]
    want = _check(P, Gt).numpy()
    assert np.minimum(want[:, 2], want[:, 3]).tolist() == sizes + [CAP, CAP, CAP + 1, CAP + 1]
    assert want[-4:, 2].tolist() == [3 * CAP, CAP, 3 * (CAP + 1), CAP + 1]
    assert (want[2:, 4] > 0).all() and (want[2:, 4] < np.maximum(want[2:, 2], want[2:, 3])).all()      # from 63 segments on: neither 0 nor all


def test_epic_tent_fixture_raw_and_voted():
    g = json.load(gzip.open(os.path.join(G, "g8_output_miniROAD.json.gz")))
    gold = json.load(open(os.path.join(G, "segmental_epic_tent.json")))
    P, Gt = [np.asarray(v["pred"], np.int32) for v in g.values()], [np.asarray(v["gt"], np.int32) for v in g.values()]
    assert torch.equal(_device_records(P, Gt), torch.tensor(gold["frames"], dtype=torch.int32))
    # the vote on the device as Evaluate runs it: prego_window_vote per video, expanded back to frames
    lib = _lib.load()
    V = []
    for p in P:
        pd = torch.from_numpy(p).to(DEV)
        votes = torch.empty((len(p) + 199) // 200, dtype=torch.int32, device=DEV)
        assert lib.prego_window_vote(C.c_void_p(pd.data_ptr()), len(p), 200, 12, C.c_void_p(votes.data_ptr()), None) == 0
        V.append(torch.repeat_interleave(votes, 200)[:len(p)].cpu().numpy())
        assert np.array_equal(V[-1], voted_frames(p, 200))
    assert torch.equal(_device_records(V, Gt), torch.tensor(gold["vote"], dtype=torch.int32))


def test_device_report_defer_and_host_tensors():
    rng = np.random.default_rng(9)
    P, Gt, bg = random_videos(rng, 7, 900, 12, False, "some")
    pf, off = concat(P)
    gf, _ = concat(Gt)
    pd, gd, od = (torch.from_numpy(x).to(DEV) for x in (pf, gf, off))
    fn = segmental_scores_device(pd, gd, od, bg=bg, defer=True)
    assert callable(fn)
    rep = fn()
    assert rep == segmental_report(segmental_records(P, Gt, bg))
    assert set(rep) == {"MoF", "Edit", "F1@10", "F1@25", "F1@50", "videos", "per_video"} and rep["videos"] == 7
    with pytest.raises(PregoError, match="CUDA"):
        segmental_scores_device(pd.cpu(), gd.cpu(), od.cpu())
    with pytest.raises(PregoError, match="int32"):
        segmental_scores_device(pd.long(), gd, od)
    # no frames at all: every record is eight zeros, no workspace
    z = torch.zeros(0, dtype=torch.int32, device=DEV)
    rec = segmental_scores_device(z, z, torch.zeros(4, dtype=torch.int32, device=DEV), raw=True)
    assert rec.shape == (3, 8) and not rec.any()


def test_offsets_are_clamped():
    """offsets words outside [0, n_frames] are clamped before they index memory and a descending pair is an empty video"""
    p = torch.from_numpy(_alternating(1000, 2)).to(DEV)
    g = torch.from_numpy(_alternating(1000, 3)).to(DEV)
    hp, hg = p.cpu().numpy(), g.cpu().numpy()
    off = torch.tensor([-5, 400, 2 ** 31 - 1], dtype=torch.int32, device=DEV)            # [0, 400), [400, 1000)
    assert np.array_equal(segmental_scores_device(p, g, off, raw=True), segmental_records([hp[:400], hp[400:]], [hg[:400], hg[400:]]))
    off = torch.tensor([300, 200, 1000, -2 ** 31], dtype=torch.int32, device=DEV)        # empty, [200, 1000), empty
    assert np.array_equal(segmental_scores_device(p, g, off, raw=True),
                          segmental_records([hp[:0], hp[200:], hp[:0]], [hg[:0], hg[200:], hg[:0]]))


def _p(t):
    return C.c_void_p(t.data_ptr())


def test_every_refusal_leaves_records_and_workspace_untouched():
    lib = _lib.load()
    n, V = 5000, 3
    pred = torch.zeros(n, dtype=torch.int32, device=DEV)
    gt = torch.ones(n, dtype=torch.int32, device=DEV)
    off = torch.tensor([0, 100, 100, n], dtype=torch.int32, device=DEV)
    need = lib.prego_segmental_workspace_bytes(n, V)
    assert need > 0 and lib.prego_segmental_workspace_bytes(0, V) == 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=DEV)
    rec = torch.full((V * 8 + 4,), -77, dtype=torch.int32, device=DEV)
    assert rec.data_ptr() % 16 == 0
    num = lambda *v: (C.c_int32 * 3)(*v)
    EINVAL, EWORKSPACE = -1, -3                                     # PREGO_EINVAL, PREGO_EWORKSPACE

    def call(pred_=pred, gt_=gt, off_=off, V_=V, n_=n, num_=None, den_=None, rec_=rec, ws_=ws, ws_bytes=need):
        return lib.prego_segmental_scores(_p(pred_) if pred_ is not None else None, _p(gt_) if gt_ is not None else None,
                                          _p(off_) if off_ is not None else None, V_, n_, None, num_, den_,
                                          C.c_void_p(rec_) if isinstance(rec_, int) else (_p(rec_) if rec_ is not None else None),
                                          _p(ws_) if ws_ is not None else None, ws_bytes, None)
    refused = [call(pred_=None), call(gt_=None), call(off_=None), call(rec_=None), call(ws_=None), call(V_=0), call(V_=-3), call(n_=-1),
               call(n_=2 ** 31), call(rec_=rec.data_ptr() + 4), call(num_=num(0, 1, 1), den_=num(10, 4, 2)),
               call(num_=num(1, 5, 1), den_=num(10, 4, 2)), call(num_=num(1, 1, 1), den_=num(10, 4, 32769)),
               call(num_=num(1, -1, 1), den_=num(10, 4, 2)), call(num_=num(1, 1, 1), den_=None)]
    assert refused == [EINVAL] * len(refused)
    assert b"segmental_scores" in lib.prego_last_error()
    short = call(ws_bytes=need - 1)
    assert short == EWORKSPACE and b"prego_segmental_workspace_bytes" in lib.prego_last_error()
    torch.cuda.synchronize()
    assert bool((rec == -77).all()) and bool((ws == 0x5A).all())
    assert call() == 0                                              # and the same arguments unrefused run
    torch.cuda.synchronize()
    want = segmental_records([np.zeros(100), np.zeros(0), np.zeros(n - 100)], [np.ones(100), np.ones(0), np.ones(n - 100)])
    assert np.array_equal(rec[:V * 8].cpu().numpy().reshape(V, 8), want) and bool((rec[V * 8:] == -77).all())
    assert call(n_=0, ws_=None, ws_bytes=0) == 0                     # no frames: legal without a workspace
    torch.cuda.synchronize()
    assert not rec[:V * 8].any() and bool((rec[V * 8:] == -77).all())


def test_no_allocation_and_no_host_wait_in_the_entry():
    dbg = _lib.load_debug()
    rng = np.random.default_rng(3)
    P, Gt, _ = random_videos(rng, 5, 2000, 12)
    pf, off = concat(P)
    gf, _ = concat(Gt)
    pd, gd, od = (torch.from_numpy(x).to(DEV) for x in (pf, gf, off))
    ws = torch.empty(dbg.prego_segmental_workspace_bytes(len(pf), 5), dtype=torch.uint8, device=DEV)
    rec = torch.empty((5, 8), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()

    def counts():
        a, w = C.c_int64(), C.c_int64()
        assert dbg.prego_debug_alloc_count(C.byref(a), C.byref(w)) == 0
        return a.value, w.value
    n0 = counts()
    assert dbg.prego_segmental_scores(_p(pd), _p(gd), _p(od), 5, len(pf), None, None, None, _p(rec), _p(ws), ws.numel(), None) == 0
    assert counts() == n0
    torch.cuda.synchronize()
    assert np.array_equal(rec.cpu().numpy(), segmental_records(P, Gt))


# ---- Evaluate ----
def _eval_items(lens, multi=False):
    from prego_amd import weights as W
    items = []
    for i, T in enumerate(lens):
        rgb = torch.from_numpy(W.tsn_features((T, 2048), 21, f"seg.rgb.{i}"))[None].pin_memory()
        tgt = torch.zeros(1, T, 12)
        tgt[0, torch.arange(T), (torch.arange(T) // 41 + i) % 12] = 1
        if multi and i == 2:
            tgt[0, 100:200, 7] = 1
        items.append((rgb, torch.zeros(1, 1, 2048).expand(1, T, 2048), tgt.pin_memory(), (f"v{i}",), torch.tensor([0]), torch.tensor([T])))
    return items


def _run_eval(tmp_path, tag, items, **over):
    from prego_amd import weights as W
    from prego_amd.config import epic_tent_cfg
    from prego_amd.registry import build_eval, build_model
    import prego_amd.evaluate, prego_amd.model  # noqa: F401
    vl = os.path.join(tmp_path, "video_list.json")
    json.dump({"EPIC-TENT-O": {"class_index": [f"c{i}" for i in range(12)]}}, open(vl, "w"))
    out_dir = tmp_path / tag
    cfg = epic_tent_cfg(eval="dummy.pth", video_list_path=vl, compute_dtype="fp16", eval_output_dir=str(out_dir), **over)
    model = build_model(cfg, DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_state_dict(cfg, 20, head_gain=8.0).items()})
    ev = build_eval(cfg)
    return ev, model, out_dir


def test_evaluate_segmental(tmp_path):
    lens = [900, 1, 2500, 333, 64]
    items = _eval_items(lens)
    log = logging.getLogger("t")
    ev, model, out_dir = _run_eval(tmp_path, "on", items, eval_segmental=True)
    mAP = ev(model, items, log, DEV)
    js = json.load(open(out_dir / "output_miniROAD.json"))
    P, Gt = [js[f"v{i}"]["pred"] for i in range(len(lens))], [js[f"v{i}"]["gt"] for i in range(len(lens))]
    assert ev.last_segmental["frames"] == segmental_report(segmental_records(P, Gt))
    assert ev.last_segmental["vote"] == segmental_report(segmental_records([voted_frames(p, 200) for p in P], Gt))
    ev50, model50, _ = _run_eval(tmp_path, "w50", items, eval_segmental=True, eval_segmental_window=50)
    ev50(model50, items, log, DEV)
    assert ev50.last_segmental["frames"] == ev.last_segmental["frames"]
    assert ev50.last_segmental["vote"] == segmental_report(segmental_records([voted_frames(p, 50) for p in P], Gt))
    # the key off: no report, and nothing else about the pass differs
    ev0, model0, out0 = _run_eval(tmp_path, "off", items)
    mAP0 = ev0(model0, items, log, DEV)
    assert getattr(ev0, "last_segmental", None) is None
    assert mAP0 == mAP and json.load(open(out0 / "output_miniROAD.json")) == js
    assert [p for p, _ in ev0.phase_log] == [p for p, _ in ev.phase_log if p != "segmental_done"]


def test_evaluate_segmental_refusals(tmp_path, monkeypatch):
    log = logging.getLogger("t")
    items = _eval_items([300, 40, 500], multi=True)
    ev, model, _ = _run_eval(tmp_path, "dense", items, eval_segmental=True)
    with pytest.raises(PregoError, match="eval_segmental.*one class id per frame"):
        ev(model, items, log, DEV)
    ev, model, _ = _run_eval(tmp_path, "cpu", items, eval_segmental=True)
    with pytest.raises(PregoError, match="eval_segmental.*on the device"):
        ev(model, items, log, "cpu")
    import prego_amd.evaluate as E
    for name, val in (("is_available", True), ("is_initialized", True), ("get_world_size", 2), ("get_rank", 0)):
        monkeypatch.setattr(E.dist, name, lambda *a, _v=val, **k: _v)
    with pytest.raises(PregoError, match="eval_segmental.*2 ranks"):
        ev(model, items, log, DEV)
