"""GPU: per-stage average precision on the device (prego_perstage_ap_labels, csrc/metrics.hip) against the reference's figures
(tests/golden/perstage_ap_mixed.npz) and against the host form (prego_amd.metrics.perstage_ap_raw, which the CPU tests hold to the
reference and to sklearn); the C entry's refusals; `Evaluate` with cfg['eval_perstage']."""
import ctypes as C
import json
import logging
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd.metrics import STAGE_NAMES, perstage_ap_raw, perstage_average_precision, perstage_average_precision_device   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
TOL = 1e-12                                    # the project's AP tolerance (test_device_average_precision_kernel_vs_sklearn)


def _device_raw(scores, labels):
    names = [f"c{i}" for i in range(scores.shape[1])]
    return perstage_average_precision_device(torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda(), names, raw=True)


def _call(lib, scores, labels, n, ncls, ap, n_pos, ws, ws_bytes):
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    rc = lib.prego_perstage_ap_labels(p(scores), p(labels), n, ncls, p(ap), p(n_pos), p(ws), ws_bytes,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def test_golden_fixture():
    g = np.load(os.path.join(G, "perstage_ap_mixed.npz"))
    scores, labels, want = g["scores"], g["labels"], g["ap"]
    ap, n_pos = _device_raw(scores, labels)
    host_ap, host_pos = perstage_ap_raw(scores, labels)
    assert ap.shape == want.shape
    print("golden: max |device - reference|", np.abs(ap - want).max(), " max |device - host|", np.abs(ap - host_ap).max())
    assert np.abs(ap - want).max() < TOL                       # every (stage, class), class 0 and the absent class 5 included
    assert np.abs(ap - host_ap).max() < TOL
    assert np.array_equal(n_pos, host_pos)
    names = [f"c{i}" for i in range(scores.shape[1])]
    rep = perstage_average_precision_device(torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda(), names)
    assert list(rep) == [str(x) for x in g["stage_names"]] == list(STAGE_NAMES)
    for s, stage in enumerate(STAGE_NAMES):
        assert list(rep[stage]["per_class_AP"]) == names[1:]
        assert abs(rep[stage]["mean_AP"] - g["mean_ap"][s]) < TOL


@pytest.mark.parametrize("n,ncls", [(1, 3), (63, 5), (4097, 12), (8193, 86), (9001, 130)])      # radix tile and column-block edges
def test_tile_edges_vs_host(n, ncls):
    rng = np.random.default_rng(n + ncls)
    pr = rng.random((n, ncls)).astype(np.float32)
    pr[:, 2] = np.round(pr[:, 2], 1)                     # heavy ties
    if ncls > 4:
        pr[:, 4] = 0.5                                   # one threshold
        pr[:, 3] = rng.standard_normal(n).astype(np.float32) * 30          # negative scores too
    if ncls > 5:
        pr[:, 5] = np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(np.float32)     # signed zeros tie
    runs = []
    while sum(len(r) for r in runs) < n:                 # runs of 1..300 frames; ids -1 and ncls: negatives of every class
        runs.append(np.full(int(rng.integers(1, 301)), int(rng.integers(-1, ncls + 1)), np.int32))
    labels = np.concatenate(runs)[:n]
    ap, n_pos = _device_raw(pr, labels)
    host_ap, host_pos = perstage_ap_raw(pr, labels)
    print(f"n {n} C {ncls}: max |device - host| {np.abs(ap - host_ap).max():.3e}")
    assert np.array_equal(n_pos, host_pos)
    assert np.abs(ap - host_ap).max() < TOL


def long_list_case(levels):
    """(scores [5000, 3], ids): class 1 holds about 3000 frames in runs of 1..300, class 2 about 1000, class 0 none (id -1: a negative
    of every class); levels = 3: every column three long tie runs, levels = 0: tie-free"""
    from .test_cap_cpu import edge_scores
    n, ncls = 5000, 3
    rng = np.random.default_rng(50 + levels)
    scores = edge_scores(rng, n, ncls, levels)
    runs = []
    while sum(len(r) for r in runs) < n:
        runs.append(np.full(int(rng.integers(1, 301)), int(rng.choice([1, 1, 1, 2, -1])), np.int32))
    return scores, np.concatenate(runs)[:n]


@pytest.mark.parametrize("levels", [0, 3])
def test_long_lists_with_tie_runs_over_chunk_borders(levels):
    """A class with more than 2048 positives: its list takes three 1024-element chunks of the walk (csrc/metrics.hip, ap_walk_kernel),
    so the carries between chunks, every wave border and tie runs that span them are reached (by ids the edge shapes above give a class
    a few hundred positives).  All four entries by ids against the host forms within (P + 16) * 2^-52, P = the positives in that sum
    (tests/test_cap_cpu.py says why); equal positive counts; NaN exactly where the host form has it (class 0, which has no frame)."""
    from prego_amd.metrics import average_precision_columns, calibrated_average_precision_columns, perframe_ap_raw_device
    from .test_cap_cpu import close, onehot
    scores, labels = long_list_case(levels)
    ncls = scores.shape[1]
    names = [f"c{i}" for i in range(ncls)]
    pos = onehot(labels, ncls) != 0
    assert pos[:, 1].sum() > 2048 and pos[:, 2].sum() > 0 and pos[:, 0].sum() == 0
    pr, ids = torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda()
    for metric, columns in (("AP", average_precision_columns), ("cAP", calibrated_average_precision_columns)):
        got, n_pos, _ = perframe_ap_raw_device(pr, ids, metric)
        want = columns(scores, pos)
        ok, dev = close(got, want, pos.sum(0))
        print(f"levels {levels} {metric}: per-frame max |device - host| {dev:.3e}")
        assert np.isnan(want[0]) and np.isfinite(want[1:]).all()
        assert np.array_equal(n_pos, pos.sum(0))
        assert ok, (metric, got, want)
        got, n_pos = perstage_average_precision_device(pr, ids, names, raw=True, metrics=metric)
        want, want_pos = perstage_ap_raw(scores, labels, metric)
        ok, dev = close(got, want, want_pos)
        print(f"levels {levels} {metric}: per-stage max |device - host| {dev:.3e}")
        assert np.isfinite(want[:, 1:]).all() and (want_pos[:, 1:] > 0).all()
        assert np.array_equal(n_pos, want_pos)
        assert ok, (metric, got, want)


def test_worst_case_lists_stay_inside_the_queried_workspace():
    """every run one frame long: every positive is in all ten stages, the largest the per-stage counters get"""
    from prego_amd import _lib
    lib = _lib.load()
    n, ncls, guard = 5000, 3, 4096
    rng = np.random.default_rng(11)
    pr = np.round(rng.random((n, ncls)), 2).astype(np.float32)
    labels = (1 + np.arange(n) % 2).astype(np.int32)
    need = lib.prego_perstage_ap_workspace_bytes(n, ncls)
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.zeros((10, ncls), dtype=torch.float64, device="cuda")
    cnt = torch.zeros((10, ncls), dtype=torch.int64, device="cuda")
    assert _call(lib, torch.from_numpy(pr).cuda(), torch.from_numpy(labels).cuda(), n, ncls, out, cnt, ws, need) == 0
    assert bool((ws[need:] == 0xA5).all())
    host_ap, host_pos = perstage_ap_raw(pr, labels)
    assert np.array_equal(cnt.cpu().numpy(), host_pos) and host_pos[:, 1].tolist() == [n // 2] * 10
    assert np.abs(out.cpu().numpy() - host_ap).max() < TOL


def test_one_run_over_every_frame():
    n, ncls = 3000, 4
    pr = np.random.default_rng(3).random((n, ncls)).astype(np.float32)
    ap, n_pos = _device_raw(pr, np.full(n, 2, np.int32))
    assert np.all(ap[:, 2] == 1.0) and np.all(ap[:, [0, 1, 3]] == 0.0)
    assert np.array_equal(n_pos, perstage_ap_raw(pr, np.full(n, 2, np.int32))[1]) and n_pos[:, 2].sum() == n - 1


def test_two_calls_give_the_same_bits():
    rng = np.random.default_rng(8)
    n, ncls = 6000, 9
    pr = np.round(rng.random((n, ncls)), 2).astype(np.float32)
    labels = np.repeat(rng.integers(-1, ncls, 400), rng.integers(1, 40, 400))[:n].astype(np.int32)
    pr = pr[:labels.shape[0]]
    a, b = _device_raw(pr, labels), _device_raw(pr, labels)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_refusals_leave_outputs_and_workspace_untouched():
    from prego_amd import _lib
    lib = _lib.load()
    n, ncls = 100, 4
    pr = torch.rand(n, ncls, device="cuda")
    lab = torch.randint(0, ncls, (n,), dtype=torch.int32, device="cuda")
    need = lib.prego_perstage_ap_workspace_bytes(n, ncls)
    assert need > lib.prego_perframe_ap_workspace_bytes(n, ncls)
    assert lib.prego_perstage_ap_workspace_bytes(0, ncls) == 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((10, ncls), -7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((10, ncls), -7, dtype=torch.int64, device="cuda")
    EINVAL, EWORKSPACE = -1, -3
    for args, rc in [((None, lab, n, ncls, out, cnt, ws, need), EINVAL), ((pr, None, n, ncls, out, cnt, ws, need), EINVAL),
                     ((pr, lab, n, ncls, None, cnt, ws, need), EINVAL), ((pr, lab, n, ncls, out, cnt, None, need), EINVAL),
                     ((pr, lab, n, 0, out, cnt, ws, need), EINVAL), ((pr, lab, -1, ncls, out, cnt, ws, need), EINVAL),
                     ((pr, lab, n, ncls, out, cnt, ws, need - 1), EWORKSPACE)]:
        assert _call(lib, *args) == rc, args[2:4]
        assert bool((out == -7.0).all()) and bool((cnt == -7).all()) and bool((ws == 0x5A).all())
    assert b"prego_perstage_ap_workspace_bytes" in lib.prego_last_error()
    assert _call(lib, pr, lab, n, ncls, out, None, ws, need) == 0           # n_pos is optional
    assert bool((cnt == -7).all()) and not bool((out == -7.0).any())
    out.fill_(-7.0)
    assert _call(lib, pr, lab, 0, ncls, out, cnt, None, 0) == 0             # no frames: no error, zeros
    assert bool((out == 0.0).all()) and bool((cnt == 0).all())
    from prego_amd._lib import PregoError
    with pytest.raises(PregoError):
        perstage_average_precision_device(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), ["a", "b", "c"])
    with pytest.raises(PregoError):                                         # dense targets: the host path
        perstage_average_precision_device(torch.zeros(4, 3, device="cuda"), torch.zeros(4, 3, device="cuda"), ["a", "b", "c"])


def test_evaluate_keeps_the_perstage_report(tmp_path, monkeypatch):
    """cfg['eval_perstage']: `last_perstage` is the host function's report on the matrices the pass collected; what eval returns
    and writes is byte for byte what it is with the option off"""
    from prego_amd import weights as W
    from prego_amd.config import epic_tent_cfg
    from prego_amd.registry import build_model, build_eval
    import prego_amd.model, prego_amd.evaluate  # noqa: F401
    from .test_gpu_evaluate import _Loader
    lens = json.load(open(os.path.join(G, "g7_evaluate.json")))["lens"]
    names = [f"c{i}" for i in range(12)]
    vl = os.path.join(tmp_path, "video_list.json")
    json.dump({"EPIC-TENT-O": {"class_index": names}}, open(vl, "w"))
    seen = []
    orig = prego_amd.evaluate.perstage_average_precision_device

    def spy(pred, labels, *a, **k):
        seen.append((pred.cpu().numpy(), labels.cpu().numpy()))
        return orig(pred, labels, *a, **k)
    monkeypatch.setattr(prego_amd.evaluate, "perstage_average_precision_device", spy)
    res = {}
    for on in (True, False):
        out_dir = tmp_path / f"out_{int(on)}"
        cfg = epic_tent_cfg(eval="dummy.pth", video_list_path=vl, compute_dtype="fp16", eval_output_dir=str(out_dir), eval_perstage=on)
        model = build_model(cfg, "cuda:0")
        model.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_state_dict(cfg, 20, head_gain=8.0).items()})
        ev = build_eval(cfg)
        mAP = ev(model, _Loader(lens, 12, 20), logging.getLogger("t"), "cuda:0")
        res[on] = (mAP, open(out_dir / "output_miniROAD.json", "rb").read(), ev.last_perstage)
    assert res[True][0] == res[False][0] and res[True][1] == res[False][1]
    assert res[False][2] is None and len(seen) == 1
    pred, labels = seen[0]
    assert pred.shape == (sum(lens), 12) and labels.shape == (sum(lens),)
    want = perstage_average_precision(pred, labels, names)
    got = res[True][2]
    assert list(got) == list(want) == list(STAGE_NAMES)
    for stage in STAGE_NAMES:
        assert list(got[stage]["per_class_AP"]) == names[1:]
        for name in names[1:]:
            assert abs(got[stage]["per_class_AP"][name] - want[stage]["per_class_AP"][name]) < TOL
        assert abs(got[stage]["mean_AP"] - want[stage]["mean_AP"]) < TOL
    from prego_amd._lib import PregoError
    cfg = epic_tent_cfg(eval="dummy.pth", video_list_path=vl, compute_dtype="fp16", eval_output_dir=str(tmp_path / "out_m"),
                        eval_perstage=True, eval_label_targets=False)           # target rows travel as matrices: refused, and says so
    with pytest.raises(PregoError, match="one class id per frame"):
        build_eval(cfg)(model, _Loader(lens[:2], 12, 20), logging.getLogger("t"), "cuda:0")
