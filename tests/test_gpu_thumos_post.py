"""GPU: the THUMOS post-processing on the device (prego_thumos_postprocess(_labels), csrc/thumos_post.hip) against the reference's outputs
(tests/golden/thumos_post.npz) and the host form (prego_amd/postprocessing.py, which tests/test_thumos_post_cpu.py holds to the
reference): bit for bit - the operation is comparisons and copies.  Then the metrics on device-post-processed input, the C entries'
refusals, and `Evaluate` / `AntEvaluate` under cfg['eval_thumos_postprocessing'].

Sizes: R = the kernel's rows per tile (`_lib.THUMOS_TILE_ROWS`); the halo of the 5-frame window crosses a tile border within two rows of
it, the column chunk is 96 wide and target rows of 256 columns or more are copied by another loop, so those sizes are the cases.
Metric tolerance: `close` of tests/test_cap_cpu.py, (P + 16) * 2^-52 per value."""
import ctypes as C
import json
import logging
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import _lib                                                                                       # noqa: E402
from prego_amd._lib import PregoError                                                                            # noqa: E402
from prego_amd.metrics import (STAGE_NAMES, calibrated_average_precision_columns, perframe_average_precision,   # noqa: E402
                               perframe_average_precision_device, perstage_average_precision, perstage_average_precision_device)
from prego_amd.postprocessing import ThumosPostprocessing, thumos_postprocessing_device                         # noqa: E402
from .test_cap_cpu import close, onehot                                                                          # noqa: E402
from .test_thumos_post_cpu import COMBOS, golden, same_bits                                                      # noqa: E402

EINVAL, EWORKSPACE = -1, -3
R = _lib.THUMOS_TILE_ROWS
NAMES = [f"c{i}" for i in range(22)]


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def device_form(scores, truth, post, n_valid=None):
    """(ground_truth, prediction) as host arrays, and the device count"""
    res = thumos_postprocessing_device(cuda(scores), cuda(truth), post, n_valid)
    count = res.check()
    return res[0].cpu().numpy(), res[1].cpu().numpy(), count


def check_against_host(scores, truth, post, what):
    want_t, want_p = post(truth, scores)
    got_t, got_p, count = device_form(scores, truth, post)
    assert count == want_t.shape[0], what
    assert same_bits(got_p, want_p), (what, "scores")
    assert same_bits(got_t, want_t.astype(got_t.dtype)), (what, "targets")
    hinted_t, hinted_p, _ = device_form(scores, truth, post, n_valid=count)          # the same without the count's readback
    assert same_bits(hinted_p, got_p) and same_bits(hinted_t, got_t), (what, "n_valid hint")


def random_case(rng, n, ncls=22, amb=21, share=0.2):
    scores = rng.random((n, ncls)).astype(np.float32)
    ids = rng.integers(0, max(amb, 1), n).astype(np.int32)
    ids[rng.random(n) < share] = amb
    return scores, ids


def all_posts(**kw):
    return [ThumosPostprocessing(bool(s), bool(w), **kw) for s, w in COMBOS]


@pytest.mark.parametrize("smooth,switch", COMBOS)
def test_fixture_bit_for_bit(smooth, switch):
    g = golden()
    post = ThumosPostprocessing(bool(smooth), bool(switch))
    want_p = g[f"pred_out_{smooth}{switch}"]
    gt, pr, count = device_form(g["scores"], g["target"], post)
    assert count == want_p.shape[0] and same_bits(pr, want_p) and same_bits(gt, g["gt_out"])
    ids, pr, count = device_form(g["scores"], g["labels"], post)
    assert count == want_p.shape[0] and same_bits(pr, want_p) and same_bits(ids, g["labels"][g["target"][:, 21] != 1])


@pytest.mark.parametrize("n", [2, 3, 4, 5, R - 2, R - 1, R, R + 1, R + 2, 2 * R + 1, 5003])
def test_random_inputs_equal_the_host_form(n):
    rng = np.random.default_rng(n)
    scores, ids = random_case(rng, n)
    dense = onehot(ids, 22)
    dense[rng.random(n) < 0.1, 3] = 1                                 # multi-label rows
    for post in all_posts():
        check_against_host(scores, ids, post, (n, "ids", post))
        check_against_host(scores, dense, post, (n, "dense", post))


def _border_rows(n):
    """rows at which a tile starts, and their neighbours within the smoothing halo"""
    rows = {0, 1, n - 2, n - 1}
    for b in range(R, n, R):
        rows |= {b - 2, b - 1, b, b + 1}
    return sorted(r for r in rows if 0 <= r < n)


def test_ambiguous_and_score_patterns_at_tile_borders():
    n = 3 * R + 5
    rng = np.random.default_rng(77)
    base = rng.random((n, 22)).astype(np.float32)
    patterns = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "every other": np.arange(n) % 2 == 0}
    for off in (-2, -1, 0, 1, 2):                                     # runs of 5 ambiguous rows that END at a tile border + off
        m = np.zeros(n, bool)
        for b in range(R, n, R):
            m[b + off - 5:b + off] = True
        patterns[f"runs ending at border{off:+d}"] = m
    for name, amb in patterns.items():
        ids = rng.integers(0, 21, n).astype(np.int32)
        ids[amb] = 21
        for k, r in enumerate(_border_rows(n)):                       # one large value per border row, each in its own column set
            scores = base.copy()
            scores[r, :] = 100.0 + k
            if k % 4 == 0 or name == "none":                          # every row with no ambiguous frame, a quarter of them otherwise
                for post in all_posts():
                    check_against_host(scores, ids, post, (name, r, post))
        if name == "all":
            for post in all_posts():
                res = thumos_postprocessing_device(cuda(base), cuda(ids), post)
                assert res.check() == 0 and res[0].shape == (0,) and res[1].shape == (0, 22)
                rep = perframe_average_precision_device(cuda(base), cuda(ids), NAMES, post, "AP")
                assert not rep["per_class_AP"] and np.isnan(rep["mean_AP"])
                stage = perstage_average_precision_device(cuda(base), cuda(ids), NAMES, postprocessing=post)
                assert list(stage) == list(STAGE_NAMES) and all(v["mean_AP"] == 0.0 for v in stage.values())


@pytest.mark.parametrize("ncls,kw", [(86, dict(ambiguous=21, switch_from=5, switch_to=8)), (22, dict(ambiguous=-1)),
                                     (200, dict(ambiguous=150, switch_from=5, switch_to=190)),       # two column chunks, a switch across them
                                     (200, dict(ambiguous=3, switch_from=199, switch_to=0)),
                                     (300, dict(ambiguous=299, switch_from=100, switch_to=101))])    # dense target rows wider than a block
def test_other_widths_and_columns(ncls, kw):
    n = 2 * R + 3
    rng = np.random.default_rng(ncls)
    scores, ids = random_case(rng, n, ncls, max(kw["ambiguous"], 0))
    dense = onehot(ids, ncls)
    for post in all_posts(**kw):
        check_against_host(scores, ids, post, (ncls, kw, "ids", post))
        check_against_host(scores, dense, post, (ncls, kw, "dense", post))
    if kw["ambiguous"] == -1:
        assert device_form(scores, ids, ThumosPostprocessing(**kw))[2] == n


def test_strided_step_views_are_read_in_place():
    n, L = R + 9, 3
    rng = np.random.default_rng(9)
    pred = cuda(rng.random((n, L, 22)).astype(np.float32))
    ids = rng.integers(0, 22, (n, L))
    tgt = cuda(np.eye(22, dtype=np.float32)[ids])
    for post in all_posts():
        for l in range(L):
            p_view, t_view = pred[:, l, :], tgt[:, l, :]
            assert not p_view.is_contiguous()
            a = thumos_postprocessing_device(p_view, t_view, post)
            b = thumos_postprocessing_device(p_view.contiguous(), t_view.contiguous(), post)
            assert a.check() == b.check() == int((ids[:, l] != 21).sum())
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            want_t, want_p = post(tgt[:, l].cpu().numpy(), pred[:, l].cpu().numpy())
            assert same_bits(a[1].cpu().numpy(), want_p) and same_bits(a[0].cpu().numpy(), want_t)


def test_nothing_to_do_returns_the_inputs_and_inputs_are_never_written():
    n = 2 * R + 1
    rng = np.random.default_rng(3)
    scores, ids = random_case(rng, n, share=0.0)
    gt, pr, count = device_form(scores, ids, ThumosPostprocessing())
    assert count == n and same_bits(pr, scores) and same_bits(gt, ids)
    scores, ids = random_case(rng, n)
    s_dev, i_dev, d_dev = cuda(scores), cuda(ids), cuda(onehot(ids, 22))
    for post in all_posts():
        thumos_postprocessing_device(s_dev, i_dev, post).check()
        thumos_postprocessing_device(s_dev, d_dev, post).check()
    assert same_bits(s_dev.cpu().numpy(), scores) and same_bits(i_dev.cpu().numpy(), ids) and same_bits(d_dev.cpu().numpy(), onehot(ids, 22))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _raw(lib, scores, truth, n, ncls, flags, out_s, out_t, cnt, ws, ws_bytes, sw=(5, 8), amb=21, ld_s=None, ld_t=None):
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if truth is not None and truth.dtype == torch.int32 or (truth is None and out_t is not None and out_t.dtype == torch.int32):
        rc = lib.prego_thumos_postprocess_labels(_p(scores), ncls if ld_s is None else ld_s, _p(truth), n, ncls, flags, sw[0], sw[1], amb,
                                                 _p(out_s), _p(out_t), _p(cnt), _p(ws), ws_bytes, s)
    else:
        rc = lib.prego_thumos_postprocess(_p(scores), ncls if ld_s is None else ld_s, _p(truth), ncls if ld_t is None else ld_t, n, ncls,
                                          flags, sw[0], sw[1], amb, _p(out_s), _p(out_t), _p(cnt), _p(ws), ws_bytes, s)
    torch.cuda.synchronize()
    return rc


def test_rows_beyond_n_valid_are_not_written():
    lib = _lib.load()
    n = 2 * R + 7
    rng = np.random.default_rng(21)
    scores, some = random_case(rng, n, share=0.3)
    every = np.full(n, 21, np.int32)                                  # every frame ambiguous: no output row is written at all
    need = lib.prego_thumos_postprocess_workspace_bytes(n, 22)
    for ids, truth in ((some, cuda(some)), (some, cuda(onehot(some, 22))), (every, cuda(every)), (every, cuda(onehot(every, 22)))):
        for flags in (0, 3):
            out_s = torch.full((n, 22), -7.0, device="cuda")
            out_t = torch.full(truth.shape, -7, dtype=truth.dtype, device="cuda")
            cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
            ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
            assert _raw(lib, cuda(scores), truth, n, 22, flags, out_s, out_t, cnt, ws, need) == 0
            k = int(cnt.item())
            assert k == int((ids != 21).sum()) and (k == 0 if ids is every else 0 < k < n)
            assert bool((out_s[k:] == -7.0).all()) and bool((out_t[k:] == -7).all())
            want_t, want_p = ThumosPostprocessing(flags & 1, flags & 2)(truth.cpu().numpy(), scores)
            assert same_bits(out_s[:k].cpu().numpy(), want_p) and same_bits(out_t[:k].cpu().numpy(), want_t)


def test_refusals_leave_outputs_count_and_workspace_untouched():
    lib = _lib.load()
    n, ncls = 300, 22
    rng = np.random.default_rng(2)
    scores, ids = random_case(rng, n)
    sc, lab, den = cuda(scores), cuda(ids), cuda(onehot(ids, ncls))
    need = lib.prego_thumos_postprocess_workspace_bytes(n, ncls)
    assert need > 0 and lib.prego_thumos_postprocess_workspace_bytes(0, ncls) == 0
    out_s = torch.full((n, ncls), -7.0, device="cuda")
    out_d = torch.full((n, ncls), -7.0, device="cuda")
    out_l = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")

    def untouched():
        return bool((out_s == -7.0).all()) and bool((out_d == -7.0).all()) and bool((out_l == -7).all()) and int(cnt.item()) == -7 and \
            bool((ws == 0x5A).all())

    def refused(rc, code=EINVAL):
        assert rc == code and untouched() and lib.prego_last_error()

    # ---- NULL inputs and outputs
    refused(_raw(lib, None, den, n, ncls, 0, out_s, out_d, cnt, ws, need))
    refused(_raw(lib, sc, None, n, ncls, 0, out_s, out_d, cnt, ws, need))
    refused(_raw(lib, sc, None, n, ncls, 0, out_s, out_l, cnt, ws, need))
    refused(_raw(lib, sc, den, n, ncls, 0, None, out_d, cnt, ws, need))
    refused(_raw(lib, sc, den, n, ncls, 0, out_s, None, cnt, ws, need))
    refused(_raw(lib, sc, lab, n, ncls, 0, out_s, None, cnt, ws, need))
    refused(_raw(lib, sc, den, n, ncls, 0, out_s, out_d, None, ws, need))
    refused(_raw(lib, sc, den, n, ncls, 0, out_s, out_d, cnt, None, need))
    # ---- sizes
    refused(_raw(lib, sc, den, -1, ncls, 0, out_s, out_d, cnt, ws, need))
    refused(_raw(lib, sc, lab, 2 ** 31, ncls, 0, out_s, out_l, cnt, ws, need))
    refused(_raw(lib, sc, den, n, 0, 0, out_s, out_d, cnt, ws, need))
    refused(_raw(lib, sc, den, n, 65536, 0, out_s, out_d, cnt, ws, need))
    refused(_raw(lib, sc, den, n, ncls, 0, out_s, out_d, cnt, ws, need, ld_s=ncls - 1))
    refused(_raw(lib, sc, den, n, ncls, 0, out_s, out_d, cnt, ws, need, ld_t=ncls - 1))
    refused(_raw(lib, sc, lab, n, ncls, 0, out_s, out_l, cnt, ws, need, ld_s=ncls - 1))
    # ---- columns and flags
    refused(_raw(lib, sc, den, n, ncls, 0, out_s, out_d, cnt, ws, need, amb=ncls))
    refused(_raw(lib, sc, lab, n, ncls, 0, out_s, out_l, cnt, ws, need, amb=-2))
    refused(_raw(lib, sc, den, n, ncls, 2, out_s, out_d, cnt, ws, need, sw=(-1, 8)))
    refused(_raw(lib, sc, den, n, ncls, 2, out_s, out_d, cnt, ws, need, sw=(5, ncls)))
    refused(_raw(lib, sc, lab, n, ncls, 3, out_s, out_l, cnt, ws, need, sw=(8, 8)))
    refused(_raw(lib, sc, den, n, ncls, 4, out_s, out_d, cnt, ws, need))
    assert _raw(lib, sc, lab, n, ncls, 1, torch.empty_like(out_s), torch.empty_like(out_l), torch.zeros_like(cnt), torch.empty_like(ws), need,
                sw=(8, 8)) == 0                                       # the switch columns matter only with the flag
    # ---- an output that overlaps an input
    refused(_raw(lib, sc, den, n, ncls, 0, sc, out_d, cnt, ws, need))
    refused(_raw(lib, sc, den, n, ncls, 0, out_s, den, cnt, ws, need))
    refused(_raw(lib, sc, den, n, ncls, 0, den, out_d, cnt, ws, need))
    refused(_raw(lib, sc, lab, n, ncls, 0, out_s, lab, cnt, ws, need))
    refused(_raw(lib, sc, den, n - 1, ncls, 0, sc[1:], out_d, cnt, ws, need))
    # ---- workspace
    refused(_raw(lib, sc, den, n, ncls, 0, out_s, out_d, cnt, ws, need - 1), EWORKSPACE)
    assert b"prego_thumos_postprocess_workspace_bytes" in lib.prego_last_error()
    # ---- no frames: no error, a zero count, no workspace
    assert _raw(lib, sc, den, 0, ncls, 3, out_s, out_d, cnt, None, 0) == 0
    assert int(cnt.item()) == 0 and bool((out_s == -7.0).all()) and bool((out_d == -7.0).all())
    # ---- the Python entries
    with pytest.raises(PregoError):
        thumos_postprocessing_device(sc.cpu(), den.cpu(), ThumosPostprocessing())
    with pytest.raises(PregoError):
        thumos_postprocessing_device(sc, den, lambda g, p: (g, p))
    with pytest.raises(PregoError):
        perstage_average_precision_device(sc, lab, NAMES, postprocessing=lambda g, p: (g, p))
    with pytest.raises(PregoError):
        perframe_average_precision_device(sc, lab, NAMES, None, "AP", n_valid=3)
    with pytest.raises(PregoError):
        thumos_postprocessing_device(sc, lab, ThumosPostprocessing(), n_valid=n + 1)


def test_a_wrong_n_valid_hint_is_reported_at_collection():
    n = R + 40
    rng = np.random.default_rng(13)
    scores, ids = random_case(rng, n)
    post = ThumosPostprocessing(True, True)
    right = post.count_valid(ids)
    sc, lab = cuda(scores), cuda(ids)
    for wrong in (right - 1, right + 1):
        res = thumos_postprocessing_device(sc, lab, post, n_valid=wrong)
        assert res[1].shape == (wrong, 22)                            # sized by the hint, nothing waited for
        with pytest.raises(PregoError, match="n_valid"):
            res.check()
        fin = perframe_average_precision_device(sc, lab, NAMES, post, "AP", defer=True, n_valid=wrong)
        with pytest.raises(PregoError, match="n_valid"):
            fin()
        fin = perstage_average_precision_device(sc, lab, NAMES, defer=True, postprocessing=post, n_valid=wrong)
        with pytest.raises(PregoError, match="n_valid"):
            fin()
    assert thumos_postprocessing_device(sc, lab, post, n_valid=right).check() == right


@pytest.mark.parametrize("metric", ["AP", "cAP"])
@pytest.mark.parametrize("smooth,switch", COMBOS)
def test_metric_on_device_postprocessed_input(metric, smooth, switch):
    g = golden()
    post = ThumosPostprocessing(bool(smooth), bool(switch))
    ref_p, ref_t = g[f"pred_out_{smooth}{switch}"], g["gt_out"]
    n_pos = (ref_t != 0).sum(0)
    for truth, ref_truth in ((g["labels"], g["labels"][g["target"][:, 21] != 1]), (g["target"], ref_t)):
        got = perframe_average_precision_device(cuda(g["scores"]), cuda(truth), NAMES, post, metric, raw=True)
        hinted = perframe_average_precision_device(cuda(g["scores"]), cuda(truth), NAMES, post, metric, defer=True, raw=True,
                                                   n_valid=ref_t.shape[0])()
        want = perframe_average_precision_device(cuda(ref_p), cuda(ref_truth), NAMES, None, metric, raw=True)
        for a, b, c in zip(got, hinted, want):                        # AP, positives, score sums: the metric kernels saw the same input
            assert same_bits(a, c) and same_bits(b, c)
    ap = got[0]                                                       # of the dense targets, which the reference's reports are about
    assert np.array_equal(got[1], n_pos)
    if metric == "AP":
        ref, ref_mean = g[f"ap_{smooth}{switch}"], float(g[f"mean_ap_{smooth}{switch}"])
    elif not smooth:
        ref, ref_mean = g[f"cap_0{switch}"], float(g[f"mean_cap_0{switch}"])
    else:       # smoothing ties neighbouring frames and the reference leaves ties to chance under cAP: the host form on its arrays
        ref = calibrated_average_precision_columns(ref_p, ref_t != 0)
        ref_mean = float(np.mean(ref[1:21]))
    ok, dev = close(ap[1:21], ref[1:21], n_pos[1:21])
    print(f"{metric} smooth={smooth} switch={switch}: max |device - reference| {dev:.3e}")
    assert ok, (ap, ref)
    assert close(np.mean(ap[1:21]), ref_mean, n_pos[1:21].max())[0]
    host = perframe_average_precision(g["scores"], g["target"], NAMES, post, metric)
    rep = perframe_average_precision_device(cuda(g["scores"]), cuda(g["target"]), NAMES, post, metric)
    assert list(rep["per_class_AP"]) == list(host["per_class_AP"])


@pytest.mark.parametrize("metric", ["AP", "cAP"])
@pytest.mark.parametrize("smooth,switch", [(0, 0), (1, 1)])
def test_perstage_on_device_postprocessed_ids(metric, smooth, switch):
    g = golden()
    post = ThumosPostprocessing(bool(smooth), bool(switch))
    ids_out = g["labels"][g["target"][:, 21] != 1]
    got = perstage_average_precision_device(cuda(g["scores"]), cuda(g["labels"]), NAMES, raw=True, metrics=metric, postprocessing=post)
    hinted = perstage_average_precision_device(cuda(g["scores"]), cuda(g["labels"]), NAMES, raw=True, metrics=metric, postprocessing=post,
                                               n_valid=ids_out.shape[0], defer=True)()
    want = perstage_average_precision_device(cuda(g[f"pred_out_{smooth}{switch}"]), cuda(ids_out), NAMES, raw=True, metrics=metric)
    for a, b, c in zip(got, hinted, want):
        assert same_bits(a, c) and same_bits(b, c)
    plain = perstage_average_precision_device(cuda(g["scores"]), cuda(g["labels"]), NAMES, raw=True, metrics=metric)
    assert not np.array_equal(plain[1], got[1])                       # removing frames changes the runs


class _ThumosLoader:
    """what the reference's test DataLoader yields (batch dim 1, vid as a 1-tuple): 22 classes in runs of 13 frames, class 21 among them"""
    def __init__(self, lens, seed):
        from prego_amd import weights as W
        self.items = []
        for i, T in enumerate(lens):
            rgb = W.tsn_features((T, 2048), seed, f"thumos.rgb.{i}")
            seg = ((np.arange(T) + 5 * i) // 13) % 22
            seg[0] = 21 if i == 0 else seg[0]
            tgt = np.zeros((T, 22), np.float32)
            tgt[np.arange(T), seg] = 1.0
            self.items.append((torch.from_numpy(rgb)[None], torch.zeros(1, T, 2048), torch.from_numpy(tgt)[None],
                               (f"synth_video_{i}",), torch.tensor([0]), torch.tensor([T])))

    def __iter__(self):
        return iter(self.items)


def test_evaluate_with_the_key(tmp_path, monkeypatch):
    """Evaluate on a synthetic THUMOS set with smoothing, the switch and the per-stage report: the metrics run on the device on
    post-processed arrays sized by the host's count, and equal the host path on the scores the pass collected; the output file keeps
    every frame"""
    from prego_amd import weights as W
    from prego_amd.config import epic_tent_cfg
    from prego_amd.registry import build_eval, build_model
    import prego_amd.evaluate
    import prego_amd.model  # noqa: F401
    lens = [300, 111, 64]
    vl = os.path.join(tmp_path, "video_list.json")
    json.dump({"THUMOS": {"class_index": NAMES}}, open(vl, "w"))
    cfg = epic_tent_cfg(data_name="THUMOS", num_classes=22, eval="dummy.pth", video_list_path=vl, compute_dtype="fp16",
                        eval_output_dir=str(tmp_path / "out"), eval_perstage=True, eval_thumos_postprocessing=True, eval_thumos_smooth=True,
                        eval_thumos_switch=True)
    seen = []
    orig = prego_amd.evaluate.thumos_postprocessing_device

    def spy(pred, gt, post, n_valid=None):
        seen.append((pred.cpu().numpy(), gt.cpu().numpy(), post, n_valid))
        return orig(pred, gt, post, n_valid)
    monkeypatch.setattr(prego_amd.evaluate, "thumos_postprocessing_device", spy)
    model = build_model(cfg, "cuda:0")
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_state_dict(cfg, 20, head_gain=8.0).items()})
    ev = build_eval(cfg)
    loader = _ThumosLoader(lens, 20)
    mean = ev(model, loader, logging.getLogger("t"), "cuda:0")
    assert ev.last_metric_path == "device"
    assert len(seen) == 1                                             # post-processed once for both metrics
    pred, labels, post, hint = seen[0]
    assert pred.shape == (sum(lens), 22) and labels.shape == (sum(lens),) and post.smooth and post.switch
    assert hint == int((labels != 21).sum()) and 0 < hint < sum(lens)  # counted on the host: nothing waited for the device's count
    host = perframe_average_precision(pred, onehot(labels, 22), NAMES, post, "AP")
    assert close(mean, host["mean_AP"], hint)[0], (mean, host["mean_AP"])
    assert abs(mean - perframe_average_precision(pred, onehot(labels, 22), NAMES, None, "AP")["mean_AP"]) > 1e-6
    host_stage = perstage_average_precision(pred, labels, NAMES, post, "AP")
    assert list(ev.last_perstage) == list(STAGE_NAMES)
    assert all(abs(ev.last_perstage[s]["mean_AP"] - host_stage[s]["mean_AP"]) < 1e-12 for s in STAGE_NAMES)
    js = json.load(open(tmp_path / "out" / "output_miniROAD.json"))
    for i, T in enumerate(lens):                                      # nothing is removed there
        ent = js[f"synth_video_{i}"]
        assert len(ent["pred"]) == len(ent["gt"]) == T
        assert ent["gt"] == np.argmax(loader.items[i][2][0].numpy(), 1).tolist()


def test_ant_evaluate_with_the_key(tmp_path, monkeypatch):
    """AntEvaluate with MiniROADA on the tiny THUMOS tree: every report on the device, the step slices handed over as strided views
    with the host's counts, each report equal to the host form's on the same scores"""
    import prego_amd.data  # noqa: F401
    import prego_amd.evaluate
    import prego_amd.model  # noqa: F401
    from prego_amd import weights as W
    from prego_amd.registry import DATA_LAYERS, EVAL, build_model
    from tests.helpers.thumos_tree import L, NAMES as TREE_NAMES, make_thumos_tree
    cfg = make_thumos_tree(str(tmp_path), compute_dtype="fp32", eval_thumos_postprocessing=True, eval_thumos_smooth=True)
    loader = torch.utils.data.DataLoader(DATA_LAYERS[cfg["data_name"]](cfg, "test"), batch_size=1, shuffle=False)
    m = build_model(cfg, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0).items()})
    m.eval()
    seen = []
    orig = prego_amd.evaluate.perframe_average_precision_device

    def spy(pred, truth, *a, **k):
        rep = orig(pred, truth, *a, **k)
        seen.append((pred.is_contiguous(), pred.cpu().numpy(), truth.cpu().numpy(), a[1], k.get("n_valid"), rep))
        return rep
    monkeypatch.setattr(prego_amd.evaluate, "perframe_average_precision_device", spy)
    ev = EVAL["ANTICIPATION"](cfg)
    mean = ev(m, loader, logging.getLogger("t"), "cuda:0")
    assert ev.last_metric_path == "device" and len(seen) == 1 + L
    reports = [ev.result] + [ev.result[f"anticipation_{l + 1}"] for l in range(L)]
    for k, ((contig, pred, truth, post, hint, rep), got) in enumerate(zip(seen, reports)):
        assert isinstance(post, ThumosPostprocessing) and post.smooth and not post.switch
        assert contig == (k == 0)                                     # a step is a [:, l, :] view: no copy in front of the C entry
        assert hint == int((truth[:, 21] != 1).sum()) and 0 < hint < truth.shape[0]
        want = perframe_average_precision(pred, truth, TREE_NAMES, post, "AP")
        assert list(rep["per_class_AP"]) == list(want["per_class_AP"])
        n_pos = (post(truth, pred)[0] != 0).sum(0)
        for c, name in enumerate(TREE_NAMES):
            if name in want["per_class_AP"]:
                assert close(rep["per_class_AP"][name], want["per_class_AP"][name], n_pos[c])[0], (k, name)
        assert close(rep["mean_AP"], want["mean_AP"], n_pos.max())[0] and got["mean_AP"] == rep["mean_AP"]
    assert mean == np.mean([r["mean_AP"] for r in reports[1:]])
