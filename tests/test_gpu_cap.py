"""GPU: calibrated average precision on the device (prego_perframe_cap(_labels), prego_perstage_cap_labels, csrc/metrics.hip)
against the reference's figures (tests/golden/cap_mixed.npz) and against the host forms
(prego_amd.metrics.calibrated_average_precision_columns, perstage_ap_raw(.., 'cAP'), which tests/test_cap_cpu.py holds to the
reference and to the integer-rank formulas); long tie runs; the C entries' refusals; `Evaluate` / `AntEvaluate` with metric 'cAP'.

Tolerance: (P + 16) * 2^-52 per value, P = the positives in that sum (tests/test_cap_cpu.py says why).  NaN must match NaN."""
import ctypes as C
import json
import logging
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd.metrics import (STAGE_NAMES, calibrated_average_precision_columns, perframe_ap_raw_device,      # noqa: E402
                               perframe_average_precision, perframe_average_precision_device, perstage_ap_raw,
                               perstage_average_precision, perstage_average_precision_device)
from .test_cap_cpu import EDGES, close, edge_scores, golden, onehot, run_labels, tol                             # noqa: E402

EINVAL, EWORKSPACE = -1, -3


def _frame(scores, truth):
    """device per-frame cAP: (cAP, positives, score mass) of host arrays; truth = dense targets [n, C] or ids [n]"""
    return perframe_ap_raw_device(torch.from_numpy(scores).cuda(), torch.from_numpy(truth).cuda(), "cAP")


def _stage(scores, labels):
    names = [f"c{i}" for i in range(scores.shape[1])]
    return perstage_average_precision_device(torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda(), names, raw=True,
                                             metrics="cAP")


def _check_frame(scores, truth, what):
    pos = truth != 0 if truth.ndim == 2 else onehot(truth, scores.shape[1]) != 0
    cap, n_pos, mass = _frame(scores, truth)
    want = calibrated_average_precision_columns(scores, pos)
    ok, dev = close(cap, want, pos.sum(0))
    print(f"{what}: per-frame max |device - host| {dev:.3e}")
    assert np.array_equal(n_pos, pos.sum(0))
    assert np.allclose(mass, scores.sum(0, dtype=np.float64), rtol=1e-9, atol=1e-9)
    assert ok, (what, cap, want)
    return cap


def _check_stage(scores, labels, what):
    cap, n_pos = _stage(scores, labels)
    want, want_pos = perstage_ap_raw(scores, labels, "cAP")
    ok, dev = close(cap, want, want_pos)
    print(f"{what}: per-stage max |device - host| {dev:.3e}")
    assert np.array_equal(n_pos, want_pos)
    assert ok, what
    return cap


def test_golden_fixture():
    g = golden()
    scores, labels = g["scores"], g["labels"]
    ncls = scores.shape[1]
    pos = onehot(labels, ncls) != 0
    cap = _check_frame(scores, labels, "golden")
    ok, dev = close(cap, g["cap"], pos.sum(0))
    print("golden: per-frame max |device - reference|", dev)
    assert ok and np.isnan(cap[6])
    stage = _check_stage(scores, labels, "golden")
    ok, dev = close(stage, g["stage_cap"], perstage_ap_raw(scores, labels, "cAP")[1])
    print("golden: per-stage max |device - reference|", dev)
    assert ok and np.isnan(stage[:, 6]).all()
    names = [f"c{i}" for i in range(ncls)]
    rep = perframe_average_precision_device(torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda(), names, None, "cAP")
    assert list(rep["per_class_AP"]) == [names[c] for c in range(1, ncls) if c != 6]
    assert abs(rep["mean_AP"] - float(g["mean_cap"])) <= tol(pos.sum(0).max())
    srep = perstage_average_precision_device(torch.from_numpy(scores).cuda(), torch.from_numpy(labels).cuda(), names, metrics="cAP")
    assert list(srep) == list(STAGE_NAMES) and all(list(srep[s]["per_class_AP"]) == names[1:] for s in STAGE_NAMES)


@pytest.mark.parametrize("levels", [0, 3])                       # tie-free, and every column three long tie runs
@pytest.mark.parametrize("n,ncls", EDGES)                        # radix tile and column-block edges
def test_tile_edges_vs_host(n, ncls, levels):
    rng = np.random.default_rng(1000 * levels + n + ncls)
    scores = edge_scores(rng, n, ncls, levels)
    labels = run_labels(rng, n, ncls)
    what = f"n {n} C {ncls} levels {levels}"
    _check_frame(scores, labels, what)
    _check_stage(scores, labels, what)


def test_columns_that_are_one_tie_run():
    rng = np.random.default_rng(21)
    n, ncls = 5003, 5
    scores = rng.random((n, ncls)).astype(np.float32)
    scores[:, 0] = 0.375                                                          # constant
    scores[:, 1] = (rng.random(n) < 0.5).astype(np.float32)                       # exact 0.0 / 1.0 only
    scores[:, 2] = np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(np.float32)    # +0.0 and -0.0 are one tie run
    scores[:, 3] = 1.0
    dense = (rng.random((n, ncls)) < 0.2).astype(np.float32)
    dense[:, 3] = 1.0                                                             # positive on every frame: w = 0
    cap = _check_frame(scores, dense, "tie runs, dense targets")
    assert abs(cap[3] - 1.0) <= tol(n)
    labels = run_labels(rng, n, ncls)
    _check_frame(scores, labels, "tie runs, ids")
    _check_stage(scores, labels, "tie runs, ids")


@pytest.mark.parametrize("n,ncls", [(140_000, 2), (90_000, 70)])
def test_more_positives_than_the_owned_ranges(n, ncls):
    """one class positive on every frame.  (90 000, 70): 16 workgroups per class own 16 x 5 456 = 87 296 composites, so this class
    takes ap_count's fallback (the sampled table and one device atomic per entry); (140 000, 2) has 64 workgroups per class"""
    rng = np.random.default_rng(n)
    scores = (rng.integers(0, 5, (n, ncls)) / np.float32(4)).astype(np.float32)
    dense = (rng.random((n, ncls)) < 0.01).astype(np.float32)
    dense[:, ncls - 1] = 1.0
    cap = _check_frame(scores, dense, f"n {n} C {ncls}, dense")
    assert abs(cap[ncls - 1] - 1.0) <= tol(n)
    if ncls == 2:                                                                 # one run over every frame, per stage
        _check_stage(scores, np.full(n, 1, np.int32), f"n {n} C {ncls}, one run")


def test_dense_targets_and_ids_give_the_same_bits():
    rng = np.random.default_rng(4)
    n, ncls = 6007, 100
    scores = np.round(rng.random((n, ncls)), 2).astype(np.float32)
    labels = run_labels(rng, n, ncls)
    a, b = _frame(scores, labels), _frame(scores, onehot(labels, ncls))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_two_calls_give_the_same_bits():
    rng = np.random.default_rng(8)
    n, ncls = 6000, 9
    scores = np.round(rng.random((n, ncls)), 1).astype(np.float32)
    labels = run_labels(rng, n, ncls)
    a, b = _frame(scores, labels), _frame(scores, labels)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    a, b = _stage(scores, labels), _stage(scores, labels)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _call_frame(lib, dense, scores, truth, n, ncls, ap, n_pos, mass, ws, ws_bytes):
    fn = lib.prego_perframe_cap if dense else lib.prego_perframe_cap_labels
    rc = fn(_p(scores), _p(truth), n, ncls, _p(ap), _p(n_pos), _p(mass), _p(ws), ws_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _call_stage(lib, scores, labels, n, ncls, ap, n_pos, ws, ws_bytes):
    rc = lib.prego_perstage_cap_labels(_p(scores), _p(labels), n, ncls, _p(ap), _p(n_pos), _p(ws), ws_bytes,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def test_worst_case_lists_stay_inside_the_queried_workspace():
    """per frame: every entry of a dense target matrix positive (every class's list is n long); per stage: every run one frame long
    (every positive is in all ten stages)"""
    from prego_amd import _lib
    lib = _lib.load()
    n, ncls, guard = 5001, 3, 4096
    rng = np.random.default_rng(11)
    pr = np.round(rng.random((n, ncls)), 2).astype(np.float32)
    dense = np.ones((n, ncls), np.float32)
    need = lib.prego_perframe_cap_workspace_bytes(n, ncls)
    assert need > lib.prego_perframe_ap_workspace_bytes(n, ncls)
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.zeros((3, ncls), dtype=torch.float64, device="cuda")
    cnt = torch.zeros(ncls, dtype=torch.int64, device="cuda")
    assert _call_frame(lib, True, torch.from_numpy(pr).cuda(), torch.from_numpy(dense).cuda(), n, ncls, out[0], cnt, out[2], ws, need) == 0
    assert bool((ws[need:] == 0xA5).all())
    assert cnt.tolist() == [n] * ncls
    assert close(out[0].cpu().numpy(), calibrated_average_precision_columns(pr, dense != 0), [n] * ncls)[0]
    labels = (1 + np.arange(n) % 2).astype(np.int32)
    need = lib.prego_perstage_cap_workspace_bytes(n, ncls)
    assert need > lib.prego_perframe_cap_workspace_bytes(n, ncls)
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.zeros((10, ncls), dtype=torch.float64, device="cuda")
    cnt = torch.zeros((10, ncls), dtype=torch.int64, device="cuda")
    assert _call_stage(lib, torch.from_numpy(pr).cuda(), torch.from_numpy(labels).cuda(), n, ncls, out, cnt, ws, need) == 0
    assert bool((ws[need:] == 0xA5).all())
    host, host_pos = perstage_ap_raw(pr, labels, "cAP")
    assert np.array_equal(cnt.cpu().numpy(), host_pos) and host_pos[:, 2].tolist() == [n // 2] * 10
    assert close(out.cpu().numpy(), host, host_pos)[0]


def test_refusals_leave_outputs_and_workspace_untouched():
    from prego_amd import _lib
    from prego_amd._lib import PregoError
    lib = _lib.load()
    n, ncls = 100, 4
    pr = torch.rand(n, ncls, device="cuda")
    lab = torch.randint(0, ncls, (n,), dtype=torch.int32, device="cuda")
    tgt = torch.nn.functional.one_hot(lab.long(), ncls).float()
    # ---- per frame, both entries
    need = lib.prego_perframe_cap_workspace_bytes(n, ncls)
    assert lib.prego_perframe_cap_workspace_bytes(0, ncls) == 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((ncls,), -7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((ncls,), -7, dtype=torch.int64, device="cuda")
    mass = torch.full((ncls,), -7.0, dtype=torch.float64, device="cuda")
    for dense, truth in ((True, tgt), (False, lab)):
        for args, rc in [((None, truth, n, ncls, out, cnt, mass, ws, need), EINVAL), ((pr, None, n, ncls, out, cnt, mass, ws, need), EINVAL),
                         ((pr, truth, n, ncls, None, cnt, mass, ws, need), EINVAL), ((pr, truth, n, ncls, out, cnt, mass, None, need), EINVAL),
                         ((pr, truth, n, 0, out, cnt, mass, ws, need), EINVAL), ((pr, truth, -1, ncls, out, cnt, mass, ws, need), EINVAL),
                         ((pr, truth, 1 << 31, ncls, out, cnt, mass, ws, need), EINVAL),
                         ((pr, truth, n, ncls, out, cnt, mass, ws, need - 1), EWORKSPACE)]:
            assert _call_frame(lib, dense, *args) == rc, args[2:4]
            assert bool((out == -7.0).all()) and bool((cnt == -7).all()) and bool((mass == -7.0).all()) and bool((ws == 0x5A).all())
        assert b"prego_perframe_cap_workspace_bytes" in lib.prego_last_error()
        assert _call_frame(lib, dense, pr, truth, n, ncls, out, None, None, ws, need) == 0      # n_pos and score_sum are optional
        assert bool((cnt == -7).all()) and bool((mass == -7.0).all()) and not bool((out == -7.0).any())
        out.fill_(-7.0)
        ws.fill_(0x5A)
        assert _call_frame(lib, dense, pr, truth, 0, ncls, out, cnt, mass, None, 0) == 0        # no frames: NaN, no positives, no mass
        assert bool(torch.isnan(out).all()) and bool((cnt == 0).all()) and bool((mass == 0.0).all())
        out.fill_(-7.0)
        cnt.fill_(-7)
        mass.fill_(-7.0)
    # ---- per stage
    need = lib.prego_perstage_cap_workspace_bytes(n, ncls)
    assert lib.prego_perstage_cap_workspace_bytes(0, ncls) == 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    out = torch.full((10, ncls), -7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((10, ncls), -7, dtype=torch.int64, device="cuda")
    for args, rc in [((None, lab, n, ncls, out, cnt, ws, need), EINVAL), ((pr, None, n, ncls, out, cnt, ws, need), EINVAL),
                     ((pr, lab, n, ncls, None, cnt, ws, need), EINVAL), ((pr, lab, n, ncls, out, cnt, None, need), EINVAL),
                     ((pr, lab, n, 0, out, cnt, ws, need), EINVAL), ((pr, lab, -1, ncls, out, cnt, ws, need), EINVAL),
                     ((pr, lab, n, ncls, out, cnt, ws, need - 1), EWORKSPACE)]:
        assert _call_stage(lib, *args) == rc, args[2:4]
        assert bool((out == -7.0).all()) and bool((cnt == -7).all()) and bool((ws == 0x5A).all())
    assert b"prego_perstage_cap_workspace_bytes" in lib.prego_last_error()
    assert _call_stage(lib, pr, lab, n, ncls, out, None, ws, need) == 0             # n_pos is optional
    assert bool((cnt == -7).all()) and not bool((out == -7.0).any())
    out.fill_(-7.0)
    assert _call_stage(lib, pr, lab, 0, ncls, out, cnt, None, 0) == 0               # no frames: no error, zeros
    assert bool((out == 0.0).all()) and bool((cnt == 0).all())
    # ---- the Python entries
    names = ["a", "b", "c"]
    with pytest.raises(PregoError):                                                 # THUMOS post-processing stays refused
        perframe_average_precision_device(torch.zeros(4, 3, device="cuda"), torch.zeros(4, 3, device="cuda"), names, lambda g, p: (g, p), "cAP")
    with pytest.raises(PregoError):
        perframe_average_precision_device(torch.zeros(4, 3, device="cuda"), torch.zeros(4, 3, device="cuda"), names, None, "mAP")
    with pytest.raises(PregoError):
        perstage_average_precision_device(torch.zeros(4, 3, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda"), names, metrics="mAP")
    with pytest.raises(PregoError):
        perstage_average_precision_device(torch.zeros(4, 3), torch.zeros(4, dtype=torch.int32), names, metrics="cAP")


def _same_report(got, want, n_pos_by_name):
    assert list(got["per_class_AP"]) == list(want["per_class_AP"])
    worst = 0.0
    for name, v in want["per_class_AP"].items():
        ok, dev = close(got["per_class_AP"][name], v, n_pos_by_name[name])
        assert ok, (name, got["per_class_AP"][name], v)
        worst = max(worst, dev)
    ok, dev = close(got["mean_AP"], want["mean_AP"], max(n_pos_by_name.values()))
    assert ok
    return max(worst, dev)


def test_evaluate_computes_cap_on_the_device(tmp_path, monkeypatch):
    """metric 'cAP' and eval_perstage_metric 'cAP' on three short synthetic videos: the reports are the host functions' on the scores
    the pass collected; with eval_perstage_metric unset the per-stage report is bit for bit the AP report"""
    from prego_amd import weights as W
    from prego_amd.config import epic_tent_cfg
    from prego_amd.registry import build_model, build_eval
    import prego_amd.model, prego_amd.evaluate  # noqa: F401
    from .test_gpu_evaluate import _Loader
    lens = [300, 111, 64]
    names = [f"c{i}" for i in range(12)]
    vl = os.path.join(tmp_path, "video_list.json")
    json.dump({"EPIC-TENT-O": {"class_index": names}}, open(vl, "w"))
    seen = []
    orig = prego_amd.evaluate.perframe_average_precision_device

    def spy(pred, truth, *a, **k):
        fn = orig(pred, truth, *a, **k)
        rec = {"pred": pred.cpu().numpy(), "truth": truth.cpu().numpy(), "metric": a[2]}
        seen.append(rec)

        def finish():
            rec["report"] = fn()
            return rec["report"]
        return finish
    monkeypatch.setattr(prego_amd.evaluate, "perframe_average_precision_device", spy)
    res = {}
    for stage_metric in ("cAP", None):
        out_dir = tmp_path / f"out_{stage_metric}"
        over = {"eval_perstage_metric": stage_metric} if stage_metric else {}
        cfg = epic_tent_cfg(eval="dummy.pth", video_list_path=vl, compute_dtype="fp16", eval_output_dir=str(out_dir), metric="cAP",
                            eval_perstage=True, **over)
        model = build_model(cfg, "cuda:0")
        model.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_state_dict(cfg, 20, head_gain=8.0).items()})
        ev = build_eval(cfg)
        assert ev.last_metric_path is None
        mean = ev(model, _Loader(lens, 12, 20), logging.getLogger("t"), "cuda:0")
        assert ev.last_metric_path == "device"
        res[stage_metric] = (mean, ev.last_perstage)
    assert len(seen) == 2 and all(r["metric"] == "cAP" for r in seen)
    pred, labels = seen[0]["pred"], seen[0]["truth"]
    assert pred.shape == (sum(lens), 12) and labels.shape == (sum(lens),) and np.array_equal(pred, seen[1]["pred"])
    n_pos = {names[c]: int((labels == c).sum()) for c in range(12)}
    want = perframe_average_precision(pred, onehot(labels, 12), names, None, "cAP")
    print("Evaluate: per-frame max |device - host|", _same_report(seen[0]["report"], want, n_pos))
    assert res["cAP"][0] == seen[0]["report"]["mean_AP"] == res[None][0]
    want_stage, stage_pos = perstage_ap_raw(pred, labels, "cAP")
    got = res["cAP"][1]
    assert list(got) == list(STAGE_NAMES)
    for s, stage in enumerate(STAGE_NAMES):
        assert list(got[stage]["per_class_AP"]) == names[1:]
        for c in range(1, 12):
            assert close(got[stage]["per_class_AP"][names[c]], want_stage[s, c], stage_pos[s, c])[0], (stage, c)
    today = perstage_average_precision_device(torch.from_numpy(pred).cuda(), torch.from_numpy(labels).cuda(), names)       # metric 'AP'
    assert json.dumps(res[None][1]) == json.dumps(today)
    host_ap = perstage_average_precision(pred, labels, names)
    assert all(abs(res[None][1][s]["mean_AP"] - host_ap[s]["mean_AP"]) < 1e-12 for s in STAGE_NAMES)


def test_ant_evaluate_computes_cap_on_the_device(tmp_path, monkeypatch):
    """AntEvaluate on a small MiniROADA (hidden_dim 512, anticipation_length 2), metric 'cAP': the OAD report and every anticipation
    step's report are the host function's on the same scores"""
    import prego_amd.data  # noqa: F401
    import prego_amd.evaluate  # noqa: F401
    import prego_amd.model  # noqa: F401
    from prego_amd import weights as W
    from prego_amd.registry import DATA_LAYERS, EVAL, build_model
    from scripts.gen_golden_anticipation import make_tree, tree_cfg
    make_tree(str(tmp_path))
    cfg = tree_cfg(str(tmp_path), metric="cAP", anticipation_length=2, compute_dtype="fp32")
    assert cfg["hidden_dim"] == 512
    loader = torch.utils.data.DataLoader(DATA_LAYERS[cfg["data_name"]](cfg, "test"), batch_size=1, shuffle=False)
    m = build_model(cfg, "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0).items()})
    m.eval()
    seen = []
    orig = prego_amd.evaluate.perframe_average_precision_device

    def spy(pred, truth, *a, **k):
        rep = orig(pred, truth, *a, **k)
        seen.append((pred.cpu().numpy(), truth.cpu().numpy(), a[2], rep))
        return rep
    monkeypatch.setattr(prego_amd.evaluate, "perframe_average_precision_device", spy)
    ev = EVAL["ANTICIPATION"](cfg)
    mean = ev(m, loader, logging.getLogger("t"), "cuda:0")
    assert ev.last_metric_path == "device"
    assert len(seen) == 3 and all(s[2] == "cAP" for s in seen)                    # the OAD scores and two anticipation steps
    names = ev.all_class_names
    reports = [ev.result] + [ev.result[f"anticipation_{l + 1}"] for l in range(2)]
    for (pred, truth, _m, rep), got in zip(seen, reports):
        assert pred.shape == truth.shape and pred.shape[1] == len(names) and pred.shape[0] > 0
        want = perframe_average_precision(pred, truth, names, None, "cAP")
        n_pos = {names[c]: int((truth[:, c] != 0).sum()) for c in range(len(names))}
        print("AntEvaluate: max |device - host|", _same_report(rep, want, n_pos))
        assert got["mean_AP"] == rep["mean_AP"]
    assert mean == np.mean([r["mean_AP"] for r in reports[1:]])
