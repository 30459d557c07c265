"""CPU: the THUMOS post-processing (prego_amd/postprocessing.py) against what the REFERENCE's thumos_postprocessing and metrics made of
tests/golden/thumos_post.npz (scripts/gen_thumos_golden.py), and the evaluators' opt-in key.

The post-processing is comparisons and copies: its outputs are held to the reference's bit for bit.  The reports are held to 1e-12
(the host metrics' bound against sklearn in the other CPU tests)."""
import os

import numpy as np
import pytest

from prego_amd.metrics import (perframe_average_precision, perstage_ap_raw, perstage_average_precision, perstage_report)
from prego_amd.postprocessing import ThumosPostprocessing, thumos_postprocessing

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATH = os.path.join(G, "thumos_post.npz")
COMBOS = [(0, 0), (0, 1), (1, 0), (1, 1)]
NAMES21 = [f"c{i}" for i in range(21)]          # the classes the reference was asked for (the fixture's script says why)


def golden():
    g = np.load(PATH)
    return {k: g[k] for k in g.files}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_fixture_is_small_and_says_what_the_tests_need():
    assert os.path.getsize(PATH) < 150_000
    g = golden()
    amb = g["target"][:, 21] == 1
    assert g["scores"].shape == (600, 22) and np.unique(g["scores"]).size == 13200
    assert 0.05 <= amb.mean() <= 0.10 and amb[0] and amb[-1] and amb[127:129].all() and amb[255:258].all()
    assert (g["target"][:, 21] == 0.5).sum() == 2 and np.array_equal(g["labels"] == 21, amb)
    assert g["gt_out"].shape[0] == (~amb).sum()


@pytest.mark.parametrize("smooth,switch", COMBOS)
def test_host_form_equals_the_reference_bit_for_bit(smooth, switch):
    g = golden()
    sc, tg, lab = g["scores"].copy(), g["target"].copy(), g["labels"].copy()
    gt, pr = thumos_postprocessing(tg, sc, smooth=bool(smooth), switch=bool(switch))
    assert same_bits(gt, g["gt_out"]) and same_bits(pr, g[f"pred_out_{smooth}{switch}"])
    ids, pr2 = thumos_postprocessing(lab, sc, smooth=bool(smooth), switch=bool(switch))
    assert same_bits(ids, g["labels"][g["target"][:, 21] != 1]) and same_bits(pr2, pr)
    gt3, pr3 = ThumosPostprocessing(bool(smooth), bool(switch))(tg, sc)
    assert same_bits(gt3, gt) and same_bits(pr3, pr)
    # the arguments are never written (the reference writes its prediction with switch and no smooth)
    assert same_bits(sc, g["scores"]) and same_bits(tg, g["target"]) and same_bits(lab, g["labels"])
    assert not np.shares_memory(pr, sc)


def _by_definition(pred, smooth, switch):
    """the header's formula, one element at a time"""
    n = pred.shape[0]
    out = pred.copy()
    if smooth:
        for i in range(n):
            for d in (-1, 1, -2, 2):
                j = i + d if 0 <= i + d < n else i
                out[i] = np.maximum(out[i], pred[j])
    if switch:
        out[:, 8] = np.maximum(out[:, 5], out[:, 8])
    return out


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("smooth,switch", COMBOS)
def test_tiny_inputs(n, smooth, switch):
    rng = np.random.default_rng(n)
    pred = rng.random((n, 22)).astype(np.float32)
    tgt = np.zeros((n, 22), np.float32)
    tgt[np.arange(n), rng.integers(0, 21, n)] = 1
    gt, pr = thumos_postprocessing(tgt, pred, smooth=bool(smooth), switch=bool(switch))
    assert same_bits(gt, tgt) and same_bits(pr, _by_definition(pred, smooth, switch))
    tgt[:, 21] = 1                                                    # every frame ambiguous
    gt, pr = thumos_postprocessing(tgt, pred, smooth=bool(smooth), switch=bool(switch))
    assert gt.shape == (0, 22) and pr.shape == (0, 22)
    rep = perframe_average_precision(pred, tgt, [f"c{i}" for i in range(22)], ThumosPostprocessing(bool(smooth), bool(switch)), "AP")
    assert not rep["per_class_AP"] and np.isnan(rep["mean_AP"])


def test_options_of_the_object():
    rng = np.random.default_rng(5)
    pred = rng.random((9, 6)).astype(np.float32)
    ids = np.array([0, 3, 3, 1, 5, 3, 2, 2, 3], np.int32)
    post = ThumosPostprocessing(switch=True, switch_from=1, switch_to=4, ambiguous=3)
    got_ids, got = post(ids, pred)
    want = pred.copy()
    want[:, 4] = np.maximum(pred[:, 1], pred[:, 4])
    assert same_bits(got_ids, ids[ids != 3]) and same_bits(got, want[ids != 3]) and post.count_valid(ids) == 5
    keep_all = ThumosPostprocessing(ambiguous=-1)
    assert same_bits(keep_all(ids, pred)[1], pred) and keep_all.count_valid(ids) == 9
    dense = np.eye(6, dtype=np.float32)[ids]
    dense[0, 3] = 0.5                                                 # not 1: kept
    assert post.count_valid(dense) == 5 and post(dense, pred)[0].shape == (5, 6)


@pytest.mark.parametrize("smooth,switch", COMBOS)
def test_host_ap_reports_match_the_reference(smooth, switch):
    g = golden()
    rep = perframe_average_precision(g["scores"], g["target"], NAMES21, ThumosPostprocessing(bool(smooth), bool(switch)), "AP")
    want = g[f"ap_{smooth}{switch}"]
    assert list(rep["per_class_AP"]) == NAMES21[1:]
    dev = max(abs(rep["per_class_AP"][f"c{c}"] - want[c]) for c in range(1, 21))
    print(f"AP smooth={smooth} switch={switch}: max |host - reference| {dev:.3e}")
    assert dev <= 1e-12 and abs(rep["mean_AP"] - float(g[f"mean_ap_{smooth}{switch}"])) <= 1e-12


@pytest.mark.parametrize("switch", [0, 1])
def test_host_cap_reports_match_the_reference_without_smoothing(switch):
    g = golden()
    rep = perframe_average_precision(g["scores"], g["target"], NAMES21, ThumosPostprocessing(False, bool(switch)), "cAP")
    want = g[f"cap_0{switch}"]
    dev = max(abs(rep["per_class_AP"][f"c{c}"] - want[c]) for c in range(1, 21))
    print(f"cAP switch={switch}: max |host - reference| {dev:.3e}")
    assert dev <= 1e-12 and abs(rep["mean_AP"] - float(g[f"mean_cap_0{switch}"])) <= 1e-12


@pytest.mark.parametrize("smooth,switch", [(0, 0), (1, 1)])
def test_host_perstage_report_on_postprocessed_ids(smooth, switch):
    """removing a frame makes its neighbours adjacent: the runs are those of the frames that are left"""
    g = golden()
    names = [f"c{i}" for i in range(22)]
    rep = perstage_average_precision(g["scores"], g["labels"], names, ThumosPostprocessing(bool(smooth), bool(switch)), "AP")
    ids_out = g["labels"][g["target"][:, 21] != 1]
    want = perstage_report(perstage_ap_raw(g[f"pred_out_{smooth}{switch}"], ids_out, "AP")[0], names)
    assert rep == want
    plain = perstage_average_precision(g["scores"], g["labels"], names, None, "AP")
    assert plain != rep


class _Log:
    def info(self, *a, **k):
        pass


def test_evaluators_refuse_thumos_without_the_key_and_the_key_elsewhere(tmp_path):
    import prego_amd.evaluate  # noqa: F401
    from prego_amd._lib import PregoError
    from prego_amd.registry import EVAL
    from tests.helpers.thumos_tree import make_thumos_tree
    cfg = make_thumos_tree(str(tmp_path))
    for name, data_name in (("ANTICIPATION", "THUMOS_ANTICIPATION"), ("OAD", "THUMOS")):
        with pytest.raises(NotImplementedError, match="eval_thumos_postprocessing"):
            EVAL[name](dict(cfg, data_name=data_name))
        ev = EVAL[name](dict(cfg, data_name=data_name, eval_thumos_postprocessing=True))
        post = ev.data_processing
        assert isinstance(post, ThumosPostprocessing) and not post.smooth and not post.switch and post.ambiguous == 21
        ev = EVAL[name](dict(cfg, data_name=data_name, eval_thumos_postprocessing=True, eval_thumos_smooth=True, eval_thumos_switch=True))
        assert ev.data_processing.smooth and ev.data_processing.switch
    from scripts.gen_golden_anticipation import make_tree
    other = make_tree(str(tmp_path / "tv"))
    for name in ("ANTICIPATION", "OAD"):
        with pytest.raises(PregoError, match="THUMOS"):
            EVAL[name](dict(other, eval_thumos_postprocessing=True))
        assert EVAL[name](other).data_processing is None


@pytest.mark.parametrize("smooth,switch", [(False, False), (True, True)])
def test_ant_evaluate_with_the_key_on_a_cpu_stand_in(tmp_path, smooth, switch):
    """every report is the host metric on arrays post-processed with that report's own targets: target[:, 21] for the OAD scores,
    ant_target[:, l, 21] for step l (eval.py:92-93 passes each step's slice)"""
    torch = pytest.importorskip("torch")
    import prego_amd.data  # noqa: F401
    import prego_amd.evaluate  # noqa: F401
    from prego_amd.registry import DATA_LAYERS, EVAL
    from scripts.gen_golden_anticipation import StandIn
    from tests.helpers.thumos_tree import C, L, NAMES, make_thumos_tree
    cfg = make_thumos_tree(str(tmp_path), eval_thumos_postprocessing=True, eval_thumos_smooth=smooth, eval_thumos_switch=switch)
    ds = DATA_LAYERS[cfg["data_name"]](cfg, "test")
    model = StandIn(C, L).eval()
    ev = EVAL["ANTICIPATION"](cfg)
    mean = ev(model, torch.utils.data.DataLoader(ds, batch_size=1, shuffle=False), _Log(), "cpu")
    assert ev.last_metric_path == "host"
    preds, gts, apreds, agts = [], [], [], []
    with torch.no_grad():
        for i in range(len(ds)):
            rgb, flow, t, at = ds[i]
            out = model(rgb[None], flow[None])
            preds.append(out["logits"][0].numpy()); gts.append(t.numpy())
            apreds.append(out["anticipation_logits"][0].numpy()); agts.append(at.numpy())
    pred, gt, apred, agt = (np.concatenate(x) for x in (preds, gts, apreds, agts))
    assert (gt[:, 21] == 1).any() and any(not np.array_equal(agt[:, l, 21], gt[:, 21]) for l in range(L))
    g_, p_ = thumos_postprocessing(gt, pred, smooth=smooth, switch=switch)
    want = perframe_average_precision(p_, g_, NAMES, None, "AP")
    assert ev.result["mean_AP"] == want["mean_AP"] and dict(ev.result["per_class_AP"]) == dict(want["per_class_AP"])
    steps = []
    for l in range(L):
        g_, p_ = thumos_postprocessing(agt[:, l], apred[:, l], smooth=smooth, switch=switch)
        assert 0 < g_.shape[0] < gt.shape[0]
        want = perframe_average_precision(p_, g_, NAMES, None, "AP")
        assert ev.result[f"anticipation_{l + 1}"]["mean_AP"] == want["mean_AP"]
        steps.append(want["mean_AP"])
        unprocessed = perframe_average_precision(apred[:, l], agt[:, l], NAMES, None, "AP")
        assert unprocessed["mean_AP"] != want["mean_AP"]
    assert mean == np.mean(steps)
