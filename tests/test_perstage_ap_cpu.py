"""CPU: the host form of per-stage average precision (prego_amd.metrics.perstage_average_precision, the reference's
utils/metrics.py:64-130) against the figures the reference itself produced (tests/golden/perstage_ap_mixed.npz, written by
scripts/gen_perstage_golden.py) and against sklearn on stage sets built by a naive per-run loop."""
import os
import warnings

import numpy as np
import pytest

from prego_amd.metrics import (STAGE_NAMES, calibrated_average_precision_columns, perstage_ap_raw, perstage_average_precision,
                               stage_members)

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-12                                    # the project's AP tolerance (test_device_average_precision_kernel_vs_sklearn)


def _golden():
    g = np.load(os.path.join(G, "perstage_ap_mixed.npz"))
    return g["scores"], g["labels"], g["ap"], g["mean_ap"], [str(x) for x in g["stage_names"]]


def _onehot(labels, C):
    m = np.zeros((labels.shape[0], C), np.float32)
    ok = (labels >= 0) & (labels < C)
    m[np.arange(labels.shape[0])[ok], labels[ok]] = 1
    return m


def naive_stage_sets(g, s):
    """frame indices of the sample set of stage s for one class (g: 0 / 1 per frame) and which of them are positives: one Python
    step per frame and per run, Python's own int * float product"""
    n = len(g)
    neg = [i for i in range(n) if not g[i]]
    pos = []
    i = 0
    while i < n:
        if g[i]:
            a = i
            while i + 1 < n and g[i + 1]:
                i += 1
            length = i - a
            lo = a + int(length * (s / 10))
            hi = max(lo + 1, a + int(length * ((s + 1) / 10)))
            pos += list(range(lo, hi))
        i += 1
    return np.array(neg + pos, dtype=np.int64), np.array([0] * len(neg) + [1] * len(pos))


def test_host_matches_the_reference_fixture():
    scores, labels, want, want_mean, stages = _golden()
    C = scores.shape[1]
    names = [f"c{i}" for i in range(C)]
    ap, n_pos = perstage_ap_raw(scores, labels)
    assert ap.shape == want.shape == (10, C)
    assert np.abs(ap - want).max() < TOL
    assert np.array_equal(perstage_ap_raw(scores, _onehot(labels, C))[0], ap)          # dense rows say the same as the ids
    rep = perstage_average_precision(scores, labels, names, None, "AP")
    assert list(rep) == stages
    for s, stage in enumerate(stages):
        assert list(rep[stage]["per_class_AP"]) == names[1:]                            # class 0 is never reported
        assert abs(rep[stage]["mean_AP"] - want_mean[s]) < TOL
    assert np.all(n_pos[:, 5] == 0) and np.all(ap[:, 5] == 0.0)                         # the class that never occurs
    # what the fixture must contain for the checks above to mean something
    runs = np.flatnonzero(np.diff(np.concatenate(([-9], labels, [-9]))))
    lens = set(np.diff(runs)[labels[runs[:-1]] > 0].tolist())
    assert {1, 2, 91, 171} <= lens and labels[0] > 0 and labels[-1] > 0 and (labels == -1).any() and not (labels == 5).any()


def test_host_matches_sklearn_on_naive_stage_sets():
    from sklearn.metrics import average_precision_score
    rng = np.random.default_rng(64)
    n, C = 2500, 7
    labels = np.concatenate([np.full(int(rng.integers(1, 120)), int(rng.integers(-1, C - 1)), np.int32) for _ in range(80)])[:n]
    n = labels.shape[0]
    scores = rng.random((n, C)).astype(np.float32)
    scores[:, 2] = np.round(scores[:, 2], 1)
    scores[:, 3] = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    scores[:, 4] = -3.0
    ap, n_pos = perstage_ap_raw(scores, labels)
    for c in range(C):
        g = (labels == c).astype(int)
        for s in range(10):
            idx, y = naive_stage_sets(g, s)
            assert n_pos[s, c] == y.sum()
            if y.sum() == 0:                   # sklearn's answer for a set without positives depends on its version: the fixture pins ours
                assert c == C - 1 and ap[s, c] == 0.0
                continue
            assert abs(ap[s, c] - average_precision_score(y, scores[idx, c])) < TOL, (c, s)


def test_stage_bounds_are_float_products():
    g = np.zeros(200, bool)
    g[10:101] = True                                            # 91 frames: len 90
    m = stage_members(g)
    assert np.flatnonzero(m[7])[0] - 10 == 62                   # 90 * 0.7 = 62.99999999999999, not 63
    assert np.flatnonzero(m[6])[-1] - 10 == 61
    assert not m[:, 100].any()                                  # the last frame of a run of two or more is in no stage
    one = np.zeros(5, bool)
    one[2] = True
    assert stage_members(one)[:, 2].all()                       # a one-frame run is in all ten stages
    for length in (1, 2, 3, 9, 10, 11, 90, 170, 1234):          # every stage of every run against Python's own arithmetic
        g = np.zeros(length + 3, bool)
        g[1:length + 2] = True
        m = stage_members(g)
        for s in range(10):
            lo = 1 + int(length * (s / 10))
            hi = max(lo + 1, 1 + int(length * ((s + 1) / 10)))
            assert np.flatnonzero(m[s]).tolist() == list(range(lo, hi)), (length, s)


def test_stage_key_strings():
    assert list(STAGE_NAMES) == [" 0%_ 10%", "10%_ 20%", "20%_ 30%", "30%_ 40%", "40%_ 50%", "50%_ 60%", "60%_ 70%", "70%_ 80%",
                                 "80%_ 90%", "90%_100%"]
    rep = perstage_average_precision(np.zeros((4, 3), np.float32), np.array([1, 1, 0, 2]), ["a", "b", "c"])
    assert list(rep) == list(STAGE_NAMES)
    assert list(rep[" 0%_ 10%"]) == ["per_class_AP", "mean_AP"]


def test_class_without_a_run_scores_zero_and_counts_in_the_mean():
    labels = np.array([0, 1, 1, 1, 0, 0, 1, 0], np.int32)
    scores = np.zeros((8, 3), np.float32)
    scores[:, 1] = [0.1, 0.9, 0.8, 0.7, 0.2, 0.3, 0.6, 0.1]                # class 1: every positive above every negative
    rep = perstage_average_precision(scores, labels, ["bg", "x", "never"])
    for stage in STAGE_NAMES:
        assert rep[stage]["per_class_AP"] == {"x": 1.0, "never": 0.0}
        assert rep[stage]["mean_AP"] == 0.5


def test_cap_is_the_calibrated_columns_on_each_stage_set():
    scores, labels, _, _, _ = _golden()
    C = scores.shape[1]
    cap, _ = perstage_ap_raw(scores, labels, "cAP")
    for c in range(C):
        g = (labels == c).astype(int)
        for s in range(10):
            idx, y = naive_stage_sets(g, s)
            idx_sorted = np.sort(idx)                           # ties keep their input order: the set in frame order
            y_sorted = y[np.argsort(idx, kind="stable")]
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = calibrated_average_precision_columns(scores[idx_sorted, c][:, None], y_sorted[:, None].astype(bool))[0]
            assert (np.isnan(want) and np.isnan(cap[s, c])) if y.sum() == 0 else abs(cap[s, c] - want) < TOL, (c, s)
    assert np.isnan(cap[:, 5]).all()
    rep = perstage_average_precision(scores, labels, [f"c{i}" for i in range(C)], None, "cAP")
    assert abs(rep["30%_ 40%"]["per_class_AP"]["c2"] - cap[3, 2]) < TOL


def test_unknown_metrics_raises():
    with pytest.raises(RuntimeError):
        perstage_average_precision(np.zeros((4, 3), np.float32), np.array([1, 1, 0, 2]), ["a", "b", "c"], None, "mAP")
