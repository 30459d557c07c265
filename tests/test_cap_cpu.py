"""CPU: the host forms of the calibrated average precision (prego_amd.metrics.calibrated_average_precision_columns and
perstage_ap_raw(.., 'cAP'); the reference's utils/metrics.py:10-22 and :64-130) against the figures the reference itself produced
(tests/golden/cap_mixed.npz, written by scripts/gen_cap_golden.py: tie-free columns, where the reference is defined), and against
the integer-rank formulas the device kernels implement (csrc/metrics.hip), restated in numpy, on inputs with long tie runs.

Tolerance: (P + 16) * 2^-52 per value, P = the positives in that sum.  Every term lies in (0, 1] and carries a few roundings; two
fp64 summations of P such terms in different orders differ by at most about 2 (P + 4) * 2^-53 after the division by P; the 16 leaves
room for the rounding of w + eps."""
import os

import numpy as np
import pytest

from prego_amd.metrics import (STAGE_NAMES, calibrated_average_precision_columns, perframe_average_precision, perstage_ap_raw,
                               perstage_average_precision, stage_members)

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -52
EDGES = [(1, 3), (63, 5), (4097, 12), (8193, 86), (9001, 130)]     # radix-tile and column-block edges of the device kernels


def tol(n_pos):
    return (np.asarray(n_pos, dtype=np.float64) + 16) * EPS


def close(got, want, n_pos):
    """(all within (P + 16) * 2^-52 and NaN exactly where NaN is wanted, the largest deviation)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False, float("inf")
    dev = np.where(nan, 0.0, np.abs(got - np.where(nan, 0.0, want)))
    return bool(np.all(dev <= tol(n_pos))), float(dev.max()) if dev.size else 0.0


def onehot(labels, C):
    m = np.zeros((labels.shape[0], C), np.float32)
    ok = (labels >= 0) & (labels < C)
    m[np.arange(labels.shape[0])[ok], labels[ok]] = 1
    return m


def golden():
    g = np.load(os.path.join(G, "cap_mixed.npz"))
    return {k: g[k] for k in g.files}


def run_labels(rng, n, ncls):
    """runs of 1..300 frames; ids -1 and ncls: negatives of every class"""
    runs = []
    while sum(len(r) for r in runs) < n:
        runs.append(np.full(int(rng.integers(1, 301)), int(rng.integers(-1, ncls + 1)), np.int32))
    return np.concatenate(runs)[:n]


def edge_scores(rng, n, ncls, levels):
    """levels = 0: tie-free columns (a permutation per column); else every column quantised to that many values"""
    if levels:
        return (rng.integers(0, levels, (n, ncls)) / np.float32(levels - 1 if levels > 1 else 1)).astype(np.float32)
    base = (np.arange(n, dtype=np.float32) - n // 2) / np.float32(max(n, 2))           # distinct float32 values, some negative
    return np.stack([rng.permutation(base) for _ in range(ncls)], axis=1)


def rank_cap_columns(scores, positive):
    """the per-frame formula from integer ranks: order by (descending score, ascending frame); q_i the positives in that order, rank_i
    the 1-based position of q_i; tps = i + 1, fps = rank_i - tps, w = (n - P) / P; cAP = (1/P) sum tps / (tps + fps / (w + eps) + eps)"""
    n, ncls = scores.shape
    out = np.full(ncls, np.nan)
    for c in range(ncls):
        order = np.lexsort((np.arange(n), -scores[:, c].astype(np.float64)))
        rank = np.flatnonzero(positive[order, c]) + 1
        P = rank.shape[0]
        if P == 0:
            continue
        tps = np.arange(1, P + 1, dtype=np.float64)
        fps = (rank - np.arange(1, P + 1)).astype(np.float64)
        w = (n - P) / P
        out[c] = np.sum(tps / (tps + fps / (w + EPS) + EPS)) / P
    return out


def rank_stage_cap(scores, labels):
    """the per-stage formula: for a stage member q_i of class c, tps = the stage members among q_0 .. q_i, fps = rank_i - (i + 1),
    w = (n - P_c) / P_cs, the sum divided by P_cs; NaN without a member.  -> (cAP [10, classes], members [10, classes])"""
    n, ncls = scores.shape
    out = np.full((10, ncls), np.nan)
    cnt = np.zeros((10, ncls), np.int64)
    for c in range(ncls):
        g = labels == c
        P = int(g.sum())
        if P == 0:
            continue
        member = stage_members(g)
        order = np.lexsort((np.arange(n), -scores[:, c].astype(np.float64)))
        at = np.flatnonzero(g[order])                                           # 0-based positions of q_0 .. q_{P-1}
        fps_all = (at + 1 - np.arange(1, P + 1)).astype(np.float64)
        for s in range(10):
            m = member[s][order][at]                                            # which q_i are stage members
            Ps = int(m.sum())
            cnt[s, c] = Ps
            if Ps == 0:
                continue
            tps = np.cumsum(m)[m].astype(np.float64)
            w = (n - P) / Ps
            out[s, c] = np.sum(tps / (tps + fps_all[m] / (w + EPS) + EPS)) / Ps
    return out, cnt


def test_fixture_is_tie_free_and_small():
    g = golden()
    n = g["scores"].shape[0]
    assert g["scores"].dtype == np.float32 and g["scores"].shape[1] == 8 and n >= 2000
    assert all(np.unique(g["scores"][:, c]).shape[0] == n for c in range(8))
    assert os.path.getsize(os.path.join(G, "cap_mixed.npz")) < 100_000
    assert [str(x) for x in g["stage_names"]] == list(STAGE_NAMES)


def test_host_matches_the_reference_fixture():
    g = golden()
    scores, labels = g["scores"], g["labels"]
    C = scores.shape[1]
    pos = onehot(labels, C) != 0
    cap = calibrated_average_precision_columns(scores, pos)
    ok, dev = close(cap, g["cap"], pos.sum(0))
    print("per-frame cAP: max |host - reference|", dev)
    assert ok and np.isnan(cap[6])
    stage, n_pos = perstage_ap_raw(scores, labels, "cAP")
    ok, dev = close(stage, g["stage_cap"], n_pos)
    print("per-stage cAP: max |host - reference|", dev)
    assert ok and np.isnan(stage[:, 6]).all()
    names = [f"c{i}" for i in range(C)]
    rep = perframe_average_precision(scores, onehot(labels, C), names, None, "cAP")
    assert list(rep["per_class_AP"]) == [names[c] for c in range(1, C) if c != 6]
    assert abs(rep["mean_AP"] - float(g["mean_cap"])) <= tol(pos.sum(0).max())
    srep = perstage_average_precision(scores, labels, names, None, "cAP")
    assert list(srep) == list(STAGE_NAMES)
    assert all(np.isnan(srep[s]["mean_AP"]) for s in STAGE_NAMES) and np.isnan(g["stage_mean_cap"]).all()     # class 6: NaN in every mean


def test_rank_formulas_match_the_fixture():
    g = golden()
    scores, labels = g["scores"], g["labels"]
    pos = onehot(labels, scores.shape[1]) != 0
    assert close(rank_cap_columns(scores, pos), g["cap"], pos.sum(0))[0]
    stage, cnt = rank_stage_cap(scores, labels)
    assert close(stage, g["stage_cap"], cnt)[0]


@pytest.mark.parametrize("levels", [0, 3, 7])
@pytest.mark.parametrize("n,ncls", EDGES[:3])
def test_rank_formulas_match_the_host_forms(n, ncls, levels):
    rng = np.random.default_rng(1000 * levels + n + ncls)
    scores = edge_scores(rng, n, ncls, levels)
    labels = run_labels(rng, n, ncls)
    pos = onehot(labels, ncls) != 0
    ok, dev = close(rank_cap_columns(scores, pos), calibrated_average_precision_columns(scores, pos), pos.sum(0))
    want, want_pos = perstage_ap_raw(scores, labels, "cAP")
    got, cnt = rank_stage_cap(scores, labels)
    ok2, dev2 = close(got, want, want_pos)
    print(f"n {n} C {ncls} levels {levels}: max |rank form - host| per frame {dev:.2e}, per stage {dev2:.2e}")
    assert ok and ok2 and np.array_equal(cnt, want_pos)


def test_rank_formulas_on_one_tie_run_and_dense_targets():
    rng = np.random.default_rng(5)
    n = 500
    scores = np.stack([np.full(n, 0.25, np.float32), (rng.random(n) < 0.5).astype(np.float32),
                       np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(np.float32), rng.random(n).astype(np.float32)], axis=1)
    pos = rng.random((n, 4)) < 0.3
    pos[:, 3] = True                                                            # positive on every frame: w = 0
    got, want = rank_cap_columns(scores, pos), calibrated_average_precision_columns(scores, pos)
    assert close(got, want, pos.sum(0))[0]
    assert abs(want[3] - 1.0) <= tol(n)
