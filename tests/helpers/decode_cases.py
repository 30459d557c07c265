"""Cases shared by tests/test_decode_cpu.py and tests/test_gpu_decode.py: hand-computed decodes, the brute force over all paths, and the
seeded random models and video sets."""
import numpy as np

from prego_amd.decode import DECODE_BLOCK, DECODE_CAP, DECODE_PREFETCH

U = lambda C, sw, st=0: (np.full((C, C), sw, np.int64) + np.diag(np.full(C, st - sw, np.int64))).tolist()

# name -> costs [T][C], trans [C][C], init [C] | None, labels, record; every value worked out by hand (see the comments)
HAND_CASES = {
    # 0 0 1 1 costs 0 + 0 + (50 + 0) + 0 = 50; staying in 0 costs 200, in 1 costs 200
    "switch_pays": dict(costs=[[0, 100], [0, 100], [100, 0], [100, 0]], trans=U(2, 50), init=None, labels=[0, 0, 1, 1], record=(50, 1)),
    # one frame of evidence for 1: staying costs 100, 0 0 1 0 costs 300, 0 0 1 1 costs 150 + 100 = 250
    "switch_does_not_pay": dict(costs=[[0, 100], [0, 100], [100, 0], [0, 100]], trans=U(2, 150), init=None, labels=[0, 0, 0, 0],
                                record=(100, 0)),
    # every path costs 5 * 7 + 4 * 3 = 47: the lowest predecessor and the lowest end state win
    "all_equal": dict(costs=[[7, 7, 7]] * 5, trans=[[3, 3, 3]] * 3, init=None, labels=[0, 0, 0, 0, 0], record=(47, 0)),
    # state 0 cannot start: d_0 = (inf, 50); d_1 = (50 + 10 + 0, 50 + 0 + 50) = (60, 100)
    "forbidden_init": dict(costs=[[0, 50], [0, 50]], trans=U(2, 10), init=[-1, 0], labels=[1, 0], record=(60, 0)),
    "infeasible_transitions": dict(costs=[[1, 2], [3, 4], [5, 6]], trans=[[-1, -1], [-1, -1]], init=None, labels=[-1, -1, -1], record=(-1, -1)),
    "infeasible_init": dict(costs=[[1, 2], [3, 4]], trans=U(2, 1), init=[-1, -7], labels=[-1, -1], record=(-1, -1)),
    # one frame never looks at trans
    "one_frame_forbidden_transitions": dict(costs=[[5, 3, 3]], trans=[[-1] * 3] * 3, init=None, labels=[1], record=(3, 1)),
    "empty": dict(costs=np.zeros((0, 3), np.int32).tolist(), trans=U(3, 1), init=None, labels=[], record=(0, -1)),
    # words out of range: a cost of -5 is 0, of 40000 is CAP; a transition of 100000 is CAP, init 99999 is CAP
    # d_0 = (CAP + 0, CAP + CAP); d_1(0) = min(CAP + 0, 2 CAP + CAP) + 10 = CAP + 10; d_1(1) = min(CAP + CAP, 2 CAP + 0) + 0 = 2 CAP: the lower i
    "clamped_words": dict(costs=[[-5, 40000], [10, -1]], trans=[[0, 100000], [100000, 0]], init=[99999, 99999], labels=[0, 0],
                          record=(DECODE_CAP + 10, 0)),
}
for _c in HAND_CASES.values():
    _c["C"] = len(_c["trans"])


def brute_force(costs, trans, init):
    """every one of the C^T paths of one video (T >= 1), by enumeration: (optimum or None when no path is allowed, the path the
    definition picks).  P[t][j] = the cheapest allowed prefix that ends in j at t, from the enumeration; the path: the lowest end state
    with the smallest P[T-1], then backwards the lowest i with the smallest P[t-1][i] + trans[i][l_t]."""
    e = np.clip(np.asarray(costs, np.int64), 0, DECODE_CAP)
    T, C = e.shape
    tr = np.asarray(trans, np.int64)
    tr = np.where(tr < 0, -1, np.minimum(tr, DECODE_CAP))
    ini = np.zeros(C, np.int64) if init is None else np.asarray(init, np.int64)
    ini = np.where(ini < 0, -1, np.minimum(ini, DECODE_CAP))
    paths = np.stack(np.meshgrid(*[np.arange(C)] * T, indexing="ij"), -1).reshape(-1, T)
    BIG = 1 << 50
    ok = ini[paths[:, 0]] >= 0
    cum = ini[paths[:, 0]] + e[0, paths[:, 0]]
    P = np.full((T, C), BIG, np.int64)
    for j in range(C):
        m = ok & (paths[:, 0] == j)
        if m.any():
            P[0, j] = cum[m].min()
    for t in range(1, T):
        step = tr[paths[:, t - 1], paths[:, t]]
        ok = ok & (step >= 0)
        cum = cum + step + e[t, paths[:, t]]
        for j in range(C):
            m = ok & (paths[:, t] == j)
            if m.any():
                P[t, j] = cum[m].min()
    if not ok.any():
        return None, None
    best = int(cum[ok].min())
    lab = [int(np.argmin(P[T - 1]))]
    for t in range(T - 1, 0, -1):
        cand = np.where((tr[:, lab[0]] >= 0) & (P[t - 1] < BIG), P[t - 1] + tr[:, lab[0]], BIG)
        lab.insert(0, int(np.argmin(cand)))
    return best, lab


def random_model(rng, C, density=0.0, given_init=True, out_of_range=False):
    """trans [C, C] and init [C] | None: costs up to 4000, a fraction `density` of the words forbidden; out_of_range: some words above
    CAP and some negative words other than -1"""
    trans = rng.integers(0, 4000, (C, C)).astype(np.int32)
    trans[rng.random((C, C)) < density] = -1
    init = rng.integers(0, 4000, C).astype(np.int32) if given_init else None
    if given_init:
        init[rng.random(C) < density] = -1
    if out_of_range:
        big = rng.random((C, C)) < 0.1
        trans[big & (trans >= 0)] = rng.integers(DECODE_CAP + 1, 2 ** 31 - 1)
        trans[trans < 0] = rng.integers(-2 ** 31, 0, int((trans < 0).sum()))
    return trans, init


def random_lengths(rng, V, max_len):
    """V lengths: the edge lengths (0, 1, 2, the backtrace block and its double +- 1, the prefetch depth +- 1) first, as many as fit,
    then random ones below max_len"""
    edge = [0, 1, 2, DECODE_BLOCK - 1, DECODE_BLOCK, DECODE_BLOCK + 1, 2 * DECODE_BLOCK - 1, 2 * DECODE_BLOCK, 2 * DECODE_BLOCK + 1,
            DECODE_PREFETCH - 1, DECODE_PREFETCH, DECODE_PREFETCH + 1]
    lens = [n for n in edge if n <= max_len][:V]
    return lens + rng.integers(0, max_len + 1, V - len(lens)).tolist()


def random_costs(rng, T, C, out_of_range=False):
    x = rng.integers(0, 3000, (T, C)).astype(np.int32)
    if out_of_range and T:
        x[rng.random((T, C)) < 0.05] = -17
        x[rng.random((T, C)) < 0.05] = 2 ** 31 - 1
    return x


def random_probs(rng, T, C):
    """softmax rows with a few special words among them: 0, a denormal, a negative, NaN, +inf, 1, more than 1"""
    z = rng.normal(0.0, 4.0, (T, C))
    p = np.exp(z - z.max(1, keepdims=True))
    p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    special = np.array([0.0, 1e-42, -0.25, np.nan, np.inf, 1.0, 1.5, -0.0], np.float32)
    hit = rng.random((T, C)) < 0.02
    p[hit] = special[rng.integers(0, special.size, int(hit.sum()))]
    return p
