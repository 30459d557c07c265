"""Cases shared by tests/test_decode_pool_cpu.py and tests/test_gpu_decode_pool.py: the prefix identity that defines online fixed-lag
decoding (through the existing `viterbi_decode`), the seeded case set, the three ways to cut a stream into pushes, and the far-state
stream."""
import numpy as np

from prego_amd.decode import DECODE_CAP, OnlineDecoder, viterbi_decode
from tests.helpers.decode_cases import HAND_CASES, random_costs, random_model, random_probs

LAGS_CPU = (0, 1, 2, 5, 16, 64, 100)
CLASSES_CPU = (1, 2, 3, 12, 86)


def prefix_labels(x, trans, init, lag):
    """label(f) = viterbi_decode(x[: min(f + L, T - 1) + 1])[0][f] for every frame, and the record of every prefix x[: t + 1]"""
    T = len(x)
    pre = [viterbi_decode(x[:t + 1], trans, init) for t in range(T)]
    labels = np.array([pre[min(f + lag, T - 1)][0][f] for f in range(T)], np.int32).reshape(T)
    return labels, [p[1] for p in pre]


def cpu_cases():
    """(name, x [T, C] costs or probabilities, trans, init, lag): every C of CLASSES_CPU, every lag of LAGS_CPU, T in 1..90, forbidden
    density 0 / 0.5 / 0.9, init given and None, both input modes, and the hand cases of the offline decode at lags 0, 1 and 2"""
    rng = np.random.default_rng(2024)
    cases, k = [], 0
    for C in CLASSES_CPU:
        for lag in LAGS_CPU:
            for density in (0.0, 0.5, 0.9):
                T = int(rng.integers(1, 91)) if k % 5 else (1, 2, 90, lag + 1, max(lag, 1))[(k // 5) % 5]
                T = min(max(T, 1), 90)
                trans, init = random_model(rng, C, density, given_init=bool(k % 2), out_of_range=k % 7 == 0)
                probs = k % 3 == 0
                x = random_probs(rng, T, C) if probs else random_costs(rng, T, C, out_of_range=k % 4 == 0)
                cases.append((f"C{C}_L{lag}_d{density}_T{T}_{'p' if probs else 'c'}", x, trans, init, lag))
                k += 1
    for name, c in sorted(HAND_CASES.items()):
        x = np.asarray(c["costs"], np.int32).reshape(-1, c["C"])
        if len(x):
            for lag in (0, 1, 2):
                cases.append((f"hand_{name}_L{lag}", x, np.asarray(c["trans"], np.int64), c["init"], lag))
    # a stream that dies at frame 3 after frame 0 was committed (lag 2)
    cases.append(("dies_at_3_L2", *dying_stream(), 2))
    return cases


def dying_stream():
    """(x, trans, init): three states in a row 0 -> 1 -> 2 with no way to stay and none out of 2: frame 3 has no finite state"""
    x = np.full((8, 3), 7, np.int32)
    trans = np.array([[-1, 0, -1], [-1, -1, 0], [-1, -1, -1]], np.int64)
    return x, trans, [0, -1, -1]


def cuts(T, kind, rng=None):
    """frame counts of the pushes that feed T frames: 'single' 1 each, 'burst' 32 each (the last shorter), 'ragged' random 1..32"""
    if kind == "single":
        return [1] * T
    if kind == "burst":
        return [32] * (T // 32) + ([T % 32] if T % 32 else [])
    out, left = [], T
    while left:
        k = min(int(rng.integers(1, 33)), left)
        out.append(k)
        left -= k
    return out


def run_host(x, trans, init, lag, counts=None, vote_window=1, max_events=1024, n_classes=None):
    """an `OnlineDecoder` fed x in pushes of `counts` frames (default: one push), then flushed: (decoder, labels [T], now [T])"""
    C = x.shape[1] if n_classes is None else n_classes
    dec = OnlineDecoder(trans, init, lag=lag, n_classes=C, vote_window=vote_window, max_events=max_events)
    labs, nows, at = [], [], 0
    for k in (counts if counts is not None else ([len(x)] if len(x) else [])):
        lab, now = dec.push(x[at:at + k])
        labs.append(lab)
        nows.append(now)
        at += k
    labs.append(dec.flush())
    return dec, np.concatenate(labs).astype(np.int32), (np.concatenate(nows).astype(np.int32) if nows else np.zeros(0, np.int32))


def far_state_stream():
    """C = 3, only self-loops, costs mode: frames 0..599 cost (0, 5, CAP), frames 600..1299 (CAP, CAP, 0).  The spread of the finite keys
    reaches 19 660 200 >= 2^24; the final keys are (22 936 900, 22 939 900, 19 660 200); the committed labels (lag 64) are 0 up to frame
    1135 and 2 from frame 1136"""
    x = np.zeros((1300, 3), np.int32)
    x[:600] = (0, 5, DECODE_CAP)
    x[600:] = (DECODE_CAP, DECODE_CAP, 0)
    trans = np.full((3, 3), -1, np.int64)
    np.fill_diagonal(trans, 0)
    return x, trans, None
