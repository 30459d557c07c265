"""The automaton shapes of the ragged streaming step (tests/test_gpu_step_ragged.py, tests/test_gpu_stream_pool_ragged.py;
tests/test_stream_ragged_cpu.py proves on the CPU that a ragged schedule of the automaton equals the per-stream slices of its
frame-by-frame run).  The references are the shared ones of step_wide_cases ("wide": n streams of 6 or 8 frames) wherever they have the
frames; the one shape none of them has - 200 streams of one frame beside one of 32 - is "straggler": the automaton of ant_step_cases'
L4-C12 (same weights, same feature seed) over exactly those clip lengths.  A shape names reference streams in call order and drives one
call per tuple of counts, every stream at its own position."""
import random

from tests.helpers import ant_step_cases as S
from tests.helpers import gru_automaton as A

STRAGGLER_LENS = [1] * 100 + [32] + [1] * 100
_R256 = tuple(range(1, 7)) * 12 + (4,)                          # 73 streams, 12 x 21 + 4 = 256 rows

# id: (source, reference case, reference streams in call order, counts of every call)
SHAPES = {
    "n1": ("wide", "L1-C12", (0,), ((1,), (2,))),
    "n3": ("wide", "L1-C12", (0, 1, 2), ((1, 2, 3), (3, 1, 2))),               # a stream ends in every launch; ascending: the walk permutes
    "n17": ("wide", "L1-C12", tuple(range(17)), ((1,) + (2,) * 15 + (4,), (4,) + (2,) * 15 + (1,))),      # alive: 17, 16, 1, 1
    "n16-equal": ("wide", "L1-C12", tuple(range(16)), ((3,) * 16, (5,) * 16)),
    "n201-straggler": ("straggler", "L4-C12", tuple(range(201)), (tuple(STRAGGLER_LENS),)),               # R = 232, 31 launches of one stream
    "R256": ("wide", "L8-C86", tuple(range(73)), (_R256,)),
}
assert sum(_R256) == 256 and sum(STRAGGLER_LENS) == 232


def straggler_reference(device="cpu"):
    """(case, sd, feats, Result) of the straggler shape, conditions() checked; the feature bits are drawn on the CPU"""
    L, C, seed, _, fseed, _ = S.CASES["L4-C12"]
    case = A.Case(ant_len=L, seed=seed, n_classes=C, **A.RGB)
    sd, meta = A.build_state_dict(case)
    feats = A.build_features(case, STRAGGLER_LENS, fseed, "cpu", sigma=meta["sigma"])
    feats = [tuple(None if t is None else t.to(device) for t in rf) for rf in feats]
    res = A.run(sd, meta, case, feats, device=device)
    A.conditions(sd, case, res)
    return case, sd, feats, res


def offsets(counts):
    """the first packed row of every stream of a call"""
    off, at = [], 0
    for k in counts:
        off.append(at)
        at += k
    return off


def reference_rows(offs, streams, pos, counts):
    """the reference's rows (clip after clip, clip s at offs[s]) a ragged call returns: stream i of the call at frames pos[i] ..
    pos[i] + counts[i]), packed in call order; and the row of every stream's last frame"""
    rows = [offs[s] + pos[i] + t for i, s in enumerate(streams) for t in range(counts[i])]
    last = [offs[s] + pos[i] + counts[i] - 1 for i, s in enumerate(streams)]
    return rows, last


def seeded_counts(n, lo, hi, seed):
    rng = random.Random(seed)
    return [rng.randint(lo, hi) for _ in range(n)]


def groups_of_equal_count(counts):
    """{K: streams with K frames, in call order}: the calls a host makes today, one step_frames per group"""
    g = {}
    for i, k in enumerate(counts):
        g.setdefault(k, []).append(i)
    return g


def ragged_schedule(n, T, seed, max_rows=256, hi=8):
    """[(streams of the call in call order, their counts)] until every stream has taken its T frames: each call a seeded subset, each
    stream a seeded count in 1..hi cut to what it has left, the call cut to max_rows rows"""
    rng = random.Random(seed)
    left, calls = [T] * n, []
    while any(left):
        can = [s for s in range(n) if left[s] > 0]
        act = rng.sample(can, rng.randint(1, len(can)))
        counts, rows, keep = [], 0, []
        for s in act:
            k = min(rng.randint(1, hi), left[s], 32)
            if rows + k > max_rows:
                break
            keep.append(s)
            counts.append(k)
            rows += k
        for s, k in zip(keep, counts):
            left[s] -= k
        calls.append((keep, counts))
    return calls
