"""CPU side of the ragged streaming step (prego_miniroad_step_ragged / _anticipation, prego_miniroad_step_pool_ragged;
csrc/stream_frames.hip): `pack_bursts` and its inverse with the offsets the kernels use; the automaton reference driven by a ragged
schedule - every stream at its own position, the state carried - equals the per-stream slices of its frame-by-frame run, which is what
tests/test_gpu_step_ragged.py relies on when it compares packed rows against rows of ONE reference; the host model of the pool's record fed
per-stream bursts equals `aggregate()`; and the entry points are declared and bound."""
import gzip
import json
import os
import random
import re

import pytest

torch = pytest.importorskip("torch")

from prego_amd._lib import PregoError                                          # noqa: E402
from prego_amd.aggregate import OnlineRecord, aggregate, aggregate_online      # noqa: E402
from prego_amd.stream_pool import burst_offsets, pack_bursts, unpack_bursts    # noqa: E402
from tests.helpers import gru_automaton as A                                   # noqa: E402
from tests.helpers import step_ragged_cases as SR                              # noqa: E402
from tests.helpers import step_wide_cases as SW                                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


@pytest.mark.parametrize("counts", [(1, 2, 3, 4), (4, 3, 2, 1), (2, 2, 2), (3, 1, 3, 1, 2), (1,), (32, 1, 1)],
                         ids=["ascending", "descending", "tied", "mixed-ties", "one", "straggler"])
def test_pack_bursts_and_its_inverse(counts):
    d = 5
    bursts = [torch.arange(k * d, dtype=torch.float32).view(k, d) + 1000 * s for s, k in enumerate(counts)]
    packed, got = pack_bursts(bursts)
    assert got == list(counts) and packed.shape == (sum(counts), d) and packed.is_contiguous()
    off = burst_offsets(got)
    assert off == SR.offsets(counts) and off[0] == 0 and all(b - a == k for a, b, k in zip(off, off[1:], counts))
    for s, k in enumerate(counts):                                # stream s owns rows off[s] .. off[s] + k) in frame order
        assert torch.equal(packed[off[s]:off[s] + k], bursts[s])
    back = unpack_bursts(packed, got)
    assert len(back) == len(bursts) and all(torch.equal(a, b) for a, b in zip(back, bursts))
    assert all(torch.equal(a, b) for a, b in zip(torch.split(packed, got), bursts))
    # all counts equal: byte for byte step_frames' [n, K, d]
    if len(set(counts)) == 1:
        assert torch.equal(packed.view(len(counts), counts[0], d), torch.stack(bursts))


def test_pack_bursts_refuses_what_it_cannot_pack():
    with pytest.raises(PregoError, match="no streams"):
        pack_bursts([])
    with pytest.raises(PregoError, match="stream 1"):
        pack_bursts([torch.zeros(2, 4), torch.zeros(2, 5)])
    with pytest.raises(PregoError, match="stream 1"):
        pack_bursts([torch.zeros(2, 4), torch.zeros(0, 4)])
    with pytest.raises(PregoError, match="counts sum to 3"):
        unpack_bursts(torch.zeros(4, 2), [1, 2])


def _drive(sd, meta, case, x, res, streams, calls):
    """the automaton restarted at every call from the states the call before left, stream i of the call at its own position"""
    full = (res.logits, res.argmax, res.h[0], res.ant_logits, res.ant_argmax)
    pos, h = [0] * len(streams), None
    for counts in calls:
        part = [(x[s][pos[i]:pos[i] + k], None) for i, (s, k) in enumerate(zip(streams, counts))]
        got = A.run(sd, meta, case, part, h0=h)
        rows, last = SR.reference_rows(res.offs, streams, pos, counts)
        for name, g, w in zip(("logits", "argmax", "state", "anticipation logits", "anticipation argmax"),
                              (got.logits, got.argmax, got.h[0], got.ant_logits, got.ant_argmax), full):
            assert torch.equal(g, w[rows]), (counts, name)
        assert torch.equal(got.h_last, full[2][last].to(torch.float32))
        h, pos = got.h_last, [p + k for p, k in zip(pos, counts)]
    return pos


@pytest.mark.parametrize("sid", ["n1", "n3", "n17", "n16-equal"])
def test_a_ragged_schedule_of_the_automaton_equals_its_frame_by_frame_run(sid):
    src, cid, streams, calls = SR.SHAPES[sid]
    assert src == "wide"
    case, sd, n, T, feats, res = SW.reference(cid)
    _, meta = A.build_state_dict(case)
    assert res.lens == [T] * n and max(streams) < n
    pos = _drive(sd, meta, case, [r for r, _ in feats], res, streams, calls)
    assert max(pos) <= T and len({tuple(c) for c in calls}) == len(calls)


def test_the_straggler_reference_is_the_shared_automaton_over_its_own_lengths():
    case, sd, feats, res = SR.straggler_reference()
    _, meta = A.build_state_dict(case)
    _, sd_wide, _, _, _, _ = SW.reference("L4-C12")
    assert sd.keys() == sd_wide.keys() and all(torch.equal(sd[k], sd_wide[k]) for k in sd)      # the weights of the shared case
    assert res.lens == SR.STRAGGLER_LENS and res.logits.shape[0] == 232
    src, cid, streams, calls = SR.SHAPES["n201-straggler"]
    assert src == "straggler" and sum(calls[0]) == 232 and max(calls[0]) == 32
    _drive(sd, meta, case, [r for r, _ in feats], res, streams, calls)
    # the 32-frame stream in two ragged calls beside its one-frame neighbours: its own slice, whatever rides along
    _drive(sd, meta, case, [r for r, _ in feats], res, (99, 100, 101), ((1, 20, 1),))
    _drive(sd, meta, case, [r for r, _ in feats], res, (100,), ((7,), (25,)))


def test_the_shapes_fit_their_references_and_the_call_limits():
    for sid, (src, cid, streams, calls) in SR.SHAPES.items():
        n_ref, T = (len(SR.STRAGGLER_LENS), None) if src == "straggler" else SW.CASES[cid]
        assert 1 <= len(streams) <= 256 and max(streams) < n_ref and len(set(streams)) == len(streams), sid
        total = [0] * len(streams)
        for counts in calls:
            assert len(counts) == len(streams) and 1 <= min(counts) and max(counts) <= 32 and sum(counts) <= 256, sid
            total = [a + k for a, k in zip(total, counts)]
        lens = SR.STRAGGLER_LENS if src == "straggler" else [T] * n_ref
        assert all(t <= lens[s] for t, s in zip(total, streams)), sid
    assert sum(SR.SHAPES["R256"][3][0]) == 256
    alive = [sum(1 for k in SR.SHAPES["n17"][3][0] if k > t) for t in range(4)]
    assert alive == [17, 16, 1, 1]                                # across a tile boundary and down to a single lane
    for n, T, seed in ((17, 8, 3), (37, 8, 4)):
        calls = SR.ragged_schedule(n, T, seed)
        took = [0] * n
        for act, counts in calls:
            assert len(act) == len(set(act)) == len(counts) >= 1 and sum(counts) <= 256 and min(counts) >= 1
            for s, k in zip(act, counts):
                took[s] += k
        assert took == [T] * n and any(len(set(c)) > 1 for _, c in calls)


def test_per_stream_bursts_of_a_ragged_schedule_equal_aggregate_on_the_g8_videos():
    with gzip.open(os.path.join(G, "g8_output_miniROAD.json.gz"), "rt") as f:
        data = json.load(f)
    vids = sorted(data, key=lambda k: len(data[k]["pred"]))[:4]
    ids = [data[v]["pred"] for v in vids]
    want = []
    for row in ids:
        a = aggregate({"v": {"pred": row, "gt": [0] * len(row)}})["v"]
        want.append({"pred": a["pred"], "changes_pred": a["changes_pred"]})
    # one pool tick = one ragged call: a seeded subset of the streams, each with its own count in 1..32
    rng = random.Random(29)
    recs, at, sizes = [OnlineRecord(200, 12, 1 << 20) for _ in ids], [0] * len(ids), [[] for _ in ids]
    while any(a < len(row) for a, row in zip(at, ids)):
        can = [s for s in range(len(ids)) if at[s] < len(ids[s])]
        for s in rng.sample(can, rng.randint(1, len(can))):
            k = min(rng.randint(1, 32), len(ids[s]) - at[s])
            recs[s].push_frames(ids[s][at[s]:at[s] + k])
            sizes[s].append(k)
            at[s] += k
    for s, rec in enumerate(recs):
        rec.flush()
        r = rec.result()
        assert rec.overflow == 0 and {"pred": r["pred"], "changes_pred": r["changes_pred"]} == want[s], vids[s]
        assert len(set(sizes[s])) == 32 and sizes[s] != sizes[(s + 1) % len(ids)][:len(sizes[s])]
        assert aggregate_online(ids[s], 200, n_classes=12, bursts=sizes[s]) == want[s]


def _args(hdr, name):
    m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/prego_amd.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_entry_points_are_declared_and_bound():
    from prego_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "prego_amd.h")).read()
    want = {"prego_miniroad_step_ragged_workspace_bytes": 3, "prego_miniroad_step_ragged": 12, "prego_miniroad_step_ragged_anticipation": 14,
            "prego_miniroad_step_pool_ragged_workspace_bytes": 3, "prego_miniroad_step_pool_ragged": 15}
    for name, n_args in want.items():
        assert len(_args(hdr, name)) == n_args, name
        assert name in _lib.SYMBOLS
    a = _args(hdr, "prego_miniroad_step_ragged")
    assert a[1].endswith("n_streams") and a[2] == "const int32_t* n_frames" and a[9].endswith("workspace") and a[11].endswith("stream")
    f = _args(hdr, "prego_miniroad_step_frames")
    assert [x.split()[-1] for x in a[3:]] == [x.split()[-1] for x in f[3:]]      # argument order follows step_frames
    a, f = _args(hdr, "prego_miniroad_step_ragged_anticipation"), _args(hdr, "prego_miniroad_step_frames_anticipation")
    assert a[2] == "const int32_t* n_frames" and [x.split()[-1] for x in a[3:]] == [x.split()[-1] for x in f[3:]]
    a, f = _args(hdr, "prego_miniroad_step_pool_ragged"), _args(hdr, "prego_miniroad_step_pool_frames")
    assert a[3] == "const int32_t* n_frames" and f[3] == "int n_frames" and a[:3] + a[4:] == f[:3] + f[4:]
    assert _args(hdr, "prego_miniroad_step_ragged_workspace_bytes")[2].endswith("n_rows")
    assert "#define PREGO_ABI_VERSION 7" in hdr
    src = open(os.path.join(ROOT, "prego_amd", "_lib.py")).read()
    for name in want:
        assert f"lib.{name}.argtypes" in src, f"{name} has no prototype in _lib"


def test_python_surface():
    import prego_amd.model as M
    from prego_amd.engine import MiniRoadEngine
    from prego_amd.stream_pool import StreamPool
    assert callable(MiniRoadEngine.step_ragged) and callable(M.MROAD.step_ragged) and callable(M.MROADA.step_ragged)
    assert M.MROADA.step_ragged is not M.MROAD.step_ragged
    assert callable(StreamPool.push_ragged)
