"""CPU side of the stream pool (prego_amd/stream_pool.py, csrc/stream_pool.hip): `aggregate_online` - the host model of a slot's vote
record, which tests/test_gpu_stream_pool.py holds the device rule against - equals the reference's aggregation (the shipped G8 pair and
`aggregate` on small streams with ties), the slot bookkeeping needs no device, and the entry points are declared and bound."""
import gzip
import json
import os
import re

import numpy as np
import pytest

from prego_amd._lib import PregoError
from prego_amd.aggregate import OVERFLOW_BAD_ID, OVERFLOW_FULL, OnlineRecord, aggregate, aggregate_online
from prego_amd.stream_pool import SlotTable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def test_aggregate_online_reproduces_the_shipped_pair_frame_by_frame():
    with gzip.open(os.path.join(G, "g8_output_miniROAD.json.gz"), "rt") as f:
        data = json.load(f)
    want = json.load(open(os.path.join(G, "g8_aggregated_data.json")))
    assert len(data) == 15
    for vid, v in data.items():
        got = aggregate_online(v["pred"], 200, n_classes=12)
        assert got == {k: want[vid][k] for k in ("pred", "changes_pred")}, vid


def _streams():
    rng = np.random.default_rng(5)
    return {
        "random-7cls-1003": rng.integers(0, 7, 1003).tolist(),
        "multiple-of-200": rng.integers(0, 3, 600).tolist(),               # no shorter last window: flush finds nothing
        "multiple-of-3": [2, 2, 1, 0, 0, 1, 1, 2, 2],
        "ties": [3, 1, 3, 1, 5, 5, 0, 0, 4, 2, 2, 4, 1, 3],                # window 4: 2-2 ties, window 2: 1-1 ties; the lowest id wins
        "constant": [4] * 37,
        "one-frame": [6],
        "long-runs": [0] * 250 + [1] * 150 + [0] * 230,
    }


@pytest.mark.parametrize("window", [1, 2, 3, 4, 200, 5000])
def test_aggregate_online_equals_aggregate(window):
    for name, ids in _streams().items():
        want = aggregate({"v": {"pred": ids, "gt": [0] * len(ids)}}, window_size=window)["v"]
        got = aggregate_online(ids, window)
        assert got == {"pred": want["pred"], "changes_pred": want["changes_pred"]}, (name, window)
    assert 5000 > max(len(v) for v in _streams().values())                 # a window larger than every stream
    assert any(len(v) % 200 == 0 for v in _streams().values())


def test_the_lowest_id_wins_a_tie():
    assert aggregate_online([3, 1, 3, 1], 4) == {"pred": [1], "changes_pred": [4]}
    assert aggregate_online([5, 2], 200) == {"pred": [2], "changes_pred": [2]}


def test_record_midway_flush_twice_overflow_and_bad_ids():
    r = OnlineRecord(window=3, n_classes=4, max_events=2)
    for i in (1, 1, 0, 2, 2):
        r.push(i)
    assert r.result() == {"pred": [1], "changes_pred": [3], "frames": 5}     # the finished windows only
    r.flush()
    r.flush()                                                               # nothing left to vote
    assert r.result() == {"pred": [1, 2], "changes_pred": [3, 5], "frames": 5} and r.overflow == 0
    for i in (0, 0, 0, 3):                                                  # the next finished window votes 0: a third event, dropped
        r.push(i)
    assert r.overflow == OVERFLOW_FULL and r.result()["pred"] == [1, 2]
    r.push(4)
    r.push(-1)
    assert r.overflow == OVERFLOW_FULL | OVERFLOW_BAD_ID and r.frames == 9  # an id outside the classes counts nothing
    with pytest.raises(ValueError, match="overflow"):
        aggregate_online([0, 1, 0, 1], 1, max_events=3)
    with pytest.raises(ValueError, match="overflow"):
        aggregate_online([0, 12], 1, n_classes=12)
    assert aggregate_online([], 200) == {"pred": [], "changes_pred": [0]}


def test_slot_bookkeeping_needs_no_device():
    t = SlotTable(4)
    assert (t.capacity, t.free) == (4, 4)
    assert [t.open() for _ in range(4)] == [0, 1, 2, 3] and t.free == 0      # lowest free first
    with pytest.raises(PregoError, match="all 4 slots are open"):
        t.open()
    t.release(2)
    t.release(0)
    assert t.free == 2 and not t.is_open(0) and t.is_open(1)
    assert t.open() == 0 and t.open() == 2                                   # reuse after close, lowest first
    t.release(1)
    with pytest.raises(PregoError, match="slot 1 is not open"):              # double close
        t.release(1)
    with pytest.raises(PregoError, match="slot 1 is not open"):              # push to a closed slot
        t.check([0, 1], "push")
    with pytest.raises(PregoError, match="slot 3 is named twice"):
        t.check([3, 0, 3], "push")
    with pytest.raises(PregoError, match="slot 4 is not open"):
        t.check([4], "push")
    with pytest.raises(PregoError, match="slot -1 is not open"):
        t.check([-1], "push")
    with pytest.raises(PregoError, match="0 slots"):
        t.check([], "push")
    assert t.check((3, 0, 2), "push") == [3, 0, 2]                           # the caller's order is kept
    with pytest.raises(PregoError, match="capacity 0"):
        SlotTable(0)
    big = SlotTable(300)
    for _ in range(300):
        big.open()
    with pytest.raises(PregoError, match="257 slots"):
        big.check(range(257), "push")
    assert len(big.check(range(256), "push")) == 256


def _args(hdr, name):
    m = re.search(r"\b(?:int|size_t|void)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/prego_amd.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_entry_points_are_declared_and_bound():
    from prego_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "prego_amd.h")).read()
    want = {"prego_stream_pool_bytes": 3, "prego_stream_pool_create": 8, "prego_stream_pool_destroy": 1,
            "prego_miniroad_step_pool_workspace_bytes": 2, "prego_miniroad_step_pool": 14, "prego_stream_pool_vote": 5,
            "prego_stream_pool_flush": 4, "prego_stream_pool_reset": 4, "prego_stream_pool_record": 4}
    for name, n_args in want.items():
        assert len(_args(hdr, name)) == n_args, name
        assert name in _lib.SYMBOLS
    a = _args(hdr, "prego_miniroad_step_pool")
    assert a[3].endswith("slots") and a[11].endswith("workspace") and a[13].endswith("stream")
    assert "#define PREGO_ABI_VERSION 7" in hdr


def test_python_surface():
    import prego_amd.model as M
    from prego_amd.stream_pool import StreamPool
    assert callable(M.MROAD.stream_pool) and callable(M.MROADA.stream_pool)
    for name in ("open", "push", "vote", "events", "close", "state", "free", "capacity"):
        assert hasattr(StreamPool, name)
