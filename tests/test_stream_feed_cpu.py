"""CPU side of the stream pools' event feed (prego_amd/stream_pool.py: FeedModel, EventFeed; csrc/stream_feed.hip): `FeedModel` - the host
model tests/test_gpu_stream_feed.py holds the device against - delivers, over all drains of a stream plus its close, exactly the sequence
`aggregate_online` gives for the stream's ids, cuts a report at max_out and goes on from the cut, forgets and notices a reset; the entry
points are declared and bound."""
import os
import random
import re

import pytest

from prego_amd.aggregate import OVERFLOW_BAD_ID, OVERFLOW_FULL, OnlineRecord, aggregate_online
from prego_amd.stream_pool import FEED_REP_SHIFT, FeedModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sequence(rec):
    """a record's events as the feed numbers them: (index, step id, first frame)"""
    return [(i, e, s) for i, (e, s) in enumerate(zip(rec.event_id, rec.event_start))]


def test_all_drains_of_a_stream_plus_close_are_its_sequence_under_churn():
    rng = random.Random(3)
    cap, window, ncls = 7, 3, 5
    records = [OnlineRecord(window, ncls, 64) for _ in range(cap)]
    model = FeedModel(records, max_out=1024)
    live, fed, got, closed, seq = {}, {}, {}, 0, 0                           # slot -> stream number; stream -> ids / drained entries
    n_streams = 0
    for tick in range(120):
        for slot in range(cap):
            if slot not in live and rng.random() < 0.15:                    # open
                live[slot] = n_streams
                fed[n_streams], got[n_streams] = [], []
                n_streams += 1
        for slot in [s for s in live if rng.random() < 0.7]:
            i = rng.randrange(ncls)
            records[slot].push(i)
            fed[live[slot]].append(i)
        if rng.random() < 0.8:
            r = model.drain()
            seq += 1
            assert r["seq"] == seq and r["pending"] == 0 and r["count"] == len(r["entries"])
            assert r["entries"] == sorted(r["entries"])                      # ascending slot, then ascending index
            for slot, index, step, start in r["entries"]:
                got[live[slot]].append((index, step, start))
        for slot in [s for s in live if len(fed[live[s]]) >= 4 and rng.random() < 0.1]:       # close: flush, read, reset, forget
            stream = live.pop(slot)
            records[slot].flush()
            whole = _sequence(records[slot])
            want = aggregate_online(fed[stream], window, ncls)
            assert [e for _, e, _ in whole] == want["pred"] and [s for _, _, s in whole][1:] + [len(fed[stream])] == want["changes_pred"]
            assert got[stream] == whole[:len(got[stream])], stream           # no gap, no duplicate, nothing that is not in the sequence
            assert len(whole) - len(got[stream]) <= 2                        # close adds what came after the last drain
            records[slot] = OnlineRecord(window, ncls, 64)
            model.forget([slot])
            closed += 1
    assert closed >= 8 and n_streams > cap                                   # slots were reused
    assert any(len(v) >= 3 for v in got.values())


def test_the_max_out_cut_and_its_continuation():
    records = [OnlineRecord(1, 8, 16) for _ in range(6)]
    for slot, ids in {0: [1, 2], 2: [3], 3: [4, 5, 4, 5], 4: [6, 7, 6], 5: [0, 1]}.items():      # window 1: every change is an event
        for i in ids:
            records[slot].push(i)
    want = [(s, i, e, st) for s in range(6) for i, e, st in _sequence(records[s])]
    assert len(want) == 12
    model, whole = FeedModel(records, max_out=5), []
    for count, pending in ((5, 7), (5, 2), (2, 0), (0, 0)):
        r = model.drain()
        assert (r["count"], r["pending"]) == (count, pending)
        whole += r["entries"]
    assert whole == want
    assert whole[4][0] == 3 and whole[5][0] == 3                             # slot 3's four events straddle the first cut
    assert model.delivered == [2, 0, 1, 4, 3, 2]
    with pytest.raises(ValueError, match="max_out 0"):
        FeedModel(records, max_out=0)


def test_overflow_entries_come_once_and_in_front_of_the_slots_events():
    records = [OnlineRecord(1, 4, 2) for _ in range(3)]
    model = FeedModel(records)
    for i in (0, 1, 0):                                                      # the third event finds the record full
        records[1].push(i)
    records[2].push(9)                                                       # an id outside the classes: nothing counted
    assert model.drain()["entries"] == [(1, -1, OVERFLOW_FULL, 3), (1, 0, 0, 0), (1, 1, 1, 1), (2, -1, OVERFLOW_BAD_ID, 0)]
    assert model.cursor(1) == 2 | OVERFLOW_FULL << FEED_REP_SHIFT
    assert model.drain()["entries"] == []
    records[1].push(7)                                                       # the other bit of slot 1: reported alone
    assert model.drain()["entries"] == [(1, -1, OVERFLOW_BAD_ID, 3)]
    assert model.drain()["count"] == 0


def test_forget_and_the_reset_rule():
    records = [OnlineRecord(1, 4, 8) for _ in range(2)]
    model = FeedModel(records)
    for i in (0, 1, 2):
        records[0].push(i)
        records[1].push(i)
    assert model.drain()["count"] == 6
    model.forget([1])                                                        # the record still holds its events: they come again
    assert model.drain()["entries"] == [(1, 0, 0, 0), (1, 1, 1, 1), (1, 2, 2, 2)]
    records[0] = OnlineRecord(1, 4, 8)                                       # a reset behind the feed's back
    records[0].push(3)
    assert model.drain()["entries"] == [(0, 0, 3, 0)]                        # n_events 1 < delivered 3: the cursor restarted at 0
    records[1] = OnlineRecord(1, 4, 8)
    assert model.drain()["entries"] == [] and model.delivered == [1, 0]
    records[1].push(5)                                                       # a reported overflow bit that is gone is a reset too
    assert model.drain()["entries"] == [(1, -1, OVERFLOW_BAD_ID, 0)]
    records[1] = OnlineRecord(1, 4, 8)
    records[1].push(2)
    assert model.drain()["entries"] == [(1, 0, 2, 0)] and model.reported == [0, 0]
    records[1].push(6)
    assert model.drain()["entries"] == [(1, -1, OVERFLOW_BAD_ID, 1)]


def _args(hdr, name):
    m = re.search(r"\b(?:int|size_t|void)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/prego_amd.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_entry_points_are_declared_and_bound():
    from prego_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "prego_amd.h")).read()
    want = {"prego_stream_pool_feed_bytes": 2, "prego_stream_pool_feed_report_bytes": 1, "prego_stream_pool_feed_create": 6,
            "prego_vit_stream_pool_feed_create": 6, "prego_stream_pool_feed_destroy": 1, "prego_stream_pool_feed_drain": 4,
            "prego_stream_pool_feed_forget": 4}
    for name, n_args in want.items():
        assert len(_args(hdr, name)) == n_args, name
        assert name in _lib.SYMBOLS
    assert "const prego_stream_pool*" in _args(hdr, "prego_stream_pool_feed_create")[1]
    assert "const prego_vit_stream_pool*" in _args(hdr, "prego_vit_stream_pool_feed_create")[1]
    a = _args(hdr, "prego_stream_pool_feed_drain")
    assert a[1].endswith("report") and a[2].endswith("report_bytes") and a[3].endswith("stream")
    assert "#define PREGO_ABI_VERSION 7" in hdr


def test_python_surface():
    from prego_amd.stream_pool import EventFeed, FeedTicket, StreamPool, TransformerStreamPool
    for pool in (StreamPool, TransformerStreamPool):
        assert callable(pool.event_feed)
    for name in ("drain", "forget"):
        assert hasattr(EventFeed, name)
    for name in ("ready", "events", "pending"):
        assert hasattr(FeedTicket, name)
