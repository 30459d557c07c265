"""The stream pools' event feed (prego_stream_pool_feed_*, `pool.event_feed()`; csrc/stream_feed.hip) on the device.  Every comparison is
of integers and exact.  Ids go through `pool.vote`, so no model time is spent, and a host mirror - one `OnlineRecord` per slot fed the same
ids, under a `FeedModel` - says what every report must hold:
  1. churn at capacity 37 (one workgroup, no multiple of a wave): every report of ~40 ticks equals the model's;
  2. capacity 777 = four workgroups of 256 slots: events on both sides of every workgroup boundary, a tick without events, a tick with an
     event in every slot;  3. max_out 5 with 12 events due: 5 + 5 + 2, the tails intact;  4. overflow entries, once;  5. a closed slot and
     a raw reset start again at index 0;  6. the pool is only read, refusals write nothing;  7. no allocation, no host wait;
  8. the tickets;  9. through the models (MiniROAD: push, push_frames, push_ragged; Transformer: push, push_bursts) the union of all
     drained entries of a slot is what `pool.events(slot)`, the existing reader, returns."""
import ctypes as C
import random

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import _lib                                            # noqa: E402
from prego_amd._lib import PregoError                                 # noqa: E402
from prego_amd.aggregate import OVERFLOW_BAD_ID, OVERFLOW_FULL, OnlineRecord, aggregate_online   # noqa: E402
from prego_amd.stream_pool import FeedModel, StreamPool               # noqa: E402
from tests import test_gpu_step_wide as TW                            # noqa: E402  the engines are built once and shared

DEV = "cuda:0"
EINVAL, EWORKSPACE = -1, -3
NCLS = 86
WG = 256                                                              # slots one workgroup of the drain handles per trip (kFeedWg)


def _mirror(pool, max_out):
    records = [OnlineRecord(pool.window, NCLS, pool.max_events) for _ in range(pool.capacity)]
    return records, FeedModel(records, max_out)


def _vote(pool, records, votes):
    """votes: {slot: id}, at most 256 per call on the device"""
    slots = list(votes)
    for a in range(0, len(slots), 256):
        pool.vote(slots[a:a + 256], [votes[s] for s in slots[a:a + 256]])
    for s, i in votes.items():
        records[s].push(i)


def _same(ticket, want):
    got = {"count": ticket.count, "pending": ticket.pending, "seq": ticket.seq, "entries": ticket.entries}
    assert got == want, (got, want)
    return got


def _sequence(rec):
    return [(i, e, s) for i, (e, s) in enumerate(zip(rec.event_id, rec.event_start))]


# ---- 1. churn --------------------------------------------------------------------------------------------------------------------------------
def test_every_report_equals_the_models_under_churn():
    e = TW._real_engine("bf16", 3)
    pool = StreamPool(e, capacity=37, window=3, max_events=8)
    feed = pool.event_feed(max_out=64, depth=2)
    records, model = _mirror(pool, 64)
    rng = random.Random(17)
    open_at = {t: rng.randint(2, 6) for t in range(0, 40, 4)}               # streams opened at staggered ticks
    age, fed, got, n_closed, n_entries = {}, {}, {}, 0, 0
    for tick in range(40):
        for _ in range(open_at.get(tick, 0)):
            s = pool.open()
            age[s], fed[s], got[s] = 0, [], []
        votes = {s: rng.randrange(3) for s in age if rng.random() < 0.8}
        if votes:
            _vote(pool, records, votes)
            for s, i in votes.items():
                fed[s].append(i)
                age[s] += 1
        r = _same(feed.drain(), model.drain())
        assert r["pending"] == 0 and r["seq"] == tick + 1 and r["entries"] == sorted(r["entries"])
        n_entries += r["count"]
        for s, index, step, start in r["entries"]:
            got[s].append((index, step, start))
        for s in [s for s in age if age[s] >= 21 or (age[s] >= 5 and rng.random() < 0.12)]:      # at most 7 windows + the flushed one
            want = aggregate_online(fed[s], 3, NCLS)
            assert pool.close(s) == want
            whole = list(zip(range(len(want["pred"])), want["pred"], [0] + want["changes_pred"][:-1]))
            assert got[s] == whole[:len(got[s])] and len(whole) - len(got[s]) <= 1, s             # close adds the flushed last window
            records[s] = OnlineRecord(3, NCLS, 8)
            model.forget([s])
            del age[s]
            n_closed += 1
    assert n_closed >= 10 and n_entries >= 60 and pool.free < 37
    assert max(got) >= 10                                                     # slots beyond the first few were in use


# ---- 2. more than one workgroup ------------------------------------------------------------------------------------------------------------
def test_four_workgroups_boundaries_an_empty_tick_and_a_full_one():
    cap = 777
    assert cap >= 600 and cap >= 2 * WG + 1
    e = TW._real_engine("bf16", 3)
    pool = StreamPool(e, capacity=cap, window=1, max_events=4)
    feed = pool.event_feed(max_out=1024, depth=2)
    records, model = _mirror(pool, 1024)
    for _ in range(cap):
        pool.open()
    edge = [0, WG - 1, WG, 2 * WG - 1, 2 * WG, 3 * WG - 1, 3 * WG, cap - 1]  # the first, the last, both sides of every boundary
    _vote(pool, records, {s: 1 + s % 5 for s in edge})
    r = _same(feed.drain(), model.drain())
    assert [x[0] for x in r["entries"]] == edge and r["seq"] == 1
    _vote(pool, records, {s: 1 + s % 5 for s in edge})                       # the same ids again: frames advance, no event
    k = feed._next
    feed._dev[k].fill_(0x5A)
    r = _same(feed.drain(), model.drain())
    assert r["count"] == 0 and r["seq"] == 2
    words = feed._dev[k].view(torch.int32).cpu()
    assert words[:4].tolist() == [0, 0, 2, 0] and bool((words[4:] == 0x5A5A5A5A).all())      # the header alone was written
    _vote(pool, records, {s: 7 + s % 3 for s in range(cap)})                 # a new event in every slot
    r = _same(feed.drain(), model.drain())
    assert r["count"] == cap and [x[0] for x in r["entries"]] == list(range(cap))
    assert {x[1] for x in r["entries"]} == {0, 1} and r["pending"] == 0
    assert _same(feed.drain(), model.drain())["count"] == 0


# ---- 3. the cut --------------------------------------------------------------------------------------------------------------------------------
def test_max_out_5_with_12_events_due():
    e = TW._real_engine("bf16", 3)
    pool = StreamPool(e, capacity=6, window=1, max_events=16)
    feed = pool.event_feed(max_out=5, depth=3)
    records, model = _mirror(pool, 5)
    for _ in range(6):
        pool.open()
    streams = {0: [1, 2], 2: [3], 3: [4, 5, 4, 5], 4: [6, 7, 6], 5: [0, 1]}
    for t in range(4):
        _vote(pool, records, {s: ids[t] for s, ids in streams.items() if len(ids) > t})
    want = [(s, i, ev, st) for s in range(6) for i, ev, st in _sequence(records[s])]
    assert len(want) == 12 and want[3][0] == want[6][0] == 3                 # slot 3's four events straddle the first cut
    for buf in feed._dev:
        buf.fill_(0xC3)
    whole = []
    for k, (count, pending) in enumerate(((5, 7), (5, 2), (2, 0))):
        r = _same(feed.drain(), model.drain())
        assert (r["count"], r["pending"], r["seq"]) == (count, pending, k + 1)
        whole += r["entries"]
        words = feed._dev[k].view(torch.int32).cpu()
        assert bool((words[4 + 4 * count:] == -0x3C3C3C3D).all()), "written behind entry `count`"      # 0xC3C3C3C3 as int32
    assert whole == want
    assert [t.events() for t in feed._tickets] and _same(feed.drain(), model.drain())["count"] == 0


# ---- 4. overflow entries -----------------------------------------------------------------------------------------------------------------------
def test_overflow_entries_come_once_and_the_events_still_arrive():
    e = TW._real_engine("bf16", 3)
    pool = StreamPool(e, capacity=5, window=1, max_events=2)
    feed = pool.event_feed(max_out=16, depth=2)
    records, model = _mirror(pool, 16)
    a, b, c = pool.open(), pool.open(), pool.open()
    _vote(pool, records, {a: 4, b: NCLS, c: 1})                              # b: an id outside the classes, nothing counted
    _vote(pool, records, {b: 2})
    t = feed.drain()
    r = _same(t, model.drain())
    assert r["entries"] == [(a, 0, 4, 0), (b, -1, OVERFLOW_BAD_ID, 1), (b, 0, 2, 0), (c, 0, 1, 0)]
    with pytest.raises(PregoError, match=r"slot 1 was fed a step id outside \[0, 86\)"):
        t.events()
    for i in (0, 1):                                                         # c: a second event fills the record, the third is dropped
        _vote(pool, records, {c: i})
    t = feed.drain()
    r = _same(t, model.drain())
    assert r["entries"] == [(c, -1, OVERFLOW_FULL, 3), (c, 1, 0, 1)]
    with pytest.raises(PregoError, match="slot 2 produced more than max_events = 2 events"):
        t.events()
    with pytest.raises(PregoError, match="max_events = 2"):                  # events()' wording: the same reader, the same words
        pool.events(c)
    _vote(pool, records, {a: 4, c: 1})                                       # nothing new: the bits are not reported again
    t = feed.drain()
    assert _same(t, model.drain())["count"] == 0 and t.events() == []


# ---- 5. reuse ----------------------------------------------------------------------------------------------------------------------------------
def test_a_closed_slot_and_a_raw_reset_start_again_at_index_0():
    e = TW._real_engine("bf16", 3)
    pool = StreamPool(e, capacity=4, window=1, max_events=8)
    feed = pool.event_feed(max_out=16)
    records, model = _mirror(pool, 16)
    s, other = pool.open(), pool.open()
    for i in (3, 4, 5):
        _vote(pool, records, {s: i, other: i + 1})
    assert feed.drain().events() == model.drain()["entries"] and model.delivered[:2] == [3, 3]
    assert pool.close(s) == {"pred": [3, 4, 5], "changes_pred": [1, 2, 3]}   # close has the feed forget the slot
    records[s] = OnlineRecord(1, NCLS, 8)
    model.forget([s])
    assert pool.open() == s
    _vote(pool, records, {s: 9, other: 0})
    assert feed.drain().events() == model.drain()["entries"] == [(s, 0, 9, 0), (other, 3, 0, 3)]
    # a reset behind the feed's back: the cursor (3 delivered) is above n_events, an in-bounds but inconsistent pair
    arr = (C.c_int32 * 1)(other)
    assert e.lib.prego_stream_pool_reset(pool.p, 1, arr, None) == 0
    records[other] = OnlineRecord(1, NCLS, 8)
    assert _same(feed.drain(), model.drain())["count"] == 0 and model.delivered[other] == 0
    _vote(pool, records, {other: 6})
    assert feed.drain().events() == model.drain()["entries"] == [(other, 0, 6, 0)]
    cur = feed._block[:16].view(torch.int32).cpu().tolist()
    assert cur == [model.cursor(k) for k in range(4)] == [1, 1, 0, 0]


# ---- 6. the pool is only read, refusals write nothing ------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _slots(*s):
    return (C.c_int32 * len(s))(*s)


def test_refusals_and_what_a_drain_leaves_untouched():
    e = TW._real_engine("bf16", 3)
    lib = e.lib
    err = lambda: lib.prego_last_error().decode()
    cap, max_out = 300, 8
    need_pool = lib.prego_stream_pool_bytes(e.h, cap, 4)
    pblock = torch.full((need_pool,), 0xA5, dtype=torch.uint8, device=DEV)
    p = C.c_void_p()
    assert lib.prego_stream_pool_create(C.byref(p), e.h, cap, 1, 4, _p(pblock), need_pool, None) == 0
    need, rbytes = lib.prego_stream_pool_feed_bytes(cap, max_out), lib.prego_stream_pool_feed_report_bytes(max_out)
    assert need >= cap * 4 + 4 and need % 256 == 0 and rbytes >= (1 + max_out) * 16 and rbytes % 256 == 0
    assert lib.prego_stream_pool_feed_bytes(0, 8) == 0 and lib.prego_stream_pool_feed_bytes(8, 0) == 0
    assert lib.prego_stream_pool_feed_report_bytes(0) == 0
    fblock = torch.full((need + 512,), 0x77, dtype=torch.uint8, device=DEV)
    report = torch.full((rbytes + 512,), 0x3C, dtype=torch.uint8, device=DEV)
    assert fblock.data_ptr() % 256 == 0 and report.data_ptr() % 256 == 0
    f = C.c_void_p()
    for args, rc, msg in (((p, 0, _p(fblock), need), EINVAL, "max_out 0"), ((None, max_out, _p(fblock), need), EINVAL, "pool is NULL"),
                          ((p, max_out, None, need), EINVAL, "block is NULL"),
                          ((p, max_out, C.c_void_p(fblock.data_ptr() + 16), need), EINVAL, "256-byte aligned"),
                          ((p, max_out, _p(fblock), need - 1), EWORKSPACE, f"need {need}")):
        assert lib.prego_stream_pool_feed_create(C.byref(f), *args, None) == rc and msg in err() and not f.value, msg
    assert lib.prego_stream_pool_feed_create(None, p, max_out, _p(fblock), need, None) == EINVAL and "out is NULL" in err()
    torch.cuda.synchronize()
    assert bool((fblock == 0x77).all())
    assert lib.prego_stream_pool_feed_create(C.byref(f), p, max_out, _p(fblock), need, None) == 0
    torch.cuda.synchronize()
    assert not bool(fblock[:need].any()) and bool((fblock[need:] == 0x77).all())           # create zeroes exactly the feed block
    ids = torch.tensor([5, 6, 7], dtype=torch.int32, device=DEV)
    assert lib.prego_stream_pool_vote(p, 3, _slots(2, 255, 256), _p(ids), None) == 0
    torch.cuda.synchronize()
    snaps = [t.clone() for t in (pblock, fblock, report)]

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(t, s) for t, s in zip((pblock, fblock, report), snaps))

    drain = lambda feed=f, rep=_p(report), nb=rbytes: lib.prego_stream_pool_feed_drain(feed, rep, nb, None)
    for kw, rc, msg in ((dict(feed=None), EINVAL, "feed is NULL"), (dict(rep=None), EINVAL, "report is NULL"),
                        (dict(rep=C.c_void_p(report.data_ptr() + 16)), EINVAL, "256-byte aligned"),
                        (dict(nb=rbytes - 1), EWORKSPACE, f"need {rbytes}"), (dict(nb=0), EWORKSPACE, f"need {rbytes}")):
        assert drain(**kw) == rc and msg in err(), (kw, err())
        assert untouched(), kw
    forget = lambda feed=f, n=2, slots=_slots(1, 2): lib.prego_stream_pool_feed_forget(feed, n, slots, None)
    for kw, msg in ((dict(feed=None), "feed is NULL"), (dict(slots=None), "slots is NULL"), (dict(n=0), "0 slots"),
                    (dict(n=257, slots=_slots(*range(257))), "257 slots"), (dict(slots=_slots(1, cap)), f"slots[1] = {cap} is outside the pool"),
                    (dict(slots=_slots(-1, 2)), "slots[0] = -1 is outside the pool"), (dict(slots=_slots(2, 2)), "slot 2 is named twice")):
        assert forget(**kw) == EINVAL and msg in err(), (kw, err())
        assert untouched(), kw
    assert drain() == 0                                                      # after the refusals a valid drain works
    torch.cuda.synchronize()
    assert torch.equal(pblock, snaps[0]), "the drain wrote the pool's block"
    assert bool((fblock[need:] == 0x77).all()) and bool((report[rbytes:] == 0x3C).all())
    words = report[:rbytes].view(torch.int32).cpu()
    assert words[:16].tolist() == [3, 0, 1, 0, 2, 0, 5, 0, 255, 0, 6, 0, 256, 0, 7, 0]
    assert bool((words[16:] == 0x3C3C3C3C).all())
    assert fblock[:need].view(torch.int32)[[2, 255, 256]].cpu().tolist() == [1, 1, 1]
    assert forget(n=2, slots=_slots(256, 2)) == 0 and drain() == 0           # forgotten, the events of a record that was not reset come again
    torch.cuda.synchronize()
    assert report[:64].view(torch.int32).cpu().tolist() == [2, 0, 2, 0, 2, 0, 5, 0, 256, 0, 7, 0, 256, 0, 7, 0]
    assert torch.equal(pblock, snaps[0])
    lib.prego_stream_pool_feed_destroy(f)
    lib.prego_stream_pool_destroy(p)


# ---- 7. no allocation, no host wait --------------------------------------------------------------------------------------------------------------
def test_drain_and_forget_allocate_nothing_and_wait_for_nothing():
    dbg = _lib.load_debug()
    e = TW._real_engine("bf16", 8, lib=dbg)
    pool = StreamPool(e, capacity=600, window=1)
    assert pool.lib is dbg
    slots = [pool.open() for _ in range(600)][::7]
    pool.vote(slots, [3] * len(slots))
    f = C.c_void_p()
    need, rbytes = dbg.prego_stream_pool_feed_bytes(600, 128), dbg.prego_stream_pool_feed_report_bytes(128)
    fblock, report = torch.empty(need, dtype=torch.uint8, device=DEV), torch.empty(rbytes, dtype=torch.uint8, device=DEV)
    assert dbg.prego_stream_pool_feed_create(C.byref(f), pool.p, 128, _p(fblock), need, None) == 0
    assert dbg.prego_stream_pool_feed_drain(f, _p(report), rbytes, None) == 0
    torch.cuda.synchronize()

    def counts():
        a, w = C.c_int64(), C.c_int64()
        assert dbg.prego_debug_alloc_count(C.byref(a), C.byref(w)) == 0
        return a.value, w.value
    n0 = counts()
    assert dbg.prego_stream_pool_feed_drain(f, _p(report), rbytes, None) == 0
    assert dbg.prego_stream_pool_feed_forget(f, 3, _slots(0, 7, 599), None) == 0
    assert counts() == n0                                    # no device allocation and no host wait inside the calls
    torch.cuda.synchronize()
    assert report[:16].view(torch.int32).cpu().tolist() == [0, 0, 2, 0]
    dbg.prego_stream_pool_feed_destroy(f)


# ---- 8. the tickets ------------------------------------------------------------------------------------------------------------------------------
def test_tickets_become_ready_and_unread_tickets_stop_the_drain():
    e = TW._real_engine("bf16", 3)
    pool = StreamPool(e, capacity=4, window=1, max_events=8)
    feed = pool.event_feed(max_out=4, depth=2)
    s = pool.open()
    pool.vote([s], [1])
    t1 = feed.drain()
    pool.vote([s], [2])
    t2 = feed.drain()
    torch.cuda.synchronize()
    assert t1.ready() and t2.ready()
    pool.vote([s], [3])
    with pytest.raises(PregoError, match="all 2 report buffers hold unread tickets"):
        feed.drain()
    assert t1.pending == 0 and t1.events() == [(s, 0, 1, 0)]                 # `pending` alone does not hand the buffer back
    t3 = feed.drain()
    assert t3.seq == 3, "the refused drain launched something"
    assert t2.events() == [(s, 1, 2, 1)] and t3.events() == [(s, 2, 3, 2)] and t3.ready()
    with pytest.raises(PregoError, match="depth 0"):
        pool.event_feed(depth=0)
    with pytest.raises(PregoError, match="max_out 0"):
        pool.event_feed(max_out=0)


# ---- 9. through the models: the union of the drains is what events(slot) reads ----------------------------------------------------------------------
def _union_is_events(pool, drained, slots):
    n = 0
    for s in slots:
        ev = pool.events(s)
        got = sorted(x for x in drained if x[0] == s)
        assert [x[1] for x in got] == list(range(len(got))), s               # no gap, no duplicate
        assert [x[2] for x in got] == ev["pred"], s
        assert [x[3] for x in got] == ([0] + ev["changes_pred"][:-1] if got else []), s
        n += len(got)
    assert len(drained) == n
    return n


def test_miniroad_pool_push_push_frames_and_push_ragged_feed_one_feed():
    e = TW._real_engine("bf16", 3)
    pool = StreamPool(e, capacity=16, window=2)
    feed = pool.event_feed(max_out=64)
    slots = [pool.open() for _ in range(6)][::-1][:4]                        # 5, 4, 3, 2
    scale = torch.arange(1, 5, device=DEV, dtype=torch.float32)
    drained = []
    for t in range(3):
        pool.push(slots, TW._feat((4, 2048), 500 + t) * scale[:, None], None, want_ant=False)
        drained += feed.drain().events()
        pool.push_frames(slots[:3], TW._feat((3, 3, 2048), 510 + t) * scale[:3, None, None], None, want_ant=False)
        drained += feed.drain().events()
        counts = [1, 2, 3, 4]
        pool.push_ragged(slots, counts, TW._feat((10, 2048), 520 + t) * (1 + t), None, want_ant=False)
        drained += feed.drain().events()
    assert pool.events(slots[0])["frames"] == 3 * (1 + 3 + 1) and pool.events(slots[3])["frames"] == 3 * (1 + 4)
    assert _union_is_events(pool, drained, slots) >= 4
    e.check()


def test_transformer_pool_push_and_push_bursts_feed_one_feed():
    from tests import test_gpu_vit_stream_pool as VT
    m = VT._model()
    pool = m.stream_pool(capacity=8, vote_window=2, max_events=64)
    feed = pool.event_feed(max_out=64)
    slots = [pool.open() for _ in range(5)][::-1][:3]                        # 4, 3, 2
    vids = [(torch.from_numpy(r).to(DEV), torch.from_numpy(f).to(DEV)) for r, f in VT._videos()]
    at, drained = [0, 0, 0], []

    def rows(counts):
        rgb = torch.cat([vids[i][0][at[i]:at[i] + k] for i, k in enumerate(counts)]).contiguous()
        flow = torch.cat([vids[i][1][at[i]:at[i] + k] for i, k in enumerate(counts)]).contiguous()
        for i, k in enumerate(counts):
            at[i] += k
        return rgb, flow

    for t in range(3):
        pool.push(slots, *rows([1, 1, 1]))
        drained += feed.drain().events()
        counts = [1 + t, 3, 2]
        pool.push_bursts(slots, counts, *rows(counts))
        drained += feed.drain().events()
    assert [pool.events(s)["frames"] for s in slots] == at == [9, 12, 9]
    assert _union_is_events(pool, drained, slots) >= 3
