"""CPU side of the stream pools' slot images (prego_amd/stream_pool.py: PoolSnapshot, image_fault, model_image, FeedModel.seek;
prego_amd/aggregate.py: OnlineRecord.to_words / from_words; csrc/pool_image.h): the entry points are declared and bound; a record goes
through its device words and back at every point of a stream and carries on to `aggregate`'s result; the validity rule accepts every
image the model writes and names the clause of every broken word, and the Python statement of the rule agrees with the C++ one the
restore kernel evaluates; a snapshot goes through the host and a file; a feed model taken up at a cursor word delivers nothing twice."""
import ctypes as C
import os
import random
import re

import pytest

torch = pytest.importorskip("torch")

from prego_amd.aggregate import OVERFLOW_BAD_ID, OVERFLOW_FULL, OnlineRecord, aggregate, aggregate_online   # noqa: E402
from prego_amd import stream_pool as SP                              # noqa: E402
from prego_amd._lib import PregoError                                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRU = {"kind": 1, "dim": 1024, "window_size": 0, "n_classes": 86, "vote_window": 3, "max_events": 6}
VIT = {"kind": 2, "dim": 256, "window_size": 4, "n_classes": 7, "vote_window": 3, "max_events": 6}


def _args(hdr, name):
    m = re.search(r"\b(?:int|size_t|void)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/prego_amd.h"
    return [re.sub(r"/\*.*?\*/", "", a).strip() for a in m.group(1).split(",")]


def test_the_six_entry_points_are_declared_and_bound():
    from prego_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "prego_amd.h")).read()
    for pre, pool in (("prego_stream_pool", "prego_stream_pool*"), ("prego_vit_stream_pool", "prego_vit_stream_pool*")):
        a = _args(hdr, pre + "_image_bytes")
        assert a == [f"const {pool} p"]
        a = _args(hdr, pre + "_snapshot")
        assert a == [f"{pool} p", "const prego_stream_pool_feed* feed", "int n", "const int32_t* slots", "void* images", "size_t bytes",
                     "prego_stream_t stream"], a
        a = _args(hdr, pre + "_restore")
        assert a == [f"{pool} p", "prego_stream_pool_feed* feed", "int n", "const int32_t* slots", "const void* images", "size_t bytes",
                     "int32_t* status", "prego_stream_t stream"], a
        for name in ("_image_bytes", "_snapshot", "_restore"):
            assert pre + name in _lib.SYMBOLS
    assert re.search(r"size_t\s+prego_stream_pool_image_bytes", hdr) and re.search(r"size_t\s+prego_vit_stream_pool_image_bytes", hdr)
    assert "#define PREGO_ABI_VERSION 7" in hdr
    lib = _lib.load()
    vp, sz, i32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_int32)
    for pre in ("prego_stream_pool", "prego_vit_stream_pool"):
        assert getattr(lib, pre + "_image_bytes").argtypes == [vp] and getattr(lib, pre + "_image_bytes").restype is sz
        assert getattr(lib, pre + "_snapshot").argtypes == [vp, vp, C.c_int, i32p, vp, sz, vp]
        assert getattr(lib, pre + "_restore").argtypes == [vp, vp, C.c_int, i32p, vp, sz, vp, vp]
    for pool in (SP.StreamPool, SP.TransformerStreamPool):
        for name in ("snapshot", "restore", "detach", "image_geometry"):
            assert callable(getattr(pool, name))
        assert {"image_bytes", "snapshot", "restore"} <= set(pool._C)


def _stream(seed, n, ncls, bad_at=()):
    rng = random.Random(seed)
    ids = [rng.randrange(ncls) if rng.random() < 0.6 else 1 for _ in range(n)]
    for t in bad_at:
        ids[t] = ncls + 3
    return ids


@pytest.mark.parametrize("window,ncls,max_events,bad_at", [(3, 5, 64, ()), (4, 7, 3, ()), (1, 4, 64, ()), (3, 5, 64, (4, 9))],
                         ids=["w3", "w4-record-fills", "w1", "w3-bad-ids"])
def test_a_record_goes_through_its_words_at_every_point_and_carries_on(window, ncls, max_events, bad_at):
    ids = _stream(11, 29, ncls, bad_at)
    whole = OnlineRecord(window, ncls, max_events)
    points = set()
    for t in range(len(ids) + 1):
        w = whole.to_words()
        pad = (ncls + 3) // 4 * 4
        assert len(w) == (4 + pad + 2 * max_events + 3) // 4 * 4 and len(w) % 4 == 0
        assert w[0] == whole.frames and w[2] == len(whole.event_id) and w[3] == whole.overflow
        assert w[4 + pad + len(whole.event_id):4 + pad + max_events] == [0] * (max_events - len(whole.event_id))      # the tail is zero
        back = OnlineRecord.from_words(w, window, ncls, max_events)
        assert back.__dict__ == whole.__dict__, t
        assert back.to_words() == w
        points.add("mid" if whole.frames % window else "boundary")
        if whole.overflow:
            points.add("overflow")
        for i in ids[t:]:                                                    # the rebuilt record fed the rest of the stream
            back.push(i)
        rest = OnlineRecord(window, ncls, max_events)
        for i in ids:
            rest.push(i)
        assert back.__dict__ == rest.__dict__, t
        back.flush()
        rest.flush()
        assert back.result() == rest.result()
        flushed = OnlineRecord.from_words(back.to_words(), window, ncls, max_events)       # after a flush
        assert flushed.__dict__ == back.__dict__, t
        if not back.overflow:
            good = [i for i in ids if i < ncls]
            want = aggregate({"v": {"pred": good, "gt": [0] * len(good)}}, window_size=window)["v"]
            assert back.result()["pred"] == want["pred"] and back.result()["changes_pred"] == want["changes_pred"]
            assert aggregate_online(good, window, ncls) == {"pred": want["pred"], "changes_pred": want["changes_pred"]}
        if t < len(ids):
            whole.push(ids[t])
    assert points >= ({"boundary"} if window == 1 else {"mid", "boundary"})
    if max_events == 3:
        assert whole.overflow & OVERFLOW_FULL
    if bad_at:
        assert whole.overflow & OVERFLOW_BAD_ID and "overflow" in points
    wider = whole.to_words(n_classes=ncls + 6, max_events=max_events + 2)      # into a pool of more classes and a longer record
    assert OnlineRecord.from_words(wider, window, ncls + 6, max_events + 2).result() == whole.result()
    with pytest.raises(ValueError, match="below the record's"):
        whole.to_words(n_classes=ncls - 1)
    with pytest.raises(ValueError, match="words"):
        OnlineRecord.from_words(wider[:-4], window, ncls + 6, max_events + 2)


def _cxx_fault(words, g):
    """csrc/pool_image.h: pool_image_fault through the debug library's host hook (no device)"""
    from prego_amd import _lib
    dbg = _lib.load_debug()
    lay = SP.image_layout(g)
    r0 = SP.IMAGE_TAG_WORDS + lay["state_words"]
    arr = lambda x: (C.c_int32 * len(x))(*[v - (1 << 32) if v >= 1 << 31 else v for v in x])
    geom = [g["kind"], g["dim"], g["window_size"], g["n_classes"], g["vote_window"], g["max_events"]]
    return dbg.prego_debug_pool_image_fault(arr(geom), arr(words[:16]), arr(words[r0:r0 + 4 + lay["ncls_pad"]]))


def _images(g):
    """every image of one seeded stream, with the cursor of a feed drained every other frame"""
    rec = OnlineRecord(g["vote_window"], g["n_classes"], g["max_events"])
    feed = SP.FeedModel([rec])
    out = [SP.model_image(g, rec)]
    for t in range(30):                                                      # every window votes another id than the one before: ten events
        rec.push(g["n_classes"] + 3 if t == 20 else (t // g["vote_window"]) % 3 if t % 3 else 1 + (t // g["vote_window"]) % 3)
        if t % 2:
            feed.drain()
        out.append(SP.model_image(g, rec, cursor_word=feed.cursor_word(0)))
    assert rec.overflow == (OVERFLOW_FULL | OVERFLOW_BAD_ID) and feed.cursor_word(0) >> SP.FEED_REP_SHIFT == 3
    return out


@pytest.mark.parametrize("g", [GRU, VIT], ids=["gru", "transformer"])
def test_the_rule_accepts_every_image_of_the_model(g):
    lay = SP.image_layout(g)
    assert lay["image_words"] % 64 == 0 and lay["state_words"] % 4 == 0 and lay["rec_words"] % 4 == 0
    for w in _images(g):
        assert len(w) == lay["image_words"] and w[12:16] == [0] * 4
        assert SP.image_fault(w, g) == 0 and _cxx_fault(w, g) == 0
        if g["kind"] == 2:
            assert (w[SP.TAG_HEAD], w[SP.TAG_FILL]) == (w[SP.TAG_FRAMES] % 4, min(w[SP.TAG_FRAMES], 4))
        else:
            assert (w[SP.TAG_HEAD], w[SP.TAG_FILL]) == (0, 0)


def _breaks(g):
    """(name, word index, new value or a function of the old one, the clause): one word of a good image broken at a time"""
    lay = SP.image_layout(g)
    r0 = SP.IMAGE_TAG_WORDS + lay["state_words"]
    cases = [("magic", 0, 0x12345678, SP.FAULT_GEOMETRY), ("version", 1, 2, SP.FAULT_GEOMETRY), ("kind", 2, 3 - g["kind"], SP.FAULT_GEOMETRY),
             ("dim", 3, g["dim"] * 2, SP.FAULT_GEOMETRY), ("window_size", 4, 8, SP.FAULT_GEOMETRY),
             ("n_classes", 5, g["n_classes"] + 1, SP.FAULT_GEOMETRY), ("vote window", 6, g["vote_window"] + 1, SP.FAULT_GEOMETRY),
             ("max_events", 7, g["max_events"] * 2, SP.FAULT_GEOMETRY),
             ("tag frames", SP.TAG_FRAMES, lambda v: v + g["window_size"] if g["kind"] == 2 else v + 1, SP.FAULT_FRAMES),
             ("negative frames", SP.TAG_FRAMES, -1, SP.FAULT_FRAMES), ("record frames", r0, lambda v: v - 1, SP.FAULT_FRAMES),
             ("n_events above", r0 + 2, g["max_events"] + 1, SP.FAULT_EVENTS), ("n_events huge", r0 + 2, 0x7fffffff, SP.FAULT_EVENTS),
             ("n_events negative", r0 + 2, -1, SP.FAULT_EVENTS | SP.FAULT_CURSOR),      # and the cursor stands above it
             ("last vote", r0 + 1, g["n_classes"] + 1, SP.FAULT_VOTE), ("last vote negative", r0 + 1, -1, SP.FAULT_VOTE),
             ("overflow", r0 + 3, 4, SP.FAULT_OVERFLOW), ("overflow negative", r0 + 3, -4, SP.FAULT_OVERFLOW),
             ("first counter", r0 + 4, g["vote_window"] + 1, SP.FAULT_COUNTER), ("last counter", r0 + 4 + g["n_classes"] - 1, -1, SP.FAULT_COUNTER),
             ("padding counter", r0 + 4 + lay["ncls_pad"] - 1, 1 << 30, SP.FAULT_COUNTER),
             ("cursor", SP.TAG_CURSOR, lambda v: (v & ~SP.FEED_COUNT_MASK) | ((v & SP.FEED_COUNT_MASK) + 4), SP.FAULT_CURSOR)]
    if g["kind"] == 2:
        cases += [("head", SP.TAG_HEAD, lambda v: (v + 1) % 4, SP.FAULT_RING), ("fill", SP.TAG_FILL, lambda v: v - 1, SP.FAULT_RING),
                  ("head outside", SP.TAG_HEAD, 4, SP.FAULT_RING), ("fill outside", SP.TAG_FILL, 5, SP.FAULT_RING)]
    return cases


@pytest.mark.parametrize("g", [GRU, VIT], ids=["gru", "transformer"])
def test_one_broken_word_names_its_clause(g):
    good = _images(g)[11]                                                    # mid window, events in the record, a cursor behind them
    assert good[SP.TAG_FRAMES] % g["vote_window"] and good[SP.TAG_CURSOR] & SP.FEED_COUNT_MASK
    seen = 0
    for name, at, new, clause in _breaks(g):
        w = list(good)
        w[at] = new(w[at]) if callable(new) else new
        assert w != good, name
        assert SP.image_fault(w, g) == clause, name                          # that clause and no other
        assert _cxx_fault(w, g) == clause, name
        assert SP.image_fault_names(clause) == [SP.IMAGE_FAULTS[b] for b in SP.IMAGE_FAULTS if clause & b]
        seen |= clause
    assert seen == (255 if g["kind"] == 2 else 255 - SP.FAULT_RING)
    w = list(good)
    w[0], w[SP.TAG_CURSOR] = 0, 1 << 20
    assert SP.image_fault(w, g) == _cxx_fault(w, g) == SP.FAULT_GEOMETRY | SP.FAULT_CURSOR
    assert SP.image_fault_names(SP.FAULT_GEOMETRY | SP.FAULT_CURSOR) == ["geometry", "feed cursor"]
    state_word = SP.IMAGE_TAG_WORDS + 1                                      # the state is data: no word of it is judged
    w = list(good)
    w[state_word] = -1
    assert SP.image_fault(w, g) == 0 and _cxx_fault(w, g) == 0


def test_snapshot_through_the_host_and_a_file(tmp_path):
    g = VIT
    words = torch.tensor(_images(g)[9:12], dtype=torch.int32)
    snap = SP.PoolSnapshot(words.view(torch.uint8).reshape(3, -1).clone(), g, "fp16")
    assert snap.n == 3 and snap.frames() == [9, 10, 11] and snap.device.type == "cpu"
    assert snap.geometry == g and all(type(v) is int for v in snap.geometry.values())
    again = snap.cpu()
    assert torch.equal(again.images, snap.images) and again.geometry == g and again.compute_dtype == "fp16"
    path = tmp_path / "pool.snap"
    snap.save(path)
    raw = torch.load(path, weights_only=True)                                # a plain dict of tensors, ints and strings
    assert set(raw) == {"format", "images", "geometry", "compute_dtype", "n"} and raw["n"] == 3 and raw["geometry"] == g
    back = SP.PoolSnapshot.load(path)
    assert torch.equal(back.images, snap.images) and back.geometry == g and back.compute_dtype == "fp16" and back.n == 3
    assert [SP.image_fault(w.tolist(), g) for w in back.words()] == [0, 0, 0]
    torch.save({"format": "something else"}, path)
    with pytest.raises(PregoError, match="not a saved PoolSnapshot"):
        SP.PoolSnapshot.load(path)
    with pytest.raises(PregoError, match="uint8"):
        SP.PoolSnapshot(words, g, "fp16")
    with pytest.raises(PregoError, match="bytes, the geometry"):
        SP.PoolSnapshot(snap.images[:, :-256], g, "fp16")


def test_a_feed_model_taken_up_at_a_cursor_word_delivers_nothing_twice():
    window, ncls = 2, 5
    ids = _stream(23, 40, ncls)
    rec_a = OnlineRecord(window, ncls, 64)
    feed_a = SP.FeedModel([OnlineRecord(window, ncls, 64), rec_a])          # the stream lives in slot 1 of A
    first = []
    for i in ids[:21]:                                                       # 21 frames: mid window
        rec_a.push(i)
    first += feed_a.drain()["entries"]
    for i in ids[21:25]:                                                     # events the consumer has not heard yet travel along
        rec_a.push(i)
    word = feed_a.cursor_word(1)
    assert word == feed_a.cursor(1) == len(first) and len(rec_a.event_id) > len(first) >= 3
    rec_b = OnlineRecord.from_words(rec_a.to_words(), window, ncls, 64)      # ... into slot 3 of B
    records_b = [OnlineRecord(window, ncls, 64) for _ in range(5)]
    records_b[3] = rec_b
    feed_b = SP.FeedModel(records_b)
    feed_b.seek(3, word)
    assert feed_b.cursor_word(3) == word
    for i in ids[25:]:
        rec_b.push(i)
    later = feed_b.drain()["entries"]
    rec_b.flush()
    later += feed_b.drain()["entries"]
    got = [(i, e, s) for _, i, e, s in first] + [(i, e, s) for _, i, e, s in later]
    want = aggregate_online(ids, window, ncls)
    assert [i for i, _, _ in got] == list(range(len(got)))                   # no event twice, none missing, the true indices
    assert [e for _, e, _ in got] == want["pred"] and [s for _, _, s in got][1:] + [len(ids)] == want["changes_pred"]
    assert all(slot == 3 for slot, *_ in later)
    fresh = SP.FeedModel(records_b)                                          # without a seek the slot is delivered from index 0
    assert [i for _, i, _, _ in fresh.drain()["entries"]] == list(range(len(rec_b.event_id)))
    full = OnlineRecord(1, 4, 2)                                             # the reported overflow bits travel in the word
    for i in (0, 1, 0):
        full.push(i)
    fa = SP.FeedModel([full])
    assert fa.drain()["entries"][0] == (0, -1, OVERFLOW_FULL, 3)
    fb = SP.FeedModel([OnlineRecord.from_words(full.to_words(), 1, 4, 2)])
    fb.seek(0, fa.cursor_word(0))
    assert fb.drain()["entries"] == [] and fb.cursor_word(0) == 2 | OVERFLOW_FULL << SP.FEED_REP_SHIFT
    fb.seek(0, (2 | OVERFLOW_FULL << SP.FEED_REP_SHIFT) - (1 << 32))         # the word as the int32 a tag holds
    assert fb.cursor_word(0) == 2 | OVERFLOW_FULL << SP.FEED_REP_SHIFT
