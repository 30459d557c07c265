"""Slot images of the stream pools on the device (pool.snapshot / restore / detach = prego_stream_pool_snapshot / _restore and their
prego_vit_ counterparts; csrc/stream_image.hip, csrc/pool_image.h).  Every comparison is exact (torch.equal, integers):
  a. GRU pool against the saturated-gate automaton: streams detached mid vote window from pool A, restored into pool B under other slot
     numbers and pushed on, equal the uninterrupted automaton after every push and `aggregate()` at close; the streams left in A go on;
  b. GRU pool on real weights: interrupted streams equal uninterrupted twins in a third pool - outputs, state, record words;
  c. Transformer pool: snapshot at fill < window_size, at fill == window_size with head != 0 and at frames == 0, restore elsewhere, push
     and push_bursts (a burst across the wrap) on: logits, argmax, window, ring words and record equal the uninterrupted pool's bytes;
  d. canonical bytes: a stream in a fresh slot and in a slot with stale ring rows gives one image, rows from fill on are zero;
  e. the host route (cpu, save, load, to) leaves the same bytes in a pool as the device route;
  f. refusals write nothing; for each clause of the validity rule one broken image between two good ones: its slot and feed cursor
     untouched, the clause in status, the neighbours restored, guards intact, pool.restore raises and leaves no slot open;
  g. a stream moved with its feed position: nothing delivered twice, true indices; without feed= it is delivered from index 0;
  h. no allocation, no host wait, no HIP error left behind."""
import ctypes as C
import random

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import _lib                                            # noqa: E402
from prego_amd import stream_pool as SP                               # noqa: E402
from prego_amd._lib import PregoError                                 # noqa: E402
from prego_amd.aggregate import OnlineRecord, aggregate               # noqa: E402
from prego_amd.engine import MiniRoadEngine                           # noqa: E402
from prego_amd.stream_pool import FeedModel, PoolSnapshot, StreamPool  # noqa: E402
from tests import test_gpu_step_wide as TW                            # noqa: E402  its references and engines are computed once and shared
from tests import test_gpu_vit_stream_pool as VT                      # noqa: E402

DEV = "cuda:0"
EINVAL, EWORKSPACE = -1, -3
NCLS = 86


def _agg(ids, window):
    a = aggregate({"v": {"pred": [int(i) for i in ids], "gt": [0] * len(ids)}}, window_size=window)["v"]
    return {"pred": a["pred"], "changes_pred": a["changes_pred"]}


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _arr(*s):
    return (C.c_int32 * len(s))(*s)


def _is_vit(pool):
    return isinstance(pool, SP.TransformerStreamPool)


def _slot_ranges(pool, slot):
    """the byte ranges of the pool's block that belong to a slot: (GRU) state row, record; (Transformer) ring rows, ring words, record"""
    if _is_vit(pool):
        return VT._slot_bytes(pool, slot)
    ptr, nb = C.c_void_p(), C.c_size_t()
    assert pool.lib.prego_stream_pool_record(pool.p, slot, C.byref(ptr), C.byref(nb)) == 0
    rec = ptr.value - pool._block.data_ptr()
    return [(slot * pool._hid * 4, (slot + 1) * pool._hid * 4), (rec, rec + nb.value)]


def _slot_bytes(pool, slot):
    return [pool._block[a:b].clone() for a, b in _slot_ranges(pool, slot)]


def _record_words(pool, slot):
    a, b = _slot_ranges(pool, slot)[-1]
    return pool._block[a:b].view(torch.int32).clone()


def _image_parts(pool, image):
    """what a restore of `image` (uint8 [image_bytes], device) leaves in a slot, part for part as _slot_ranges orders them"""
    lay = SP.image_layout(pool.image_geometry())
    w = image.view(torch.int32)
    s0 = SP.IMAGE_TAG_WORDS
    state, rec = w[s0:s0 + lay["state_words"]], w[s0 + lay["state_words"]:s0 + lay["state_words"] + lay["rec_words"]]
    if _is_vit(pool):
        hf = torch.stack([w[SP.TAG_HEAD], w[SP.TAG_FILL], torch.zeros_like(w[0]), torch.zeros_like(w[0])])
        return [state.view(torch.uint8), hf.view(torch.uint8), rec.view(torch.uint8)]
    return [state.view(torch.uint8), rec.view(torch.uint8)]


def _scattered(pool, n, seed):
    """n open slots of the pool, scattered and in a seeded order: the pool is filled and all but a sample are closed again"""
    rng = random.Random(seed)
    for _ in range(pool.capacity):
        pool.open()
    keep = rng.sample(range(pool.capacity), n)
    for s in set(range(pool.capacity)) - set(keep):
        pool.close(s)
    return keep


# ---- a. the automaton ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_detached_streams_go_on_in_another_pool_exactly_as_the_automaton(dtype):
    case, sd, n, T, x, res = TW._ref("L1-C12")
    L, Cn, window = case.ant_len, case.n_classes, 3
    e = MiniRoadEngine(case.d_rgb, case.d_flow, case.emb, case.hid, Cn, DEV, dtype)
    e.set_weights(sd)
    e.set_anticipation(sd[TW.A_KEYS[0]], sd[TW.A_KEYS[1]], L)
    want_l, want_a, want_h = (t.view(n, T, -1) for t in (res.logits, res.argmax, res.h[0]))
    want_al, want_aa = res.ant_logits.view(n, T, L, Cn), res.ant_argmax.view(n, T, L)
    pool_a = StreamPool(e, capacity=64, window=window, max_events=8)
    pool_b = StreamPool(e, capacity=200, window=window, max_events=8)
    rng = random.Random(7)                                                    # scattered slots: the pool is filled, a seeded sample is closed again
    for _ in range(64):
        pool_a.open()
    holes = rng.sample(range(64), n)
    for s in holes:
        pool_a.close(s)
    slot_of = {}                                                              # stream -> (pool, slot)
    frame = [0] * n

    def tick(pool, streams):
        slots = [slot_of[s][1] for s in streams]
        fr = [frame[s] for s in streams]
        got = pool.push(slots, torch.stack([x[s, f] for s, f in zip(streams, fr)]), None, softmax=False)
        si, fi = torch.tensor(streams, device=DEV), torch.tensor(fr, device=DEV)
        assert torch.equal(got[0].to(torch.float64), want_l[si, fi]), "logits"
        assert torch.equal(got[1], want_a[si, fi, 0]), "argmax"
        assert torch.equal(got[2].to(torch.float64), want_al[si, fi]), "anticipation logits"
        assert torch.equal(got[3], want_aa[si, fi]), "anticipation argmax"
        assert torch.equal(torch.stack([pool.state(s) for s in slots]), want_h[si, fi].to(torch.float32)), "state"
        for s in streams:
            frame[s] += 1

    t1 = 4
    for t in range(t1):                                                       # staggered: stream s opens at tick s % 3
        for s in range(n):
            if s % 3 == t:
                slot_of[s] = (pool_a, pool_a.open())
        tick(pool_a, [s for s in range(n) if s in slot_of])
    assert sorted(v[1] for v in slot_of.values()) == sorted(holes)
    moved = [s for s in range(n) if frame[s] % window != 0 and s % 2 == 0]    # taken mid vote window: 4 or 2 frames in
    assert len(moved) >= 4 and {frame[s] for s in moved} == {2, 4} and len(moved) < n - 4
    for _ in range(9):                                                        # other slot numbers in B: 0..8 are taken
        pool_b.open()
    free_before = pool_a.free
    snap = pool_a.detach([slot_of[s][1] for s in moved])
    assert snap.n == len(moved) and snap.frames() == [frame[s] for s in moved] and pool_a.free == free_before + len(moved)
    new = pool_b.restore(snap)
    assert new == list(range(9, 9 + len(moved)))
    for s, slot in zip(moved, new):
        assert slot != slot_of[s][1]
        slot_of[s] = (pool_b, slot)
    stay = [s for s in range(n) if s not in moved]
    while min(frame) < T:
        for pool, group in ((pool_a, stay), (pool_b, moved)):
            live = [s for s in group if frame[s] < T]
            if live:
                tick(pool, live)
    ids = want_a[:, :, 0].cpu().tolist()
    for s in range(n):
        pool, slot = slot_of[s]
        assert pool.close(slot) == _agg(ids[s], window), f"stream {s}"
    assert pool_a.free == n and pool_b.free == 200 - 9
    e.check()


# ---- b. real weights: interrupted streams and their uninterrupted twins ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,n", [(d, n) for d in ("bf16", "fp16") for n in (5, 37)], ids=lambda v: str(v))
def test_interrupted_streams_equal_their_uninterrupted_twins_on_real_weights(dtype, n):
    e = TW._real_engine(dtype, 3)
    pool_a, pool_b, pool_c = (StreamPool(e, capacity=c, window=3, max_events=16) for c in (64, 200, 64))
    slots_a, slots_c = _scattered(pool_a, n, n), _scattered(pool_c, n, n + 1)
    assert slots_a != slots_c

    def feats(t):
        return TW._feat((n, 2048), 310 + t), TW._feat((n, 2048), 320 + t)
    for t in range(2):                                                        # two frames: mid vote window
        rgb, flow = feats(t)
        pool_a.push(slots_a, rgb, flow)
        pool_c.push(slots_c, rgb, flow)
    snap = pool_a.snapshot(slots_a)
    assert snap.frames() == [2] * n and snap.compute_dtype == dtype
    before_a = pool_a._block.clone()
    for _ in range(3):
        pool_b.open()
    slots_b = pool_b.restore(snap)
    assert slots_b == list(range(3, 3 + n))
    assert torch.equal(pool_a._block, before_a), "snapshot or restore wrote the source pool"
    for t in range(2, 6):
        rgb, flow = feats(t)
        got, want = pool_b.push(slots_b, rgb, flow), pool_c.push(slots_c, rgb, flow)
        for name, g, w in zip(("out", "argmax", "ant_out", "ant_argmax"), got, want):
            assert torch.equal(g, w), f"tick {t}: {name}"
        for sb, sc in zip(slots_b, slots_c):
            assert torch.equal(pool_b.state(sb), pool_c.state(sc)), f"tick {t}: state"
            assert torch.equal(_record_words(pool_b, sb), _record_words(pool_c, sc)), f"tick {t}: record"
    assert int(_record_words(pool_b, slots_b[0])[0]) == 6 and int(_record_words(pool_b, slots_b[0])[2]) >= 1
    assert [pool_b.close(s) for s in slots_b] == [pool_c.close(s) for s in slots_c]
    e.check()


# ---- c. the Transformer pool ----------------------------------------------------------------------------------------------------------------------
_VIT = {}


def _vit(dtype="fp16"):
    if dtype not in _VIT:
        _VIT[dtype] = VT._model(1, dtype)
    return _VIT[dtype]


def _vit_rows(vids, at, streams, counts):
    rgb = torch.cat([vids[s][0][at[s]:at[s] + k] for s, k in zip(streams, counts)]).contiguous()
    flow = torch.cat([vids[s][1][at[s]:at[s] + k] for s, k in zip(streams, counts)]).contiguous()
    return rgb, flow


def _same_slot(pool_x, sx, pool_y, sy, what):
    wx, fx = pool_x.window(sx)
    wy, fy = pool_y.window(sy)
    assert fx == fy and torch.equal(wx, wy), f"{what}: window"
    bx, by = _slot_bytes(pool_x, sx), _slot_bytes(pool_y, sy)
    assert torch.equal(bx[1], by[1]), f"{what}: ring words"
    assert torch.equal(bx[2], by[2]), f"{what}: record"


@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_transformer_streams_restored_elsewhere_give_the_uninterrupted_pools_bytes(dtype):
    m = _vit(dtype)
    T = VT.WINDOW
    pool_u, pool_a, pool_b = (m.stream_pool(capacity=8, vote_window=3, max_events=32) for _ in range(3))
    vids = [(torch.from_numpy(r).to(DEV), torch.from_numpy(f).to(DEV)) for r, f in VT._videos()]
    slots_u = [pool_u.open() for _ in range(3)]                               # 0, 1, 2
    slots_a = [pool_a.open() for _ in range(6)][3:][::-1]                     # 5, 4, 3
    at = [0, 0, 0]
    for t in range(T + 8):                                                    # stream 0: 40 frames, stream 1: 20, stream 2: opened, no frame
        streams = [0, 1] if t < 20 else [0]
        rgb, flow = _vit_rows(vids, at, streams, [1] * len(streams))
        pool_u.push([slots_u[s] for s in streams], rgb, flow)
        pool_a.push([slots_a[s] for s in streams], rgb, flow)
        for s in streams:
            at[s] += 1
    snap = pool_a.snapshot(slots_a)
    assert snap.frames() == at == [T + 8, 20, 0]
    tags = snap.words()[:, :SP.IMAGE_TAG_WORDS].cpu().tolist()
    assert [(w[SP.TAG_HEAD], w[SP.TAG_FILL]) for w in tags] == [(8, T), (20, 20), (0, 0)]      # wrapped with head != 0; not full; empty
    assert tags[0][:8] == SP.image_geometry_words(pool_a.image_geometry())
    for _ in range(2):
        pool_b.open()
    slots_b = pool_b.restore(snap)
    assert slots_b == [2, 3, 4] and slots_b != slots_a
    for s in range(3):
        _same_slot(pool_b, slots_b[s], pool_u, slots_u[s], f"restored stream {s}")
    for t in range(5):                                                        # the same rows, the same n_active, the same order
        rgb, flow = _vit_rows(vids, at, [0, 1, 2], [1, 1, 1])
        want, got = pool_u.push(slots_u, rgb, flow), pool_b.push(slots_b, rgb, flow)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"push {t}"
        for s in range(3):
            at[s] += 1
            _same_slot(pool_b, slots_b[s], pool_u, slots_u[s], f"push {t}, stream {s}")
    counts = [3, 8, 2]                                                        # stream 1 stands at 25 frames: its burst crosses the wrap at 32
    assert at[1] < T < at[1] + counts[1]
    rgb, flow = _vit_rows(vids, at, [0, 1, 2], counts)
    want, got = pool_u.push_bursts(slots_u, counts, rgb, flow), pool_b.push_bursts(slots_b, counts, rgb, flow)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), "push_bursts"
    for s in range(3):
        _same_slot(pool_b, slots_b[s], pool_u, slots_u[s], f"push_bursts, stream {s}")
    again = pool_b.snapshot(slots_b[1:2])                                     # a snapshot of a restored, wrapped stream round-trips as well
    assert torch.equal(again.images, pool_u.snapshot(slots_u[1:2]).images)
    assert [pool_b.close(s) for s in slots_b] == [pool_u.close(s) for s in slots_u]


# ---- d. canonical bytes, e. the host route ----------------------------------------------------------------------------------------------------------
def _two_homes_of_one_stream(m):
    """pool with the same 5 frames in slot 0 (fresh) and slot 1 (held a 40-frame stream before: stale ring rows)"""
    pool = m.stream_pool(capacity=4, vote_window=2, max_events=32)
    vids = [(torch.from_numpy(r).to(DEV), torch.from_numpy(f).to(DEV)) for r, f in VT._videos()]
    fresh = pool.open()
    used = pool.open()
    for t in range(40):
        pool.push([used], vids[0][0][t:t + 1].contiguous(), vids[0][1][t:t + 1].contiguous())
    pool.close(used)
    assert pool.open() == used
    for slot in (fresh, used):
        for t in range(5):
            pool.push([slot], vids[1][0][t:t + 1].contiguous(), vids[1][1][t:t + 1].contiguous())
    return pool, fresh, used


def test_an_image_is_canonical_and_rows_beyond_fill_are_zero():
    m = _vit("fp16")
    pool, fresh, used = _two_homes_of_one_stream(m)
    T, E = pool._T, pool._E
    (a0, b0), _, _ = _slot_ranges(pool, used)
    ring_used = pool._block[a0:b0].view(torch.float32).view(T, E)
    assert bool(ring_used[5:].ne(0).any()), "the slot's ring holds nothing stale: the test shows nothing"
    snap = pool.snapshot([used, fresh])
    assert torch.equal(snap.images[0], snap.images[1]), "the image depends on the slot's history"
    assert torch.equal(pool.snapshot([fresh]).images[0], snap.images[0])      # nor on the call it was taken in
    lay = SP.image_layout(pool.image_geometry())
    w = snap.words()[0]
    rows = w[SP.IMAGE_TAG_WORDS:SP.IMAGE_TAG_WORDS + T * E].view(T, E)
    assert bool(rows[:5].ne(0).any(dim=1).all()) and not bool(rows[5:].ne(0).any())
    assert torch.equal(rows[:5].view(torch.float32), ring_used[:5])
    end = SP.IMAGE_TAG_WORDS + lay["state_words"] + lay["rec_words"]
    assert not bool(w[end:].ne(0).any()) and w.numel() == lay["image_words"] and snap.images.data_ptr() % 256 == 0
    assert SP.image_fault(w[:SP.IMAGE_TAG_WORDS].tolist() + [0] * lay["state_words"] + w[SP.IMAGE_TAG_WORDS + lay["state_words"]:].tolist(),
                          pool.image_geometry()) == 0                         # the host rule accepts what the device writes
    rec = OnlineRecord.from_words(w[SP.IMAGE_TAG_WORDS + lay["state_words"]:end].tolist(), 2, pool._ncls, 32)
    assert rec.frames == 5 and rec.result()["pred"] == pool.events(fresh)["pred"]
    # the GRU pool: a slot that held another stream before gives the image of the fresh one
    e = TW._real_engine("bf16", 3)
    gp = StreamPool(e, capacity=4, window=2, max_events=8)
    s0, s1 = gp.open(), gp.open()
    gp.push([s1], TW._feat((1, 2048), 401), None)
    gp.close(s1)
    assert gp.open() == s1
    for s in (s0, s1):
        for t in range(3):
            gp.push([s], TW._feat((1, 2048), 410 + t), None)
    gs = gp.snapshot([s0, s1])
    assert torch.equal(gs.images[0], gs.images[1]) and gs.frames() == [3, 3]


def test_the_host_route_leaves_the_same_bytes_as_the_device_route(tmp_path):
    m = _vit("fp16")
    pool, fresh, used = _two_homes_of_one_stream(m)
    snap = pool.snapshot()                                                    # all open slots, ascending
    assert snap.n == 2
    host = snap.cpu()
    assert host.device.type == "cpu" and host.geometry == snap.geometry
    host.save(tmp_path / "pool.snap")
    back = PoolSnapshot.load(tmp_path / "pool.snap").to(DEV)
    assert torch.equal(back.images, snap.images) and back.compute_dtype == "fp16"
    b1, b2 = (m.stream_pool(capacity=4, vote_window=2, max_events=32) for _ in range(2))
    b1.open(), b2.open()
    assert b1.restore(snap) == b2.restore(back) == [1, 2]
    torch.cuda.synchronize()
    assert torch.equal(b1._block, b2._block) and bool(b1._block.ne(0).any())
    for slot in (1, 2):
        for got, want in zip(_slot_bytes(b1, slot), _image_parts(b1, snap.images[slot - 1])):
            assert torch.equal(got, want)
    assert all(not bool(t.ne(0).any()) for slot in (0, 3) for t in _slot_bytes(b1, slot))      # nothing beside the slots named


# ---- f. refusals and the validity rule --------------------------------------------------------------------------------------------------------------
def _counts(dbg):
    a, w = C.c_int64(), C.c_int64()
    assert dbg.prego_debug_alloc_count(C.byref(a), C.byref(w)) == 0
    return a.value, w.value


def _voted_pool(e, capacity, streams, window=3, max_events=6):
    """a GRU pool whose slots hold real streams: one pushed frame each (a state row), then ids through vote; {slot: ids}"""
    pool = StreamPool(e, capacity=capacity, window=window, max_events=max_events)
    for _ in range(capacity):
        pool.open()
    slots = sorted(streams)
    pool.push(slots, TW._feat((len(slots), 2048), 500 + capacity), None, want_ant=False)
    for t in range(max(len(v) for v in streams.values())):
        now = [s for s in slots if len(streams[s]) > t]
        pool.vote(now, [streams[s][t] for s in now])
    return pool


def test_host_refusals_launch_nothing_and_write_nothing():
    dbg = _lib.load_debug()
    e = TW._real_engine("bf16", 8, lib=dbg)
    lib = dbg
    err = lambda: lib.prego_last_error().decode()
    pool = _voted_pool(e, 6, {1: [3, 3, 4, 5], 2: [1, 1, 1, 2, 2], 4: [7]})
    other = _voted_pool(e, 6, {0: [1]})
    feed, other_feed = pool.event_feed(max_out=16), other.event_feed(max_out=16)
    feed.drain().events()
    nb = lib.prego_stream_pool_image_bytes(pool.p)
    lay = SP.image_layout(pool.image_geometry())
    assert nb == 4 * lay["image_words"] and nb % 256 == 0 and lib.prego_stream_pool_image_bytes(None) == 0
    images = torch.full((3 * nb + 512,), 0x5A, dtype=torch.uint8, device=DEV)
    status = torch.full((8,), -77, dtype=torch.int32, device=DEV)
    assert images.data_ptr() % 256 == 0
    torch.cuda.synchronize()
    kept = [t.clone() for t in (pool._block, feed._block, images, status)]

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(t, k) for t, k in zip((pool._block, feed._block, images, status), kept))

    def snapshot(p=pool.p, f=None, n=3, slots=_arr(1, 2, 4), img=_p(images), nbytes=3 * nb):
        return lib.prego_stream_pool_snapshot(p, f, n, slots, img, nbytes, None)

    def restore(p=pool.p, f=None, n=3, slots=_arr(1, 2, 4), img=_p(images), nbytes=3 * nb, st=_p(status)):
        return lib.prego_stream_pool_restore(p, f, n, slots, img, nbytes, st, None)
    inside = C.c_void_p(pool._block.data_ptr() + 256)
    cases = [(dict(p=None), EINVAL, "pool is NULL"), (dict(n=0), EINVAL, "0 slots"), (dict(n=7, slots=_arr(*range(7))), EINVAL, "7 slots"),
             (dict(n=257, slots=_arr(*range(257))), EINVAL, "257 slots"), (dict(slots=None), EINVAL, "slots is NULL"),
             (dict(slots=_arr(1, 6, 4)), EINVAL, "slots[1] = 6 is outside the pool"), (dict(slots=_arr(-1, 2, 4)), EINVAL, "slots[0] = -1"),
             (dict(slots=_arr(1, 2, 1)), EINVAL, "slot 1 is named twice"), (dict(img=None), EINVAL, "images is NULL"),
             (dict(img=C.c_void_p(images.data_ptr() + 16)), EINVAL, "256-byte aligned"), (dict(nbytes=3 * nb - 1), EWORKSPACE, f"need {3 * nb}"),
             (dict(nbytes=0), EWORKSPACE, f"need {3 * nb}"), (dict(f=other_feed.f), EINVAL, "the feed belongs to another pool"),
             (dict(img=inside, nbytes=pool._block.numel()), EINVAL, "overlap the pool's block")]
    n0 = _counts(dbg)
    for call in (snapshot, restore):
        for kw, rc, msg in cases:
            assert call(**kw) == rc and msg in err(), (call.__name__, kw, err())
            assert untouched(), (call.__name__, kw)
    assert restore(st=C.c_void_p(images.data_ptr() + 4)) == EINVAL and "status overlaps" in err() and untouched()
    assert _counts(dbg) == n0
    # the Python surface refuses before it opens a slot or launches anything
    snap = pool.snapshot([1, 2, 4])
    torch.cuda.synchronize()
    kept = [t.clone() for t in (pool._block, feed._block, images, status)]
    free = other.free
    small = StreamPool(e, capacity=2, window=3, max_events=6)
    e16 = TW._real_engine("fp16", 3)
    for target, kw, msg in ((StreamPool(e, capacity=6, window=4, max_events=6), {}, "geometry"), (StreamPool(e, capacity=6, window=3, max_events=7), {}, "geometry"),
                            (StreamPool(e16, capacity=6, window=3, max_events=6), {}, "compute_dtype 'bf16'"), (small, {}, "3 streams, 2 free slots"),
                            (pool, {"feed": other_feed}, "feed belongs to another pool"), (pool, {"slots": [1, 2]}, "3 images, 2 slots"),
                            (other, {"slots": [1, 2, 2]}, "named twice")):
        free_t = target.free
        with pytest.raises(PregoError, match=msg):
            target.restore(snap, **kw)
        assert target.free == free_t
    vit_pool = _vit("fp16").stream_pool(capacity=2, vote_window=3, max_events=6)
    with pytest.raises(PregoError, match="pool kind 1"):
        vit_pool.restore(snap)
    with pytest.raises(PregoError, match="PoolSnapshot"):
        pool.restore(snap.images)
    other.close(3)
    for call, msg in ((lambda: other.snapshot([3]), "slot 3 is not open"), (lambda: other.detach([0, 0]), "named twice"),
                      (lambda: pool.snapshot([1], feed=other_feed), "feed belongs to another pool")):
        with pytest.raises(PregoError, match=msg):
            call()
    assert other.free == free + 1 and small.free == 2 and vit_pool.free == 2 and untouched()
    e.check()


GRU_BREAKS = [("magic", "tag", 0, 0x12345678, SP.FAULT_GEOMETRY), ("max_events", "tag", 7, 12, SP.FAULT_GEOMETRY),
              ("frames", "tag", SP.TAG_FRAMES, lambda v: v + 1, SP.FAULT_FRAMES), ("n_events", "rec", 2, 0x7fffffff, SP.FAULT_EVENTS),
              ("last vote", "rec", 1, NCLS + 1, SP.FAULT_VOTE), ("overflow", "rec", 3, 4, SP.FAULT_OVERFLOW),
              ("counter", "rec", SP.REC_HEADER + NCLS - 1, 4, SP.FAULT_COUNTER), ("first counter", "rec", SP.REC_HEADER, -1, SP.FAULT_COUNTER),
              ("cursor", "tag", SP.TAG_CURSOR, lambda v: v + 40, SP.FAULT_CURSOR)]


def _refusal_round(pool, feed, good, slots, breaks):
    """`good`: uint8 [3, image_bytes] valid images; for every break the middle image with one word broken goes to slots[1] of a call
    over `slots`: status carries the clause, slots[1] and its cursor keep their bytes, the neighbours take their images, the guards and
    every other byte of the pool's and the feed's block stay"""
    lib, nb = pool.lib, good.shape[1]
    lay = SP.image_layout(pool.image_geometry())
    r0 = SP.IMAGE_TAG_WORDS + lay["state_words"]
    restore = getattr(lib, pool._C["restore"])
    block0, fblock0 = pool._block.clone(), feed._block.clone()
    seen = 0
    for name, part, at, new, clause in breaks:
        buf = torch.full((3 * nb + 1024,), 0x5A, dtype=torch.uint8, device=DEV)
        assert buf.data_ptr() % 256 == 0
        buf[:3 * nb] = good.reshape(-1)
        words = buf[nb:2 * nb].view(torch.int32)
        k = at if part == "tag" else r0 + at
        old = int(words[k])
        value = new(old) if callable(new) else new
        assert value != old, name
        words[k] = value
        assert SP.image_fault(words[:SP.IMAGE_TAG_WORDS].tolist() + [0] * lay["state_words"] + words[r0:].tolist(),
                              pool.image_geometry()) & clause, name           # the host model names the clause as well
        sent = buf.clone()
        status = torch.full((3 + 5,), -77, dtype=torch.int32, device=DEV)
        pool._block.copy_(block0)
        feed._block.copy_(fblock0)
        assert restore(pool.p, feed.f, 3, _arr(*slots), _p(buf), 3 * nb, _p(status), None) == 0, name
        torch.cuda.synchronize()
        st = status.cpu().tolist()
        assert st[0] == 0 and st[2] == 0 and st[1] & clause and st[3:] == [-77] * 5, (name, st)
        assert st[1] == SP.image_fault(words[:SP.IMAGE_TAG_WORDS].tolist() + [0] * lay["state_words"] + words[r0:].tolist(), pool.image_geometry()), name
        assert torch.equal(buf, sent), f"{name}: restore wrote the images or their guard"
        want, fwant = block0.clone(), fblock0.clone()
        for i in (0, 2):
            for (a, b), bytes_ in zip(_slot_ranges(pool, slots[i]), _image_parts(pool, buf[i * nb:(i + 1) * nb])):
                want[a:b] = bytes_
            fwant[:4 * pool.capacity].view(torch.int32)[slots[i]] = buf[i * nb:(i + 1) * nb].view(torch.int32)[SP.TAG_CURSOR]
        assert torch.equal(pool._block, want), f"{name}: the refused slot, or a byte beside the restored ones, changed"
        assert torch.equal(feed._block, fwant), f"{name}: the refused slot's cursor, or a word beside the restored ones, changed"
        assert not torch.equal(want, block0) and not torch.equal(fwant, fblock0)            # the neighbours did change
        seen |= clause
    pool._block.copy_(block0)
    feed._block.copy_(fblock0)
    torch.cuda.synchronize()
    return seen


def test_a_broken_image_leaves_its_slot_untouched_and_names_its_clause_gru_pool():
    e = TW._real_engine("bf16", 3)
    src = _voted_pool(e, 8, {0: [3, 3, 3, 4, 4, 4, 5], 5: [1, 1, 2, 2, 2, 2, 6, 6], 6: [9, 9, 9, 8, 8, 8, 7, 7, 7, 6, 6]})
    src_feed = src.event_feed(max_out=32)
    src_feed.drain().events()
    src.vote([0, 5, 6], [1, 2, 3])                                            # one pushed frame, the ids above, this one: 9, 10 and 13 frames
    good = src.snapshot([0, 5, 6], feed=src_feed).images
    tags = good.view(torch.int32)[:, :SP.IMAGE_TAG_WORDS].cpu().tolist()
    assert [w[SP.TAG_FRAMES] for w in tags] == [9, 10, 13] and all(w[SP.TAG_CURSOR] >= 2 for w in tags)      # the middle one: mid window
    pool = _voted_pool(e, 8, {s: [10 + s] * (2 + s) + [20 + s] * 3 for s in range(8)})       # every slot pre-filled by a real stream
    feed = pool.event_feed(max_out=64)
    feed.drain().events()                                                     # every cursor stands at 1 or more
    torch.cuda.synchronize()
    assert int(feed._block[:32].view(torch.int32).min()) >= 1
    seen = _refusal_round(pool, feed, good, [6, 2, 3], GRU_BREAKS)
    assert seen == 255 - SP.FAULT_RING
    # pool.restore: raises, names image and clause, leaves no slot open that it opened and no byte behind
    for s in (1, 4, 7):
        pool.close(s)
    feed.drain().events()
    torch.cuda.synchronize()
    block0, free0 = pool._block.clone(), pool.free
    bad = good.clone()
    lay = SP.image_layout(pool.image_geometry())
    bad[1].view(torch.int32)[SP.IMAGE_TAG_WORDS + lay["state_words"] + SP.REC_HEADER] = 4      # a counter above the vote window
    with pytest.raises(PregoError, match=r"image 1 refused \(counter\)"):
        pool.restore(PoolSnapshot(bad, pool.image_geometry(), "bf16"), feed=feed)
    torch.cuda.synchronize()
    assert pool.free == free0 and torch.equal(pool._block, block0)
    assert feed._block[:32].view(torch.int32)[[1, 4, 7]].cpu().tolist() == [0, 0, 0]
    assert pool.restore(PoolSnapshot(good, pool.image_geometry(), "bf16"), feed=feed) == [1, 4, 7]      # the good ones go in afterwards
    assert [pool.events(s)["frames"] for s in (1, 4, 7)] == [9, 10, 13]
    e.check()


def test_a_broken_image_leaves_its_slot_untouched_and_names_its_clause_transformer_pool():
    m = _vit("fp16")
    T = VT.WINDOW
    vids = [(torch.from_numpy(r).to(DEV), torch.from_numpy(f).to(DEV)) for r, f in VT._videos()]
    src = m.stream_pool(capacity=4, vote_window=3, max_events=8)
    pool = m.stream_pool(capacity=4, vote_window=3, max_events=8)
    for p_ in (src, pool):
        for _ in range(4):
            p_.open()
    at = [0, 0, 0]
    for t in range(T + 3):                                                    # 35, 10 and 4 frames
        streams = [s for s, stop in enumerate((T + 3, 10, 4)) if t < stop]
        src.push(streams, *_vit_rows(vids, at, streams, [1] * len(streams)))
        for s in streams:
            at[s] += 1
    for t in range(6):                                                        # the target's slots hold streams of their own
        pool.push([0, 1, 2, 3], vids[2][0][t:t + 1].repeat(4, 1).contiguous(), vids[2][1][t:t + 1].repeat(4, 1).contiguous())
    src_feed, feed = src.event_feed(max_out=32), pool.event_feed(max_out=32)
    src_feed.drain().events()                                                 # the target's feed is not drained: its cursors stand at 0,
    good = src.snapshot([0, 1, 2], feed=src_feed).images                      # every image carries 1 or more
    assert int(good.view(torch.int32)[:, SP.TAG_CURSOR].min()) >= 1
    breaks = [("head", "tag", SP.TAG_HEAD, lambda v: (v + 1) % T, SP.FAULT_RING), ("fill", "tag", SP.TAG_FILL, lambda v: v + 1, SP.FAULT_RING),
              ("head outside the ring", "tag", SP.TAG_HEAD, T, SP.FAULT_RING), ("fill outside the ring", "tag", SP.TAG_FILL, 0x7fffffff, SP.FAULT_RING),
              ("window_size", "tag", 4, 2 * T, SP.FAULT_GEOMETRY), ("kind", "tag", 2, 1, SP.FAULT_GEOMETRY),
              ("n_events", "rec", 2, -5, SP.FAULT_EVENTS), ("frames", "rec", 0, lambda v: v + T, SP.FAULT_FRAMES)]
    assert _refusal_round(pool, feed, good, [3, 1, 0], breaks) & SP.FAULT_RING
    bad = good.clone()
    bad[2].view(torch.int32)[SP.TAG_HEAD] = 7
    free0 = pool.free
    pool.close(2)
    torch.cuda.synchronize()
    block0 = pool._block.clone()
    with pytest.raises(PregoError, match=r"image 0 refused \(ring head / fill\)"):
        pool.restore(PoolSnapshot(bad[2:3].clone(), pool.image_geometry(), "fp16"))
    with pytest.raises(PregoError, match="1 free slots"):
        pool.restore(PoolSnapshot(good, pool.image_geometry(), "fp16"))
    torch.cuda.synchronize()
    assert pool.free == free0 + 1 and torch.equal(pool._block, block0)


# ---- g. the feed ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_stream_moves_with_its_feed_position():
    e = TW._real_engine("bf16", 3)
    pool_a, pool_b, pool_c = (StreamPool(e, capacity=c, window=1, max_events=32) for c in (8, 16, 8))
    feed_a, feed_b, feed_c = pool_a.event_feed(max_out=64), pool_b.event_feed(max_out=64), pool_c.event_feed(max_out=64)
    rec_a = [OnlineRecord(1, NCLS, 32) for _ in range(8)]
    rec_b = [OnlineRecord(1, NCLS, 32) for _ in range(16)]
    model_a, model_b = FeedModel(rec_a, 64), FeedModel(rec_b, 64)
    for _ in range(4):
        pool_a.open()
    for _ in range(5):
        pool_b.open()
    streams = {1: [3, 4, 4, 5, 6, 7, 7, 8, 9], 3: [1, 1, 2, 3, 3, 4, 5, 6, 6], 2: [5, 5, 5, 5, 5, 5, 5, 5, 5]}

    def vote(pool, records, slot_of, t):
        slots = [slot_of[s] for s in streams]
        pool.vote(slots, [streams[s][t] for s in streams])
        for s in streams:
            records[slot_of[s]].push(streams[s][t])
    home_a = {s: s for s in streams}
    for t in range(3):
        vote(pool_a, rec_a, home_a, t)
    first = feed_a.drain().events()
    assert first == model_a.drain()["entries"] and len(first) >= 5
    for t in range(3, 5):                                                     # events nobody has heard yet travel in the images
        vote(pool_a, rec_a, home_a, t)
    snap = pool_a.detach([1, 3], feed=feed_a)
    words = [model_a.cursor_word(1), model_a.cursor_word(3)]
    assert snap.words()[:, SP.TAG_CURSOR].cpu().tolist() == words and min(words) >= 2
    assert pool_a.free == 6
    new = pool_b.restore(snap, feed=feed_b)
    assert new == [5, 6]
    for slot, old, word in zip(new, (1, 3), words):
        rec_b[slot] = OnlineRecord.from_words(rec_a[old].to_words(), 1, NCLS, 32)
        model_b.seek(slot, word)
        rec_a[old] = OnlineRecord(1, NCLS, 32)
    model_a.forget([1, 3])
    streams_b = {1: streams[1], 3: streams[3]}
    for t in range(5, 9):
        slots = [5, 6]
        pool_b.vote(slots, [streams_b[1][t], streams_b[3][t]])
        rec_b[5].push(streams_b[1][t])
        rec_b[6].push(streams_b[3][t])
    later = feed_b.drain().events()
    assert later == model_b.drain()["entries"]
    for old, slot in ((1, 5), (3, 6)):                                        # exactly the events after the first drain, with their true indices
        got = [(i, e_, s_) for sl, i, e_, s_ in first if sl == old] + [(i, e_, s_) for sl, i, e_, s_ in later if sl == slot]
        whole = list(zip(range(len(rec_b[slot].event_id)), rec_b[slot].event_id, rec_b[slot].event_start))
        assert got == whole and len(whole) >= 6, (old, got, whole)
        assert pool_b.events(slot)["pred"] == rec_b[slot].event_id
    assert feed_b.drain().events() == []
    # A: the slots are empty and its feed has forgotten them; the stream that stayed goes on
    pool_a.vote([2], [9])
    rec_a[2].push(9)
    assert feed_a.drain().events() == model_a.drain()["entries"] == [(2, 1, 9, 5)]
    assert pool_a.open() == 1 and pool_a.events(1) == {"pred": [], "changes_pred": [0], "frames": 0}
    # without feed=: an attached feed delivers the slot from index 0
    pool_c.open()
    new_c = pool_c.restore(snap)
    assert new_c == [1, 2]
    got_c = feed_c.drain().events()
    for k, slot in enumerate(new_c):
        frames = snap.frames()[k]
        ev = pool_c.events(slot)
        assert [(i, e_) for sl, i, e_, _ in got_c if sl == slot] == list(enumerate(ev["pred"])) and ev["frames"] == frames == 5
    assert len(got_c) >= 6
    e.check()


# ---- h. cleanliness -----------------------------------------------------------------------------------------------------------------------------------
def test_snapshot_and_restore_allocate_nothing_and_wait_for_nothing():
    dbg = _lib.load_debug()
    e = TW._real_engine("bf16", 8, lib=dbg)
    pool_a, pool_b = StreamPool(e, capacity=300, window=3), StreamPool(e, capacity=300, window=3)
    assert pool_a.lib is dbg
    slots = [pool_a.open() for _ in range(300)][::-1][:256]                   # the most a call takes, descending
    for a in range(0, 256, 64):
        pool_a.push(slots[a:a + 64], TW._feat((64, 2048), 600 + a), None, want_ant=False)
    feed_a, feed_b = pool_a.event_feed(max_out=16), pool_b.event_feed(max_out=16)
    nb = dbg.prego_stream_pool_image_bytes(pool_a.p)
    images = torch.empty(256 * nb, dtype=torch.uint8, device=DEV)
    status = torch.full((256,), -1, dtype=torch.int32, device=DEV)
    arr_a, arr_b = _arr(*slots), _arr(*range(256))
    torch.cuda.synchronize()
    n0 = _counts(dbg)
    assert dbg.prego_stream_pool_snapshot(pool_a.p, feed_a.f, 256, arr_a, _p(images), 256 * nb, None) == 0
    assert dbg.prego_stream_pool_restore(pool_b.p, feed_b.f, 256, arr_b, _p(images), 256 * nb, _p(status), None) == 0
    assert dbg.prego_stream_pool_restore(pool_b.p, None, 256, arr_b, _p(images), 256 * nb, None, None) == 0      # status and feed are nullable
    assert _counts(dbg) == n0                                                 # no device allocation and no host wait inside the calls
    torch.cuda.synchronize()
    assert not bool(status.ne(0).any())
    hid = pool_a._hid
    state = lambda p: p._block[:300 * hid * 4].view(torch.float32).view(300, hid)
    assert torch.equal(state(pool_b)[:256], state(pool_a)[slots]) and bool(state(pool_b)[:256].ne(0).any())
    assert not bool(state(pool_b)[256:].ne(0).any())
    for k in (0, 100, 255):
        assert torch.equal(_record_words(pool_b, k), _record_words(pool_a, slots[k]))
    e.check()                                                                 # no HIP error left behind
