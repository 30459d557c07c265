"""The stream pool's burst call (prego_miniroad_step_pool_frames, StreamPool.push_frames; csrc/stream_pool.hip: pool_commit_frames,
csrc/stream_frames.hip):
  1. exactly, against the saturated-gate automaton, with churn: streams opened at staggered ticks into scattered slots, each tick a seeded
     subset takes a burst of a seeded K in 1..8; outputs and slot state are compared after EVERY call, close() equals aggregate() of the
     reference ids with window 3, so window boundaries fall inside bursts;
  2. push_frames against K push calls on two pools with real weights: identical outputs, identical raw records;
  3. the window rule at the smallest shapes;  4. overflow inside a burst writes nothing past the record;
  5. refusals through raw ctypes, each with its message, nothing launched;  6. no allocation, no host wait."""
import ctypes as C
import random

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import _lib                                            # noqa: E402
from prego_amd._lib import PregoError                                 # noqa: E402
from prego_amd.aggregate import OnlineRecord, aggregate               # noqa: E402
from prego_amd.engine import MiniRoadEngine                           # noqa: E402
from prego_amd.stream_pool import StreamPool                          # noqa: E402
from tests import test_gpu_step_wide as TW                            # noqa: E402  its references and engines are computed once and shared

DEV = "cuda:0"
EINVAL = -1


def _agg(ids, window):
    a = aggregate({"v": {"pred": [int(i) for i in ids], "gt": [0] * len(ids)}}, window_size=window)["v"]
    return {"pred": a["pred"], "changes_pred": a["changes_pred"]}


# ---- 1. the automaton, with churn ---------------------------------------------------------------------------------------------------------
CHURN = [(cid, dt, ant) for cid in ("L1-C12", "L4-C12") for dt in ("bf16", "fp16") for ant in (True, False)]


def _schedule(n, T, seed):
    """[(streams opened at this tick, streams that take a burst at this tick in call order, K)]: every stream of a call takes the same K
    frames, K in 1..8 drawn per tick and cut to what the chosen streams all still have and to n K <= 256"""
    rng = random.Random(seed)
    order = list(range(n))
    rng.shuffle(order)
    open_at = [order[:4], order[4:12], order[12:]]
    left, live, ticks = [T] * n, [], []
    while True:
        t = len(ticks)
        opened = open_at[t] if t < 3 else []
        live += opened
        can = [s for s in live if left[s] > 0]
        if not can:
            break
        act = rng.sample(can, rng.randint(1, len(can)))
        K = min([rng.randint(1, 8)] + [left[s] for s in act] + [256 // len(act)])
        for s in act:
            left[s] -= K
        ticks.append((opened, act, K))
    assert all(v == 0 for v in left)
    return ticks


@pytest.mark.parametrize("cid,dtype,ant", CHURN, ids=[f"{c}-{d}-{'ant' if a else 'trunk'}" for c, d, a in CHURN])
def test_push_frames_equals_the_automaton_with_churn(cid, dtype, ant):
    case, sd, n, T, x, res = TW._ref(cid)
    L, Cn, window = case.ant_len, case.n_classes, 3
    e = MiniRoadEngine(case.d_rgb, case.d_flow, case.emb, case.hid, Cn, DEV, dtype)
    e.set_weights(sd)
    if ant:
        e.set_anticipation(sd[TW.A_KEYS[0]], sd[TW.A_KEYS[1]], L)
    want_l, want_a, want_h = (t.view(n, T, -1) for t in (res.logits, res.argmax, res.h[0]))
    want_al, want_aa = res.ant_logits.view(n, T, L, Cn), res.ant_argmax.view(n, T, L)
    pool = StreamPool(e, capacity=64, window=window, max_events=8)
    rng = random.Random(7)
    for _ in range(64):
        pool.open()
    holes = rng.sample(range(64), n)
    for s in holes:
        assert pool.close(s) == {"pred": [], "changes_pred": [0]}
    slot_of, frame, Ks = {}, [0] * n, set()
    for opened, act, K in _schedule(n, T, 11):
        for s in opened:
            slot_of[s] = pool.open()
        slots = [slot_of[s] for s in act]
        rgb = torch.stack([x[s, frame[s]:frame[s] + K] for s in act])
        got = pool.push_frames(slots, rgb, None, softmax=False)
        assert len(got) == (4 if ant else 2)
        Ks.add(K)
        si = torch.tensor(act, device=DEV)[:, None]
        fi = torch.tensor([frame[s] for s in act], device=DEV)[:, None] + torch.arange(K, device=DEV)[None, :]
        assert got[0].shape == (len(act), K, Cn) and torch.equal(got[0].to(torch.float64), want_l[si, fi]), "logits"
        assert got[1].dtype == torch.int32 and torch.equal(got[1], want_a[si, fi, 0]), "argmax"
        assert torch.equal(torch.stack([pool.state(s) for s in slots]), want_h[si[:, 0], fi[:, -1]].to(torch.float32)), "state"
        if ant:
            assert torch.equal(got[2].to(torch.float64), want_al[si, fi]), "anticipation logits"
            assert torch.equal(got[3], want_aa[si, fi]), "anticipation argmax"
        for s in act:
            frame[s] += K
    assert frame == [T] * n and len(Ks) >= 4 and any(K % window for K in Ks) and max(Ks) > window
    assert sorted(slot_of.values()) == sorted(holes)
    ids = want_a[:, :, 0].cpu().tolist()
    for s in range(n):
        assert pool.close(slot_of[s]) == _agg(ids[s], window), f"stream {s}"
    e.check()


# ---- 2. push_frames against K push calls ----------------------------------------------------------------------------------------------------
def _raw_record(pool, slot):
    ptr, nb = C.c_void_p(), C.c_size_t()
    assert pool.lib.prego_stream_pool_record(pool.p, slot, C.byref(ptr), C.byref(nb)) == 0
    off = ptr.value - pool._block.data_ptr()
    return pool._block[off:off + nb.value].view(torch.int32).cpu().tolist()


BITS = [(dt, n, K, sm, ant) for dt in ("bf16", "fp16") for (n, K) in ((5, 4), (37, 6)) for sm in (True, False) for ant in (True, False)]


@pytest.mark.parametrize("dtype,n,K,softmax,ant", BITS,
                         ids=[f"{d}-n{n}-K{K}-{'probs' if s else 'logits'}-{'ant' if a else 'trunk'}" for d, n, K, s, a in BITS])
def test_push_frames_equals_k_pushes_on_real_weights(dtype, n, K, softmax, ant):
    e = TW._real_engine(dtype, 3)
    window = 4                                                # K = 4: a multiple; K = 6: boundaries wander through the bursts
    burst, single = StreamPool(e, capacity=64, window=window, max_events=16), StreamPool(e, capacity=200, window=window, max_events=16)
    rng = random.Random(n)
    taken = []
    for pool, cap in ((burst, 64), (single, 200)):
        for _ in range(cap):
            pool.open()
        keep = rng.sample(range(cap), n)
        for s in set(range(cap)) - set(keep):
            pool.close(s)
        taken.append(keep)
    assert taken[0] != taken[1]
    for b in range(2):
        # the streams' features differ in scale, so that their ids do: the records have something to tell apart
        scale = torch.arange(1, n + 1, device=DEV)[:, None, None].to(torch.float32)
        rgb, flow = TW._feat((n, K, 2048), 110 + b) * scale, TW._feat((n, K, 2048), 120 + b)
        got = burst.push_frames(taken[0], rgb, flow, softmax=softmax, want_ant=ant)
        want = [torch.stack(ts, dim=1) for ts in zip(*[single.push(taken[1], rgb[:, t].contiguous(), flow[:, t].contiguous(), softmax=softmax,
                                                                   want_ant=ant) for t in range(K)])]
        assert len(got) == len(want) == (4 if ant else 2)
        for name, g, w in zip(("out", "argmax", "ant_out", "ant_argmax"), got, want):
            assert g.shape == w.shape and torch.equal(g, w), f"burst {b}: {name}"
        for sb, ss in zip(*taken):
            assert torch.equal(burst.state(sb), single.state(ss)), f"burst {b}: state"
            rb, rs = _raw_record(burst, sb), _raw_record(single, ss)
            assert rb == rs and rb[0] == (b + 1) * K, f"burst {b}: record"
    e.check()


# ---- 3. the window rule at the smallest shapes ----------------------------------------------------------------------------------------------
def _push_ids(e, pool, slots, K, seed):
    """one push_frames of K frames; returns the ids it voted, per slot"""
    n = len(slots)
    rgb = TW._feat((n, K, 2048), seed) * torch.arange(1, n * K + 1, device=DEV).view(n, K, 1).to(torch.float32)
    return pool.push_frames(slots, rgb, None, want_ant=False)[1].cpu().tolist()


@pytest.mark.parametrize("window,bursts", [(1, (1, 3, 2)), (2, (4, 2, 6)), (3, (2, 5, 1, 4)), (3, (8,)), (4, (32, 3))],
                         ids=["w1", "w2-multiples", "w3-not-multiples", "w3-two-windows-and-a-third", "w4-K32"])
def test_window_rule_inside_bursts(window, bursts):
    e = TW._real_engine("bf16", 3)
    pool = StreamPool(e, capacity=8, window=window, max_events=64)
    slots = [pool.open() for _ in range(3)][::-1]
    ids, model = {s: [] for s in slots}, {s: OnlineRecord(window, 86, 64) for s in slots}
    for b, K in enumerate(bursts):
        for s, row in zip(slots, _push_ids(e, pool, slots, K, 500 + b)):
            ids[s] += row
            model[s].push_frames(row)
        for s in slots:                                       # midway: the finished windows only, as the host model has them
            assert pool.events(s) == model[s].result(), (s, b)
    for s in slots:
        assert len(ids[s]) == sum(bursts)
        assert pool.close(s) == _agg(ids[s], window), s
    e.check()


# ---- 4. overflow inside a burst ------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _slots(*s):
    return (C.c_int32 * len(s))(*s)


def _raw_pool(e, capacity, window, max_events, tail=4096):
    need = e.lib.prego_stream_pool_bytes(e.h, capacity, max_events)
    assert need > 0
    block = torch.full((need + tail,), 0xA5, dtype=torch.uint8, device=DEV)
    assert block.data_ptr() % 256 == 0
    p = C.c_void_p()
    assert e.lib.prego_stream_pool_create(C.byref(p), e.h, capacity, window, max_events, _p(block), need, None) == 0
    return p, block, need


def _rec(e, p, block, slot):
    ptr, nb = C.c_void_p(), C.c_size_t()
    assert e.lib.prego_stream_pool_record(p, slot, C.byref(ptr), C.byref(nb)) == 0
    off = ptr.value - block.data_ptr()
    return block[off:off + nb.value].view(torch.int32).cpu().tolist()


def test_overflow_inside_a_burst_drops_events_and_writes_nothing_past_the_record():
    e = TW._real_engine("bf16", 3)
    lib = e.lib
    K, me, cpad = 24, 2, 88
    p, block, need = _raw_pool(e, 3, 1, me)                   # window 1: every change of id inside the burst is an event
    rgb = TW._feat((2, K, 2048), 600) * torch.arange(1, 2 * K + 1, device=DEV).view(2, K, 1).to(torch.float32)
    am = torch.full((2, K), -7, dtype=torch.int32, device=DEV)
    ws_need = lib.prego_miniroad_step_pool_frames_workspace_bytes(e.h, 2, K)
    ws = torch.empty((ws_need,), dtype=torch.uint8, device=DEV)
    assert lib.prego_miniroad_step_pool_frames(e.h, p, 2, K, _slots(1, 2), _p(rgb), None, None, _p(am), None, None, 1, _p(ws), ws_need, None) == 0
    torch.cuda.synchronize()
    ids = am.cpu().tolist()
    r0, r1, r2 = (_rec(e, p, block, s) for s in range(3))
    for r, row in ((r1, ids[0]), (r2, ids[1])):
        m = OnlineRecord(1, 86, me)
        m.push_frames(row)
        assert len(r) == 4 + cpad + 2 * me
        assert r[:4] == [K, m.last_vote + 1, len(m.event_id), m.overflow] and r[4:4 + cpad] == [0] * cpad
        assert r[4 + cpad:4 + cpad + me] == m.event_id + [0] * (me - len(m.event_id))
        assert r[4 + cpad + me:] == m.event_start + [0] * (me - len(m.event_start))
    changes = [sum(1 for a, b in zip(row, row[1:]) if a != b) for row in ids]
    assert max(changes) >= me, f"the burst's ids change {changes} times: no overflow to test"
    assert (r1[3] | r2[3]) & 1, "bit 0: the record is full"
    assert r0 == [0] * len(r0)                                # the neighbouring record
    assert bool((block[need:] == 0xA5).all()), "written past prego_stream_pool_bytes"
    lib.prego_stream_pool_destroy(p)
    # the Python surface: close raises and frees the slot all the same
    pool = StreamPool(e, capacity=4, window=1, max_events=me)
    s, nb = pool.open(), pool.open()
    got = pool.push_frames([s, nb], rgb, None, want_ant=False)[1].cpu().tolist()
    assert got == ids
    over = [sum(1 for a, b in zip(row, row[1:]) if a != b) >= me for row in ids]
    for slot, o, row in zip((s, nb), over, ids):
        if o:
            with pytest.raises(PregoError, match=f"max_events = {me}"):
                pool.close(slot)
        else:
            assert pool.close(slot) == _agg(row, 1)
    assert pool.free == 4
    e.check()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi():
    e = TW._real_engine("bf16", 3)
    lib = e.lib
    err = lambda: lib.prego_last_error().decode()
    cap, n, K = 8, 3, 4
    p, block, need = _raw_pool(e, cap, 200, 16)
    torch.cuda.synchronize()
    ws_need = lib.prego_miniroad_step_pool_frames_workspace_bytes(e.h, n, K)
    assert ws_need > lib.prego_miniroad_step_frames_workspace_bytes(e.h, n, K) > 0
    for a, b in ((0, 1), (1, 0), (1, 33), (257, 1), (129, 2)):
        assert lib.prego_miniroad_step_pool_frames_workspace_bytes(e.h, a, b) == 0
    rgb = TW._feat((8, K, 2048), 400)
    ws = torch.full((lib.prego_miniroad_step_pool_frames_workspace_bytes(e.h, 8, K) + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    out, am = torch.full((8, K, 86), float("nan"), device=DEV), torch.full((8, K), -7, dtype=torch.int32, device=DEV)
    ao, aa = torch.full((8, K, 3, 86), float("nan"), device=DEV), torch.full((8, K, 3), -7, dtype=torch.int32, device=DEV)
    assert lib.prego_miniroad_step_pool_frames(e.h, p, n, K, _slots(5, 0, 2), _p(rgb), None, _p(out), _p(am), None, None, 1, _p(ws), ws_need, None) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[:n]).any()) and bool(torch.isnan(out[n:]).all())
    assert [_rec(e, p, block, s)[0] for s in range(cap)] == [K, 0, K, 0, 0, K, 0, 0]
    out.fill_(float("nan"))
    am.fill_(-7)
    snap, ws_snap = block.clone(), ws.clone()

    def step(handle=None, pool=p, n_active=n, n_frames=K, slots=(5, 0, 2), w=ws, w_off=0, w_bytes=None, ant=False, eng=e):
        return eng.lib.prego_miniroad_step_pool_frames((handle or eng).h if handle is not False else None, pool, n_active, n_frames,
                                                       _slots(*slots) if slots is not None else None, _p(rgb), None, _p(out), _p(am),
                                                       _p(ao) if ant else None, _p(aa) if ant else None, 1,
                                                       None if w is None else C.c_void_p(w.data_ptr() + w_off),
                                                       ws_need if w_bytes is None else w_bytes, None)

    def untouched(blk=None, sn=None):
        torch.cuda.synchronize()
        blk, sn = (block, snap) if blk is None else (blk, sn)
        return (torch.equal(blk, sn) and torch.equal(ws, ws_snap) and bool(torch.isnan(out).all()) and bool((am == -7).all())
                and bool(torch.isnan(ao).all()) and bool((aa == -7).all()))

    cases = [(dict(n_frames=0), "0 frames per stream (1..32 per call)"),
             (dict(n_frames=33), "33 frames per stream (1..32 per call)"),
             (dict(n_active=129, n_frames=2, slots=tuple(range(8))), "= 258 rows (at most 256 per call"),
             (dict(n_active=257, n_frames=1, slots=tuple(range(8))), "= 257 rows (at most 256 per call"),
             (dict(n_active=0, slots=(5,)), "0 streams (1..256 per call)"),
             (dict(n_active=9, n_frames=1, slots=tuple(range(8)) + (0,)), "9 slots (1..8 per call"),
             (dict(slots=(5, 8, 2)), "slots[1] = 8 is outside the pool (capacity 8)"),
             (dict(slots=(-1, 0, 2)), "slots[0] = -1 is outside the pool"),
             (dict(slots=(5, 0, 5)), "slot 5 is named twice"),
             (dict(slots=None), "slots is NULL"),
             (dict(pool=None), "pool is NULL"),
             (dict(w=None), "workspace"),
             (dict(w_off=16), "256-byte aligned"),
             (dict(w_bytes=ws_need - 1), f"need {ws_need}")]
    for kw, msg in cases:
        assert step(**kw) == EINVAL and msg in err(), (kw, err())
        assert untouched(), kw
    assert step() == 0                                                      # the pool and the handle survive
    torch.cuda.synchronize()
    assert not torch.equal(block, snap)
    out.fill_(float("nan"))
    am.fill_(-7)
    snap, ws_snap = block.clone(), ws.clone()
    # a pool of another shape
    e12 = MiniRoadEngine(2048, 2048, 2048, 1024, 12, DEV, "bf16")
    p12, block12, _ = _raw_pool(e12, cap, 200, 16)
    torch.cuda.synchronize()
    snap12 = block12.clone()
    assert step(pool=p12) == EINVAL and "created for hidden_dim 1024 / 12 classes" in err() and untouched(block12, snap12) and untouched()
    # everything the dense call refuses
    assert step(handle=False) == EINVAL and "handle is NULL" in err() and untouched()
    trunk = TW._real_engine("bf16", 3, ant=False)
    assert step(handle=trunk, ant=True) == EINVAL and "before set_anticipation" in err() and untouched()
    for eng, msg in ((TW._real_engine("fp32", 3), "bf16 / fp16 handles"), (TW._real_engine("bf16", 3, hid=512), "hidden_dim 1024")):
        pe, be, _ = _raw_pool(eng, cap, 200, 16)
        torch.cuda.synchronize()
        sn = be.clone()
        assert step(handle=eng, pool=pe) == EINVAL and msg in err() and untouched(be, sn) and untouched(), msg
        with pytest.raises(PregoError, match="the streaming kernels are built for"):
            sp = StreamPool(eng, capacity=4)
            sp.push_frames([sp.open()], rgb[:1], None)
        eng.lib.prego_stream_pool_destroy(pe)
    # the Python surface: a slot that is not open, a slot named twice
    pool = StreamPool(e, capacity=4)
    a = pool.open()
    with pytest.raises(PregoError, match="slot 1 is not open"):
        pool.push_frames([a, 1], rgb[:2], None)
    with pytest.raises(PregoError, match="named twice"):
        pool.push_frames([a, a], rgb[:2], None)
    with pytest.raises(PregoError, match="expected frames as"):
        pool.push_frames([a], rgb[:2], None)
    with pytest.raises(PregoError, match="33 frames"):
        pool.push_frames([a], TW._feat((1, 33, 2048), 5), None)
    assert pool.events(a)["frames"] == 0
    lib.prego_stream_pool_destroy(p)
    lib.prego_stream_pool_destroy(p12)
    e.check()


# ---- 6. no allocation, no host wait -------------------------------------------------------------------------------------------------------------
def test_push_frames_allocates_nothing_and_waits_for_nothing():
    dbg = _lib.load_debug()
    e = TW._real_engine("bf16", 8, lib=dbg)
    pool = StreamPool(e, capacity=256)
    assert pool.lib is dbg
    n, K = 16, 8
    slots = [pool.open() for _ in range(256)][::-1][:n]
    rgb = TW._feat((n, K, 2048), 8)
    bufs = pool.push_frames(slots, rgb, None)
    e.check()

    def counts():
        a, w = C.c_int64(), C.c_int64()
        assert dbg.prego_debug_alloc_count(C.byref(a), C.byref(w)) == 0
        return a.value, w.value
    n0 = counts()
    pool.push_frames(slots, rgb, None, out=bufs[0], argmax=bufs[1], ant_out=bufs[2], ant_argmax=bufs[3])
    assert counts() == n0                                    # no device allocation and no host wait inside the call
    e.check()
    assert pool.events(slots[0])["frames"] == 2 * K
