"""The stream pool's ragged burst (prego_miniroad_step_pool_ragged, StreamPool.push_ragged; csrc/stream_pool.hip: pool_commit_ragged,
csrc/stream_frames.hip):
  1. push_ragged against per-slot push calls on a twin pool with real weights: identical outputs, identical raw records, scattered slots,
     window 3, so that a window boundary falls inside some streams' bursts and not inside others';
  2. exactly, against the saturated-gate automaton, with churn: a seeded ragged schedule, outputs and slot state compared after EVERY call,
     close() equals aggregate() of the reference ids;
  3. max_events overflow inside a burst writes nothing past the record;
  4. a refused call leaves block and records untouched, through raw ctypes and through the Python surface;
  5. no allocation, no host wait."""
import ctypes as C
import random

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import _lib                                            # noqa: E402
from prego_amd._lib import PregoError                                 # noqa: E402
from prego_amd.aggregate import OnlineRecord, aggregate               # noqa: E402
from prego_amd.engine import MiniRoadEngine                           # noqa: E402
from prego_amd.stream_pool import StreamPool, pack_bursts, unpack_bursts      # noqa: E402
from tests import test_gpu_step_wide as TW                            # noqa: E402  its references and engines are computed once and shared
from tests.helpers import step_ragged_cases as SR                     # noqa: E402

DEV = "cuda:0"
EINVAL = -1


def _agg(ids, window):
    a = aggregate({"v": {"pred": [int(i) for i in ids], "gt": [0] * len(ids)}}, window_size=window)["v"]
    return {"pred": a["pred"], "changes_pred": a["changes_pred"]}


def _raw_record(pool, slot):
    ptr, nb = C.c_void_p(), C.c_size_t()
    assert pool.lib.prego_stream_pool_record(pool.p, slot, C.byref(ptr), C.byref(nb)) == 0
    off = ptr.value - pool._block.data_ptr()
    return pool._block[off:off + nb.value].view(torch.int32).cpu().tolist()


# ---- 1. push_ragged against per-slot push calls -----------------------------------------------------------------------------------------------
BITS = [(dt, n, sm, ant) for dt in ("bf16", "fp16") for n in (5, 37) for sm in (True, False) for ant in (True, False)]


@pytest.mark.parametrize("dtype,n,softmax,ant", BITS, ids=[f"{d}-n{n}-{'probs' if s else 'logits'}-{'ant' if a else 'trunk'}" for d, n, s, a in BITS])
def test_push_ragged_equals_per_slot_pushes_on_real_weights(dtype, n, softmax, ant):
    e = TW._real_engine(dtype, 3)
    window = 3
    ragged, single = StreamPool(e, capacity=64, window=window, max_events=16), StreamPool(e, capacity=200, window=window, max_events=16)
    rng = random.Random(n)
    taken = []
    for pool, cap, extra in ((ragged, 64, 0), (single, 200, 4)):
        for _ in range(cap):
            pool.open()
        keep = rng.sample(range(cap), n + extra)
        for s in set(range(cap)) - set(keep):
            pool.close(s)
        taken.append(keep)
    # four filler slots ride along in every `push`: a call of 5..256 streams, the route whose bits a burst has (<= 4 streams: step's fused
    # LayerNorm, other bits)
    taken[1], fillers = taken[1][:n], taken[1][n:]
    assert taken[0] != taken[1] and len(fillers) == 4
    fill_r, fill_f = TW._feat((4, 2048), 90), TW._feat((4, 2048), 91)
    total = [0] * n
    for b in range(2):
        counts = (3, 1, 5, 1, 2) if (n, b) == (5, 0) else SR.seeded_counts(n, 1, 6, 10 * n + b)
        inside = [(total[i] % window) + k > window for i, k in enumerate(counts)]
        assert any(inside) and not all(inside)                # a window boundary inside some bursts, not inside others
        # the streams' features differ in scale, so that their ids do: the records have something to tell apart
        bursts_r = [TW._feat((k, 2048), 1000 * b + i) * float(i + 1) for i, k in enumerate(counts)]
        bursts_f = [TW._feat((k, 2048), 1000 * b + 500 + i) for i, k in enumerate(counts)]
        rgb, flow = pack_bursts(bursts_r)[0], pack_bursts(bursts_f)[0]
        got = ragged.push_ragged(taken[0], counts, rgb, flow, softmax=softmax, want_ant=ant)
        assert len(got) == (4 if ant else 2)
        got = [unpack_bursts(t, counts) for t in got]
        for t in range(max(counts)):                          # frame by frame: one `push` of the slots that have a frame t
            live = [i for i, k in enumerate(counts) if k > t]
            w = single.push([taken[1][i] for i in live] + fillers, torch.cat([torch.stack([bursts_r[i][t] for i in live]), fill_r]),
                            torch.cat([torch.stack([bursts_f[i][t] for i in live]), fill_f]), softmax=softmax, want_ant=ant)
            for name, g, x in zip(("out", "argmax", "ant_out", "ant_argmax"), got, w):
                assert all(torch.equal(g[i][t], x[j]) for j, i in enumerate(live)), f"burst {b}, frame {t}: {name}"
        for i, (sr, ss) in enumerate(zip(*taken)):
            total[i] += counts[i]
            assert torch.equal(ragged.state(sr), single.state(ss)), f"burst {b}: state"
            rr, rs = _raw_record(ragged, sr), _raw_record(single, ss)
            assert rr == rs and rr[0] == total[i], f"burst {b}: record"
    e.check()


# ---- 2. the automaton, with churn ---------------------------------------------------------------------------------------------------------
CHURN = [(cid, dt, ant) for cid in ("L1-C12", "L4-C12") for dt in ("bf16", "fp16") for ant in (True, False)]


@pytest.mark.parametrize("cid,dtype,ant", CHURN, ids=[f"{c}-{d}-{'ant' if a else 'trunk'}" for c, d, a in CHURN])
def test_push_ragged_equals_the_automaton_with_churn(cid, dtype, ant):
    case, sd, n, T, x, res = TW._ref(cid)
    L, Cn, window = case.ant_len, case.n_classes, 3
    e = MiniRoadEngine(case.d_rgb, case.d_flow, case.emb, case.hid, Cn, DEV, dtype)
    e.set_weights(sd)
    if ant:
        e.set_anticipation(sd[TW.A_KEYS[0]], sd[TW.A_KEYS[1]], L)
    pool = StreamPool(e, capacity=64, window=window, max_events=8)
    rng = random.Random(7)
    for _ in range(64):
        pool.open()
    holes = rng.sample(range(64), n)
    for s in holes:
        assert pool.close(s) == {"pred": [], "changes_pred": [0]}
    slot_of, frame, seen = {}, [0] * n, set()
    for act, counts in SR.ragged_schedule(n, T, 11):
        for s in act:
            if s not in slot_of:                              # a stream opens when it first has frames
                slot_of[s] = pool.open()
        slots = [slot_of[s] for s in act]
        rgb = pack_bursts([x[s, frame[s]:frame[s] + k] for s, k in zip(act, counts)])[0]
        got = pool.push_ragged(slots, counts, rgb, None, softmax=False)
        assert len(got) == (4 if ant else 2)
        seen.update(counts)
        rows, last = SR.reference_rows(res.offs, act, [frame[s] for s in act], counts)
        rows, last = torch.tensor(rows, device=DEV), torch.tensor(last, device=DEV)
        assert got[0].shape == (sum(counts), Cn) and torch.equal(got[0].to(torch.float64), res.logits[rows]), "logits"
        assert got[1].dtype == torch.int32 and torch.equal(got[1], res.argmax[rows].view(-1)), "argmax"
        assert torch.equal(torch.stack([pool.state(s) for s in slots]), res.h[0][last].to(torch.float32)), "state"
        if ant:
            assert torch.equal(got[2].to(torch.float64), res.ant_logits[rows]), "anticipation logits"
            assert torch.equal(got[3], res.ant_argmax[rows]), "anticipation argmax"
        for s, k in zip(act, counts):
            frame[s] += k
    assert frame == [T] * n and len(seen) >= 4 and max(seen) > window
    assert sorted(slot_of.values()) == sorted(holes)
    ids = res.argmax.view(n, T).cpu().tolist()
    for s in range(n):
        assert pool.close(slot_of[s]) == _agg(ids[s], window), f"stream {s}"
    e.check()


# ---- 3. overflow inside a burst ------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _ints(*s):
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
    counts, me, cpad = (24, 2, 17), 2, 88
    R = sum(counts)
    p, block, need = _raw_pool(e, 4, 1, me)                   # window 1: every change of id inside the burst is an event
    rgb = TW._feat((R, 2048), 600) * torch.arange(1, R + 1, device=DEV).view(R, 1).to(torch.float32)
    am = torch.full((R,), -7, dtype=torch.int32, device=DEV)
    ws_need = lib.prego_miniroad_step_pool_ragged_workspace_bytes(e.h, 3, R)
    ws = torch.empty((ws_need,), dtype=torch.uint8, device=DEV)
    assert lib.prego_miniroad_step_pool_ragged(e.h, p, 3, _ints(*counts), _ints(1, 3, 2), _p(rgb), None, None, _p(am), None, None, 1, _p(ws),
                                               ws_need, None) == 0
    torch.cuda.synchronize()
    ids = [t.tolist() for t in torch.split(am.cpu(), list(counts))]
    recs = [_rec(e, p, block, s) for s in range(4)]
    for slot, row in zip((1, 3, 2), ids):
        r, m = recs[slot], OnlineRecord(1, 86, me)
        m.push_frames(row)
        assert len(r) == 4 + cpad + 2 * me
        assert r[:4] == [len(row), m.last_vote + 1, len(m.event_id), m.overflow] and r[4:4 + cpad] == [0] * cpad
        assert r[4 + cpad:4 + cpad + me] == m.event_id + [0] * (me - len(m.event_id))
        assert r[4 + cpad + me:] == m.event_start + [0] * (me - len(m.event_start))
    changes = [sum(1 for a, b in zip(row, row[1:]) if a != b) for row in ids]
    assert max(changes) >= me, f"the bursts' ids change {changes} times: no overflow to test"
    assert (recs[1][3] | recs[2][3] | recs[3][3]) & 1, "bit 0: the record is full"
    assert recs[0] == [0] * len(recs[0])                      # the neighbouring record
    assert bool((block[need:] == 0xA5).all()), "written past prego_stream_pool_bytes"
    lib.prego_stream_pool_destroy(p)
    # the Python surface: close raises and frees the slot all the same
    pool = StreamPool(e, capacity=4, window=1, max_events=me)
    slots = [pool.open() for _ in range(3)]
    got = [t.tolist() for t in unpack_bursts(pool.push_ragged(slots, counts, rgb, None, want_ant=False)[1].cpu(), counts)]
    assert got == ids
    for slot, row in zip(slots, ids):
        if sum(1 for a, b in zip(row, row[1:]) if a != b) >= me:
            with pytest.raises(PregoError, match=f"max_events = {me}"):
                pool.close(slot)
        else:
            assert pool.close(slot) == _agg(row, 1)
    assert pool.free == 4
    e.check()


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_leaves_block_and_records_untouched():
    e = TW._real_engine("bf16", 3)
    lib = e.lib
    err = lambda: lib.prego_last_error().decode()
    cap, n, counts = 8, 3, (4, 1, 2)
    R = sum(counts)
    p, block, need = _raw_pool(e, cap, 200, 16)
    torch.cuda.synchronize()
    q = lib.prego_miniroad_step_pool_ragged_workspace_bytes
    ws_need = q(e.h, n, R)
    assert ws_need > lib.prego_miniroad_step_ragged_workspace_bytes(e.h, n, R) > 0
    assert q(e.h, 3, 12) == lib.prego_miniroad_step_pool_frames_workspace_bytes(e.h, 3, 4)      # all counts equal: push_frames' size
    for a, b in ((0, 1), (1, 0), (3, 2), (257, 257), (2, 257)):
        assert q(e.h, a, b) == 0
    rgb = TW._feat((256, 2048), 400)
    ws = torch.full((q(e.h, 8, 256) + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    out, am = torch.full((256, 86), float("nan"), device=DEV), torch.full((256,), -7, dtype=torch.int32, device=DEV)
    ao, aa = torch.full((256, 3, 86), float("nan"), device=DEV), torch.full((256, 3), -7, dtype=torch.int32, device=DEV)
    assert lib.prego_miniroad_step_pool_ragged(e.h, p, n, _ints(*counts), _ints(5, 0, 2), _p(rgb), None, _p(out), _p(am), None, None, 1, _p(ws),
                                               ws_need, None) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[:R]).any()) and bool(torch.isnan(out[R:]).all())
    assert [_rec(e, p, block, s)[0] for s in range(cap)] == [1, 0, 2, 0, 0, 4, 0, 0]
    out.fill_(float("nan"))
    am.fill_(-7)
    snap, ws_snap = block.clone(), ws.clone()

    def step(handle=None, pool=p, n_active=n, n_frames=counts, slots=(5, 0, 2), w=ws, w_off=0, w_bytes=None, ant=False, eng=e):
        return eng.lib.prego_miniroad_step_pool_ragged((handle or eng).h if handle is not False else None, pool, n_active,
                                                       _ints(*n_frames) if n_frames is not None else None,
                                                       _ints(*slots) if slots is not None else None, _p(rgb), None, _p(out), _p(am),
                                                       _p(ao) if ant else None, _p(aa) if ant else None, 1,
                                                       None if w is None else C.c_void_p(w.data_ptr() + w_off),
                                                       ws_need if w_bytes is None else w_bytes, None)

    def untouched(blk=None, sn=None):
        torch.cuda.synchronize()
        blk, sn = (block, snap) if blk is None else (blk, sn)
        return (torch.equal(blk, sn) and torch.equal(ws, ws_snap) and bool(torch.isnan(out).all()) and bool((am == -7).all())
                and bool(torch.isnan(ao).all()) and bool((aa == -7).all()))

    cases = [(dict(n_frames=None), "n_frames is NULL"),
             (dict(n_frames=(4, 0, 2)), "n_frames[1] = 0 frames (1..32 per stream and call)"),
             (dict(n_frames=(4, 1, 33)), "n_frames[2] = 33 frames (1..32 per stream and call)"),
             (dict(n_active=8, n_frames=(32,) * 7 + (33,), slots=tuple(range(8))), "n_frames[7] = 33 frames"),
             (dict(n_active=8, n_frames=(32,) * 7 + (31,), slots=tuple(range(7)) + (0,)), "slot 0 is named twice"),
             (dict(n_active=9, n_frames=(32,) * 8 + (1,), slots=tuple(range(8)) + (0,)), "9 streams with 257 frames in all (at most 256 rows per call: use forward() with h0 / h_last)"),
             (dict(n_active=0, slots=(5,)), "0 streams (1..256 per call)"),
             (dict(n_active=9, n_frames=(1,) * 9, slots=tuple(range(8)) + (0,)), "9 slots (1..8 per call"),
             (dict(slots=(5, 8, 2)), "slots[1] = 8 is outside the pool (capacity 8)"),
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
    assert step(n_active=8, n_frames=(32,) * 8, slots=tuple(range(8)), w_bytes=ws.numel()) == 0      # R = 256 exactly
    torch.cuda.synchronize()
    assert [_rec(e, p, block, s)[0] for s in range(cap)] == [34, 32, 36, 32, 32, 40, 32, 32]
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
            sp.push_ragged([sp.open()], [1], rgb[:1], None)
        eng.lib.prego_stream_pool_destroy(pe)
    # the Python surface: a closed slot, a duplicate slot, a count of 0 or 33, more than 256 rows - block and records as they were
    pool = StreamPool(e, capacity=16, window=3, max_events=8)
    a, b = pool.open(), pool.open()
    pool.push_ragged([a, b], [2, 5], rgb[:7], None)
    torch.cuda.synchronize()
    before = pool._block.clone()
    closed = 7
    with pytest.raises(PregoError, match=f"slot {closed} is not open"):
        pool.push_ragged([a, closed], [1, 2], rgb[:3], None)
    with pytest.raises(PregoError, match="named twice"):
        pool.push_ragged([a, a], [1, 2], rgb[:3], None)
    with pytest.raises(PregoError, match=r"n_frames\[1\] = 0 frames"):
        pool.push_ragged([a, b], [3, 0], rgb[:3], None)
    with pytest.raises(PregoError, match=r"n_frames\[0\] = 33 frames"):
        pool.push_ragged([a, b], [33, 1], rgb[:34], None)
    more = [pool.open() for _ in range(7)]
    with pytest.raises(PregoError, match="257 frames in all"):
        pool.push_ragged([a, b] + more, [32] * 8 + [1], torch.cat([rgb, rgb[:1]]), None)
    with pytest.raises(PregoError, match="expected packed frames as"):
        pool.push_ragged([a, b], [1, 2], rgb[:4], None)
    with pytest.raises(PregoError, match="2 slots, 3 counts"):
        pool.push_ragged([a, b], [1, 2, 3], rgb[:6], None)
    torch.cuda.synchronize()
    assert torch.equal(pool._block, before)
    assert pool.events(a)["frames"] == 2 and pool.events(b)["frames"] == 5
    lib.prego_stream_pool_destroy(p)
    lib.prego_stream_pool_destroy(p12)
    e.check()


# ---- 5. no allocation, no host wait -------------------------------------------------------------------------------------------------------------
def test_push_ragged_allocates_nothing_and_waits_for_nothing():
    dbg = _lib.load_debug()
    e = TW._real_engine("bf16", 8, lib=dbg)
    pool = StreamPool(e, capacity=256)
    assert pool.lib is dbg
    counts = [8, 1, 3, 5, 2, 7, 4, 6] * 2
    slots = [pool.open() for _ in range(256)][::-1][:16]
    rgb = TW._feat((sum(counts), 2048), 8)
    bufs = pool.push_ragged(slots, counts, rgb, None)
    e.check()

    def alloc_counts():
        a, w = C.c_int64(), C.c_int64()
        assert dbg.prego_debug_alloc_count(C.byref(a), C.byref(w)) == 0
        return a.value, w.value
    n0 = alloc_counts()
    pool.push_ragged(slots, counts, rgb, None, out=bufs[0], argmax=bufs[1], ant_out=bufs[2], ant_argmax=bufs[3])
    assert alloc_counts() == n0                              # no device allocation and no host wait inside the call
    e.check()
    assert [pool.events(s)["frames"] for s in slots[:3]] == [16, 2, 6]
