"""The stream pool (prego_stream_pool_*, prego_miniroad_step_pool, prego_amd/stream_pool.py; csrc/stream_pool.hip):
  1. exactly, against the saturated-gate automaton, with churn: streams opened at staggered ticks into scattered slots, a seeded schedule of
     which streams tick and in what order, n_active through 1..4, 5..16 and 17 or more; after EVERY push logits, argmax, anticipation
     logits / argmax and the slot's state equal the automaton's value of that (stream, frame), and close() equals the aggregation of it;
  2. step_wide's bits on real weights: push on permuted, scattered slots against step_wide on the same dense rows, the state carried over
     three ticks, and a second pool with other slot numbers gives the same bits;
  3. the shipped G8 pair online: ids fed one frame per tick through vote(), close() equals the fixture, events() midway the host model;
  4. the window rule at the smallest shapes;  5. push feeds the vote;  6. a slot is clean after close;  7. overflow writes nothing
     past the record;  8. refusals through raw ctypes, each with its message, nothing written;  9. no allocation, no host wait."""
import ctypes as C
import gzip
import json
import os
import random

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import _lib                                            # noqa: E402
from prego_amd._lib import PregoError                                 # noqa: E402
from prego_amd.aggregate import aggregate, aggregate_online           # noqa: E402
from prego_amd.engine import MiniRoadEngine                           # noqa: E402
from prego_amd.stream_pool import StreamPool                          # noqa: E402
from tests import test_gpu_step_wide as TW                            # noqa: E402  its references and engines are computed once and shared

DEV = "cuda:0"
EINVAL = -1
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _agg(ids, window):
    a = aggregate({"v": {"pred": [int(i) for i in ids], "gt": [0] * len(ids)}}, window_size=window)["v"]
    return {"pred": a["pred"], "changes_pred": a["changes_pred"]}


# ---- 1. the automaton, with churn ---------------------------------------------------------------------------------------------------------
CHURN = [(cid, dt, ant) for cid in ("L1-C12", "L4-C12") for dt in ("bf16", "fp16") for ant in (True, False)]


def _schedule(n, T, seed):
    """[(streams opened at this tick, streams that take a frame at this tick, in call order)]: the first three ticks walk the three
    regimes of the step (<= 4: fused LayerNorm, 5..16: step's launches, >= 17: the wide kernels), the rest draw a regime and an order"""
    rng = random.Random(seed)
    order = list(range(n))
    rng.shuffle(order)
    open_at = [order[:4], order[4:12], order[12:]]
    left, live, ticks = [T] * n, [], []
    sizes = [rng.randint(1, 4), rng.randint(5, 12), n]
    while True:
        t = len(ticks)
        opened = open_at[t] if t < 3 else []
        live += opened
        can = [s for s in live if left[s] > 0]
        if not can:
            break
        k = sizes[t] if t < 3 else rng.choice([rng.randint(1, 4), rng.randint(5, 16), rng.randint(17, n)])
        act = rng.sample(can, min(k, len(can)))
        for s in act:
            left[s] -= 1
        ticks.append((opened, act))
    assert all(v == 0 for v in left)
    return ticks


@pytest.mark.parametrize("cid,dtype,ant", CHURN, ids=[f"{c}-{d}-{'ant' if a else 'trunk'}" for c, d, a in CHURN])
def test_pool_equals_the_automaton_with_churn(cid, dtype, ant):
    case, sd, n, T, x, res = TW._ref(cid)
    L, Cn, window = case.ant_len, case.n_classes, 3
    e = MiniRoadEngine(case.d_rgb, case.d_flow, case.emb, case.hid, Cn, DEV, dtype)
    e.set_weights(sd)
    if ant:
        e.set_anticipation(sd[TW.A_KEYS[0]], sd[TW.A_KEYS[1]], L)
    want_l, want_a, want_h = (t.view(n, T, -1) for t in (res.logits, res.argmax, res.h[0]))
    want_al, want_aa = res.ant_logits.view(n, T, L, Cn), res.ant_argmax.view(n, T, L)
    pool = StreamPool(e, capacity=64, window=window, max_events=8)
    # scattered slots: the pool is filled, a seeded subset of n slots is closed again, and the streams take the lowest hole as they open
    rng = random.Random(7)
    for _ in range(64):
        pool.open()
    holes = rng.sample(range(64), n)
    for s in holes:
        assert pool.close(s) == {"pred": [], "changes_pred": [0]}
    slot_of, frame, regimes = {}, [0] * n, set()
    for opened, act in _schedule(n, T, 11):
        for s in opened:
            slot_of[s] = pool.open()
        slots = [slot_of[s] for s in act]
        fr = [frame[s] for s in act]
        got = pool.push(slots, torch.stack([x[s, f] for s, f in zip(act, fr)]), None, softmax=False)
        assert len(got) == (4 if ant else 2)
        k = len(act)
        regimes.add(0 if k <= 4 else 1 if k <= 16 else 2)
        si, fi = torch.tensor(act, device=DEV), torch.tensor(fr, device=DEV)
        assert torch.equal(got[0].to(torch.float64), want_l[si, fi]), "logits"
        assert got[1].dtype == torch.int32 and torch.equal(got[1], want_a[si, fi, 0]), "argmax"
        assert torch.equal(torch.stack([pool.state(s) for s in slots]), want_h[si, fi].to(torch.float32)), "state"
        if ant:
            assert torch.equal(got[2].to(torch.float64), want_al[si, fi]), "anticipation logits"
            assert torch.equal(got[3], want_aa[si, fi]), "anticipation argmax"
        for s in act:
            frame[s] += 1
    assert regimes == {0, 1, 2} and frame == [T] * n
    assert sorted(slot_of.values()) == sorted(holes) and sorted(holes) != list(range(min(holes), min(holes) + n))
    ids = want_a[:, :, 0].cpu().tolist()
    for s in range(n):
        assert pool.close(slot_of[s]) == _agg(ids[s], window), f"stream {s}"
    e.check()


# ---- 2. step_wide's bits on real weights --------------------------------------------------------------------------------------------------
BITS = [(dt, n, sm, ant) for dt in ("bf16", "fp16") for n in (5, 37) for sm in (True, False) for ant in (True, False)]


@pytest.mark.parametrize("dtype,n,softmax,ant", BITS, ids=[f"{d}-n{n}-{'probs' if s else 'logits'}-{'ant' if a else 'trunk'}" for d, n, s, a in BITS])
def test_push_has_step_wides_bits_on_real_weights(dtype, n, softmax, ant):
    e = TW._real_engine(dtype, 3)
    pools = [StreamPool(e, capacity=64), StreamPool(e, capacity=200)]
    rng = random.Random(n)
    taken = []
    for pool, cap in zip(pools, (64, 200)):
        for _ in range(cap):
            pool.open()
        keep = rng.sample(range(cap), n)                      # permuted and scattered: the order of the list is the order of the rows
        for s in set(range(cap)) - set(keep):
            pool.close(s)
        taken.append(keep)
    assert taken[0] != taken[1] and taken[0] != sorted(taken[0])
    h = torch.zeros((n, 1024), device=DEV)
    for t in range(3):
        rgb, flow = TW._feat((n, 2048), 110 + t), TW._feat((n, 2048), 120 + t)
        want = e.step_wide(rgb, flow, h, softmax=softmax, want_ant=ant)
        for pool, slots in zip(pools, taken):
            got = pool.push(slots, rgb, flow, softmax=softmax, want_ant=ant)
            assert len(got) == len(want) == (4 if ant else 2)
            for name, g, w in zip(("out", "argmax", "ant_out", "ant_argmax"), got, want):
                assert g.shape == w.shape and torch.equal(g, w), f"tick {t}: {name}"
            assert torch.equal(torch.stack([pool.state(s) for s in slots]), h), f"tick {t}: state"
    assert float(h.abs().max()) > 0
    e.check()


# ---- 3. the shipped pair, online ------------------------------------------------------------------------------------------------------------
def test_the_four_shortest_g8_videos_online_through_vote():
    with gzip.open(os.path.join(G, "g8_output_miniROAD.json.gz"), "rt") as f:
        data = json.load(f)
    fixture = json.load(open(os.path.join(G, "g8_aggregated_data.json")))
    vids = sorted(data, key=lambda k: -len(data[k]["pred"]))[-4:]            # the longest of the four first: the live set is a prefix
    lens = [len(data[v]["pred"]) for v in vids]
    assert lens == [9015, 6971, 5157, 3702]
    mat = torch.zeros((lens[0], 4), dtype=torch.int32)
    for j, v in enumerate(vids):
        mat[:lens[j], j] = torch.tensor(data[v]["pred"], dtype=torch.int32)
    mat = mat.to(DEV)
    pool = StreamPool(TW._real_engine("bf16", 3), capacity=8, window=200)
    slots = [pool.open() for _ in vids]
    midway = 1101
    for t in range(lens[0]):
        while lens[len(slots) - 1] == t:                                     # a stream that has had its last frame closes
            j = len(slots) - 1
            assert pool.close(slots.pop()) == {k: fixture[vids[j]][k] for k in ("pred", "changes_pred")}, vids[j]
        pool.vote(slots, mat[t, :len(slots)])
        if t + 1 == midway:
            for j, s in enumerate(slots):
                ev = pool.events(s)
                assert ev.pop("frames") == midway
                assert ev == aggregate_online(data[vids[j]]["pred"][:midway - midway % 200], 200, n_classes=12), vids[j]
    assert pool.close(slots.pop()) == {k: fixture[vids[0]][k] for k in ("pred", "changes_pred")}
    assert not slots and pool.free == 8


# ---- 4. the window rule at the smallest shapes ----------------------------------------------------------------------------------------------
def _feed(pool, streams):
    """streams: {slot: ids}; one id per live stream and tick"""
    for t in range(max(len(v) for v in streams.values())):
        live = [s for s, v in streams.items() if len(v) > t]
        pool.vote(live, [streams[s][t] for s in live])


def test_window_rule_at_the_smallest_shapes():
    e = TW._real_engine("bf16", 3)
    pool = StreamPool(e, capacity=8, window=4, max_events=4)
    streams = {pool.open(): ids for ids in ([3, 1, 3, 1], [7], [2, 0, 0, 2, 5], [], [1, 1, 4, 4, 4, 1, 4, 1, 9])}
    _feed(pool, streams)
    assert pool.events(0) == {"pred": [1], "changes_pred": [4], "frames": 4}              # a 2-2 tie: the lowest id wins
    assert pool.events(1) == {"pred": [], "changes_pred": [0], "frames": 1}               # no finished window yet
    assert pool.events(2) == {"pred": [0], "changes_pred": [4], "frames": 5}
    want = [{"pred": [1], "changes_pred": [4]}, {"pred": [7], "changes_pred": [1]}, {"pred": [0, 5], "changes_pred": [4, 5]},
            {"pred": [], "changes_pred": [0]}, {"pred": [1, 9], "changes_pred": [8, 9]}]
    for s, ids in streams.items():
        got = pool.close(s)
        assert got == want[s], s
        if ids:
            assert got == aggregate_online(ids, 4) == _agg(ids, 4)
    one = StreamPool(e, capacity=2, window=1, max_events=8)
    s = one.open()
    _feed(one, {s: [2, 2, 0, 1, 1]})
    assert one.events(s) == {"pred": [2, 0, 1], "changes_pred": [2, 3, 5], "frames": 5}
    assert one.close(s) == {"pred": [2, 0, 1], "changes_pred": [2, 3, 5]}


# ---- 5. push feeds the vote -------------------------------------------------------------------------------------------------------------------
def test_push_feeds_the_vote():
    e = TW._real_engine("bf16", 3)
    pool = StreamPool(e, capacity=16, window=3)
    lens = {pool.open(): T for T in (1, 3, 4, 7, 9)}
    ids = {s: [] for s in lens}
    for t in range(9):
        live = [s for s in reversed(list(lens)) if lens[s] > t]
        rgb = TW._feat((len(live), 2048), 200 + t) * torch.arange(1, len(live) + 1, device=DEV)[:, None]
        am = pool.push(live, rgb, None, want_ant=False)[1].cpu().tolist()
        for s, a in zip(live, am):
            ids[s].append(a)
    for s, T in lens.items():
        assert len(ids[s]) == T
        assert pool.close(s) == _agg(ids[s], 3), s
    e.check()


# ---- 6. reuse ---------------------------------------------------------------------------------------------------------------------------------
def test_a_closed_slot_is_a_fresh_stream():
    e = TW._real_engine("bf16", 3)
    pool = StreamPool(e, capacity=4, window=2)
    a, b = pool.open(), pool.open()
    for t in range(3):
        pool.push([b, a], TW._feat((2, 2048), 300 + t), None)
    assert float(pool.state(b).abs().max()) > 0 and pool.events(b)["frames"] == 3
    assert len(pool.close(b)["pred"]) >= 1
    assert pool.open() == b                                                # the lowest free slot: the one just closed
    assert pool.events(b) == {"pred": [], "changes_pred": [0], "frames": 0}
    assert not bool(pool.state(b).any())
    rgb = TW._feat((1, 2048), 310)
    h = torch.zeros((1, 1024), device=DEV)
    want = e.step(rgb, None, h, want_ant=True)
    got = pool.push([b], rgb, None)
    assert all(torch.equal(g, w) for g, w in zip(got, want)) and torch.equal(pool.state(b), h[0])
    assert pool.events(a)["frames"] == 3                                   # the neighbour went on undisturbed
    e.check()


# ---- 7. / 8. the record's bounds and the refusals, through the C ABI ---------------------------------------------------------------------------
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


def _raw_record(e, p, block, slot):
    ptr, nb = C.c_void_p(), C.c_size_t()
    assert e.lib.prego_stream_pool_record(p, slot, C.byref(ptr), C.byref(nb)) == 0
    off = ptr.value - block.data_ptr()
    return block[off:off + nb.value].view(torch.int32).cpu().tolist()


def test_overflow_drops_events_and_writes_nothing_past_the_record():
    e = TW._real_engine("bf16", 3)
    lib = e.lib
    p, block, need = _raw_pool(e, 3, 1, 4)
    torch.cuda.synchronize()
    assert bool((block[:need] == 0).all()) and bool((block[need:] == 0xA5).all())          # create zeroes exactly the pool
    for t in range(7):                                                      # slot 1: seven alternating ids, slot 2: the same id
        ids = torch.tensor([t % 2, 5], dtype=torch.int32, device=DEV)
        assert lib.prego_stream_pool_vote(p, 2, _slots(1, 2), _p(ids), None) == 0
    torch.cuda.synchronize()
    cpad, me = 88, 4                                                        # 86 classes rounded up to 4
    r0, r1, r2 = (_raw_record(e, p, block, s) for s in range(3))
    assert len(r1) * 4 == (4 + cpad + 2 * me) * 4
    assert r1[:4] == [7, 1, 4, 1] and r1[4:4 + cpad] == [0] * cpad           # frames, last vote + 1, n_events, overflow: record full
    assert r1[4 + cpad:] == [0, 1, 0, 1, 0, 1, 2, 3]
    assert r2[:4] == [7, 6, 1, 0] and r2[4 + cpad:] == [5, 0, 0, 0, 0, 0, 0, 0]   # the neighbouring record is intact
    assert r0 == [0] * len(r0)
    assert bool((block[need:] == 0xA5).all()), "written past prego_stream_pool_bytes"
    assert not bool(block[:3 * 1024 * 4].any())                             # no state row was touched
    lib.prego_stream_pool_destroy(p)
    q = C.c_void_p()
    assert lib.prego_stream_pool_create(C.byref(q), e.h, 3, 1, 4, _p(block), need - 1, None) == EINVAL and not q.value
    assert f"need {need}" in lib.prego_last_error().decode()
    # the Python surface: close raises and frees the slot all the same
    pool = StreamPool(e, capacity=4, window=1, max_events=4)
    s, nb = pool.open(), pool.open()
    for t in range(6):
        pool.vote([s, nb], [t % 2, 3])
    with pytest.raises(PregoError, match="max_events = 4"):
        pool.close(s)
    assert pool.free == 3 and pool.open() == s and pool.events(s)["frames"] == 0
    assert pool.close(nb) == {"pred": [3], "changes_pred": [6]}
    pool.vote([s], [86])
    with pytest.raises(PregoError, match=r"outside \[0, 86\)"):
        pool.close(s)
    assert pool.free == 4


def test_refusals_through_the_c_abi():
    e = TW._real_engine("bf16", 3)
    lib = e.lib
    err = lambda: lib.prego_last_error().decode()
    cap, n = 8, 3
    p, block, need = _raw_pool(e, cap, 200, 16)
    torch.cuda.synchronize()
    ws_need = lib.prego_miniroad_step_pool_workspace_bytes(e.h, n)
    assert ws_need > 0 and lib.prego_miniroad_step_pool_workspace_bytes(e.h, 37) > lib.prego_miniroad_step_wide_workspace_bytes(e.h, 37)
    assert lib.prego_miniroad_step_pool_workspace_bytes(e.h, 0) == 0 and lib.prego_miniroad_step_pool_workspace_bytes(e.h, 257) == 0
    rgb = TW._feat((16, 2048), 400)
    ws = torch.full((lib.prego_miniroad_step_pool_workspace_bytes(e.h, 16) + 256,), 0x5A, dtype=torch.uint8, device=DEV)
    out, am = torch.full((16, 86), float("nan"), device=DEV), torch.full((16,), -7, dtype=torch.int32, device=DEV)
    ao, aa = torch.full((16, 3, 86), float("nan"), device=DEV), torch.full((16, 3), -7, dtype=torch.int32, device=DEV)
    assert lib.prego_miniroad_step_pool(e.h, p, n, _slots(5, 0, 2), _p(rgb), None, _p(out), _p(am), None, None, 1, _p(ws), ws_need, None) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[:n]).any()) and bool(torch.isnan(out[n:]).all())
    out.fill_(float("nan"))
    am.fill_(-7)
    snap, ws_snap = block.clone(), ws.clone()

    def step(handle=None, pool=p, n_active=n, slots=(5, 0, 2), w=ws, w_off=0, w_bytes=None, ant=False, eng=e):
        return eng.lib.prego_miniroad_step_pool((handle or eng).h if handle is not False else None, pool, n_active,
                                                _slots(*slots) if slots is not None else None, _p(rgb), None, _p(out), _p(am),
                                                _p(ao) if ant else None, _p(aa) if ant else None, 1,
                                                None if w is None else C.c_void_p(w.data_ptr() + w_off), ws_need if w_bytes is None else w_bytes, None)

    def untouched(blk=None, sn=None):
        torch.cuda.synchronize()
        blk, sn = (block, snap) if blk is None else (blk, sn)
        return (torch.equal(blk, sn) and torch.equal(ws, ws_snap) and bool(torch.isnan(out).all()) and bool((am == -7).all())
                and bool(torch.isnan(ao).all()) and bool((aa == -7).all()))

    cases = [(dict(n_active=0, slots=(5,)), "0 streams (1..256 per call)"),
             (dict(n_active=257, slots=tuple(range(8))), "257 streams (1..256 per call)"),
             (dict(n_active=9, slots=tuple(range(8)) + (0,)), "9 slots (1..8 per call"),
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
    # vote / flush / reset / record take the same slot checks
    ids = torch.zeros((3,), dtype=torch.int32, device=DEV)
    for call, tail in ((lib.prego_stream_pool_vote, (_p(ids), None)), (lib.prego_stream_pool_flush, (None,)), (lib.prego_stream_pool_reset, (None,))):
        assert call(p, 3, _slots(1, 8, 2), *tail) == EINVAL and "outside the pool" in err()
        assert call(p, 3, _slots(1, 2, 1), *tail) == EINVAL and "named twice" in err()
        assert call(p, 0, _slots(1), *tail) == EINVAL and "0 slots" in err()
        assert call(None, 1, _slots(1), *tail) == EINVAL and "pool is NULL" in err()
    assert lib.prego_stream_pool_vote(p, 1, _slots(1), None, None) == EINVAL and "ids is NULL" in err()
    ptr, nb = C.c_void_p(), C.c_size_t()
    assert lib.prego_stream_pool_record(p, 8, C.byref(ptr), C.byref(nb)) == EINVAL and "outside the pool" in err()
    assert untouched()
    # create
    q = C.c_void_p()
    blk = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    for args, msg in (((cap, 0, 16, _p(blk), need), "window 0"), ((cap, 200, 0, _p(blk), need), "max_events 0"),
                      ((0, 200, 16, _p(blk), need), "capacity 0"), ((cap, 200, 16, None, need), "block"),
                      ((cap, 200, 16, C.c_void_p(blk.data_ptr() + 16), need), "256-byte aligned"),
                      ((cap, 200, 16, _p(blk), need - 1), f"need {need}")):
        assert lib.prego_stream_pool_create(C.byref(q), e.h, *args, None) == EINVAL and msg in err() and not q.value, msg
    assert lib.prego_stream_pool_create(C.byref(q), None, cap, 200, 16, _p(blk), need, None) == EINVAL and "handle is NULL" in err()
    assert lib.prego_stream_pool_bytes(e.h, 0, 16) == 0 and lib.prego_stream_pool_bytes(e.h, cap, 0) == 0 and lib.prego_stream_pool_bytes(None, cap, 16) == 0
    torch.cuda.synchronize()
    assert bool((blk == 0xA5).all())
    # a pool created for another class count
    e12 = MiniRoadEngine(2048, 2048, 2048, 1024, 12, DEV, "bf16")
    p12, block12, _ = _raw_pool(e12, cap, 200, 16)
    torch.cuda.synchronize()
    snap12 = block12.clone()
    assert step(pool=p12) == EINVAL and "created for hidden_dim 1024 / 12 classes" in err() and untouched(block12, snap12) and untouched()
    assert step(handle=e12, pool=p12) == EINVAL and "before set_weights" in err() and untouched(block12, snap12)
    # everything step_wide refuses
    assert step(handle=False) == EINVAL and "handle is NULL" in err() and untouched()
    trunk = TW._real_engine("bf16", 3, ant=False)
    assert step(handle=trunk, ant=True) == EINVAL and "before set_anticipation" in err() and untouched()
    assert step(handle=trunk) == 0                                          # same geometry: the trunk-only handle may drive the pool
    for eng, msg in ((TW._real_engine("fp32", 3), "bf16 / fp16 handles"), (TW._real_engine("bf16", 3, hid=512), "hidden_dim 1024")):
        pe, be, _ = _raw_pool(eng, cap, 200, 16)
        torch.cuda.synchronize()
        sn = be.clone()
        out.fill_(float("nan"))
        am.fill_(-7)
        ws_snap = ws.clone()
        assert step(handle=eng, pool=pe) == EINVAL and msg in err() and untouched(be, sn), msg
        with pytest.raises(PregoError, match="the streaming kernels are built for"):
            sp = StreamPool(eng, capacity=4)
            sp.push([sp.open()], rgb[:1], None)
        eng.lib.prego_stream_pool_destroy(pe)
    # the Python surface
    pool = StreamPool(e, capacity=4)
    a = pool.open()
    with pytest.raises(PregoError, match="slot 1 is not open"):
        pool.push([a, 1], rgb[:2], None)
    with pytest.raises(PregoError, match="named twice"):
        pool.push([a, a], rgb[:2], None)
    with pytest.raises(PregoError, match="expected rgb"):
        pool.push([a], rgb[:2], None)
    pool.close(a)
    with pytest.raises(PregoError, match="slot 0 is not open"):
        pool.close(a)
    for _ in range(4):
        pool.open()
    with pytest.raises(PregoError, match="all 4 slots are open"):
        pool.open()
    lib.prego_stream_pool_destroy(p)
    lib.prego_stream_pool_destroy(p12)
    e.check()


# ---- 9. no allocation, no host wait -------------------------------------------------------------------------------------------------------------
def test_push_allocates_nothing_and_waits_for_nothing():
    dbg = _lib.load_debug()
    e = TW._real_engine("bf16", 8, lib=dbg)
    pool = StreamPool(e, capacity=256)
    assert pool.lib is dbg
    n = 144
    slots = [pool.open() for _ in range(256)][::-1][:n]
    rgb = TW._feat((n, 2048), 8)
    bufs = pool.push(slots, rgb, None)
    e.check()

    def counts():
        a, w = C.c_int64(), C.c_int64()
        assert dbg.prego_debug_alloc_count(C.byref(a), C.byref(w)) == 0
        return a.value, w.value
    n0 = counts()
    pool.push(slots, rgb, None, out=bufs[0], argmax=bufs[1], ant_out=bufs[2], ant_argmax=bufs[3])
    assert counts() == n0                                    # no device allocation and no host wait inside the call
    e.check()
    assert pool.events(slots[0])["frames"] == 2
