"""GPU tests of the Transformer stream pool's bursts (TransformerStreamPool.push_bursts = prego_vit_step_pool_bursts; csrc/vit_stream.hip:
vit_burst_tokens, vit_ring_commit_burst; csrc/stream_pool.hip: pool_vote_ragged).  The setup is tests/test_gpu_vit_stream_pool.py's,
restated: window 32, E 2048, W.vit_state_dict(cfg, 20), W.tsn_features videos of 70 / 45 / 20 frames.

Exact (torch.equal): the token kernel's fp32 rows against source + pe in torch (one add per element), the commit against the host model
(ring_after_burst), all-counts-1 bursts against `push` (the same GEMM shapes, byte-equal sources), two pools under different slot
numbers, and the vote record (integers).  At the project's tiers (tests/test_gpu_transformer.py): every returned row against
`forward_frames` - the device tier 2e-3 * max(1, scale), the routing gate of tests/test_gpu_vit_stream_pool.py (a window one frame late
is >= 6 such tiers) - and sampled rows against oracle_np.vit_forward at 1e-2 * max(1, scale).  A burst's logits are NOT promised
bit-identical to the same frames pushed one at a time (the GEMM variant goes by row count); (f) prints the measured difference."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from oracle import oracle_np as O                                  # noqa: E402
from prego_amd import _lib                                         # noqa: E402
from prego_amd import weights as W                                 # noqa: E402
from prego_amd._lib import PregoError                              # noqa: E402
from prego_amd.aggregate import OVERFLOW_FULL, OnlineRecord, aggregate_online   # noqa: E402
from prego_amd.config import assembly101_cfg                       # noqa: E402
from prego_amd.stream_pool import burst_offsets, ring_after_burst  # noqa: E402

WINDOW = 32
DEV_TIER, ORACLE_TIER = 2e-3, 1e-2
LENS, OPEN_AT = (70, 45, 20), (0, 3, 10)
SLOTS_A, SLOTS_B = (5, 0, 6), (1, 2, 3)
ORACLE_TICKS = (0, 1, 2, 30, 31, 32, 33, 63, 64, 65)               # and each stream's last
GHOST = 40                                                         # frames of video 0 a stream leaves in stream 2's slot before it


def _cfg(layers=1, dtype="fp16", window=WINDOW, **kw):
    return assembly101_cfg(model="Transformer", window_size=window, patch_dim=1, num_heads=8, attn_dropout_rate=0.0, dropout=0.0,
                           num_layers=layers, compute_dtype=dtype, **kw)


@functools.lru_cache(maxsize=None)
def _sd(layers, window=WINDOW, no_rgb=False):
    return W.vit_state_dict(_cfg(layers, window=window, no_rgb=no_rgb), 20)


@functools.lru_cache(maxsize=None)
def _videos():
    """(rgb, flow) numpy [L, 2048] per stream"""
    return tuple((W.tsn_features((L, 2048), 50 + i, "vs.rgb"), W.tsn_features((L, 2048), 50 + i, "vs.flow")) for i, L in enumerate(LENS))


@functools.lru_cache(maxsize=None)
def _cuda_videos():
    return tuple((torch.from_numpy(r).cuda(), torch.from_numpy(f).cuda()) for r, f in _videos())


@functools.lru_cache(maxsize=None)
def _model(layers=1, dtype="fp16", window=WINDOW, variant=""):
    from prego_amd.registry import build_model
    import prego_amd.transformer  # noqa: F401
    kw = {"": {}, "causal": {"causal_attention": True}, "no_rgb": {"no_rgb": True}}[variant]
    m = build_model(_cfg(layers, dtype, window, **kw), "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _sd(layers, window, variant == "no_rgb").items()})
    return m.eval()


def _windows(x, ticks, window=WINDOW):
    pad = np.concatenate([np.zeros((window - 1, x.shape[1]), np.float32), x])
    return np.stack([pad[t:t + window] for t in ticks])


@functools.lru_cache(maxsize=None)
def _oracle(layers):
    """per stream: (ticks, logits [len(ticks), C]) of oracle_np.vit_forward on the explicit windows; computed once per depth"""
    out = []
    for (rgb, flow), L in zip(_videos(), LENS):
        ticks = sorted({t for t in ORACLE_TICKS if t < L} | {L - 1})
        out.append((ticks, O.vit_forward(_sd(layers), _windows(rgb, ticks), _windows(flow, ticks), 8, num_layers=layers)["logits"][:, 0]))
    return out


@functools.lru_cache(maxsize=None)
def _frames(layers, dtype):
    m = _model(layers, dtype)
    return [m.forward_frames(r, f)[0] for r, f in _cuda_videos()]


def _open_slot(pool, want):
    """pool.open() hands out the lowest free slot: open up to `want`, give the others back"""
    got = []
    while True:
        s = pool.open()
        if s == want:
            break
        got.append(s)
    for s in got:
        pool.close(s)
    return want


def _slot_bytes(pool, slot):
    """the three byte ranges of the block that belong to a slot: ring rows, ring words, record"""
    T, E, cap = pool._T, pool._E, pool.capacity
    ring_bytes = (cap * T * E * 4 + 255) // 256 * 256
    ptr, nb = C.c_void_p(), C.c_size_t()
    assert pool.lib.prego_vit_stream_pool_record(pool.p, slot, C.byref(ptr), C.byref(nb)) == 0
    rec = ptr.value - pool._block.data_ptr()
    return [(slot * T * E * 4, (slot + 1) * T * E * 4), (ring_bytes + slot * 16, ring_bytes + slot * 16 + 16), (rec, rec + nb.value)]


def _ring_words(pool, slot):
    a, b = _slot_bytes(pool, slot)[1]
    return [int(v) for v in pool._block[a:b].view(torch.int32).cpu()]


def _ring_rows(pool, slot):
    a, b = _slot_bytes(pool, slot)[0]
    return pool._block[a:b].view(torch.float32).view(pool._T, pool._E)


def _i32(v):
    return (C.c_int32 * len(v))(*v)


# ---- the slot states of (a) and (b) ---------------------------------------------------------------------------------------------------
STATES = {"empty": (1, 0), "young": (3, 10), "full": (4, 32), "wrapped": (6, 45), "reopened": (7, 0)}      # name -> (slot, frames)


def _prepared(m):
    """a pool of 8 slots in the five states: never fed, fill < T, full with head back at 0, wrapped head, and a slot reopened after a
    stream of 37 frames (head = fill = 0, the ring rows still another stream's).  Slots 0, 2 and 5 stay closed, slot 2 with stale rows."""
    pool = m.stream_pool(capacity=8, vote_window=5, max_events=16)
    (ra, fa), (rb, fb), _ = _cuda_videos()
    for name, (slot, _) in STATES.items():
        _open_slot(pool, slot)
    _open_slot(pool, 2)
    feed = {3: 10, 4: 32, 6: 45, 7: 37, 2: 5}
    for t in range(45):
        live = [s for s, n in feed.items() if t < n]
        src = [(ra, fa) if s in (3, 6, 2) else (rb, fb) for s in live]
        pool.push(live, torch.stack([v[0][t] for v in src]), torch.stack([v[1][t] for v in src]))
    pool.close(7)
    pool.close(2)
    assert _open_slot(pool, 7) == 7
    for name, (slot, frames) in STATES.items():
        assert _ring_words(pool, slot) == [frames % WINDOW, min(frames, WINDOW), 0, 0], name
    assert float(_ring_rows(pool, 7).abs().max()) > 0                   # the reopened slot's rows are not zero
    return pool


CALLS = [(("empty", 32), ("young", 1), ("full", 2), ("wrapped", 31), ("reopened", 7)),
         (("wrapped", 1), ("reopened", 32), ("empty", 13), ("full", 31), ("young", 2)),
         (("young", 32), ("full", 19)),
         (("reopened", 1),)]


def _enc_rows(R, E, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn((R, E), generator=g, dtype=torch.float32).cuda()


# ---- (a) the token rule, exactly ----------------------------------------------------------------------------------------------------
def test_burst_tokens_x_is_source_plus_pe_exactly():
    dbg = _lib.load_debug()
    m = _model(2, "fp16")
    pool = _prepared(m)
    E = m.embedding_dim
    pe = m.position_encoding.pe.weight.detach().float()
    cls_row = m.cls_token.detach().float().reshape(1, -1) + pe[WINDOW:]
    before = {name: pool.window(slot)[0] for name, (slot, _) in STATES.items()}
    snap = pool._block.clone()
    for c, call in enumerate(CALLS):
        slots, counts = [STATES[name][0] for name, _ in call], [k for _, k in call]
        R, off = sum(counts), burst_offsets(counts)
        enc = _enc_rows(R, E, 100 + c)
        x = torch.full((R, WINDOW + 1, E), float("nan"), dtype=torch.float32, device="cuda")
        rc = dbg.prego_debug_vit_burst_tokens(pool.p, len(slots), _i32(slots), _i32(counts), C.c_void_p(enc.data_ptr()),
                                              C.c_void_p(x.data_ptr()), None)
        assert rc == 0, dbg.prego_last_error()
        torch.cuda.synchronize()
        for i, (name, K) in enumerate(call):
            stream = torch.cat([before[name], enc[off[i]:off[i] + K]])  # the slot's window before the call, then the call's rows
            for k in range(K):
                want = torch.cat([stream[k + 1:k + 1 + WINDOW] + pe[:WINDOW], cls_row])
                assert torch.equal(x[off[i] + k], want), (c, name, k, int((x[off[i] + k] != want).any(dim=1).nonzero()[0]))
    assert torch.equal(pool._block, snap)                               # the token kernel commits nothing


# ---- (b) the commit, exactly ----------------------------------------------------------------------------------------------------------
def test_burst_commit_equals_the_host_model_byte_for_byte():
    dbg = _lib.load_debug()
    m = _model(2, "fp16")
    pool = _prepared(m)
    E = m.embedding_dim
    frames = {name: f for name, (_, f) in STATES.items()}
    for c, call in enumerate(CALLS):
        slots, counts = [STATES[name][0] for name, _ in call], [k for _, k in call]
        R, off = sum(counts), burst_offsets(counts)
        enc = _enc_rows(R, E, 200 + c)
        win = {name: pool.window(STATES[name][0])[0] for name, _ in call}
        words = {name: _ring_words(pool, STATES[name][0]) for name, _ in call}
        snap = pool._block.clone()
        rc = dbg.prego_debug_vit_burst_commit(pool.p, len(slots), _i32(slots), _i32(counts), C.c_void_p(enc.data_ptr()), None)
        assert rc == 0, dbg.prego_last_error()
        torch.cuda.synchronize()
        named = set(slots)
        for slot in range(8):
            ranges = _slot_bytes(pool, slot)
            for a, b in (ranges if slot not in named else ranges[2:]):  # a named slot's record is not the commit's to touch either
                assert torch.equal(snap[a:b], pool._block[a:b]), f"call {c}: slot {slot} changed in bytes [{a}, {b})"
        for i, (name, K) in enumerate(call):
            slot = STATES[name][0]
            head, fill = words[name][:2]
            assert (head, fill) == (frames[name] % WINDOW, min(frames[name], WINDOW))
            h1, f1, rows = ring_after_burst(head, fill, WINDOW, K)
            assert _ring_words(pool, slot) == [h1, f1, 0, 0], (c, name)
            a, _ = _slot_bytes(pool, slot)[0]
            want_ring = snap[a:a + WINDOW * E * 4].view(torch.float32).view(WINDOW, E).clone()
            want_ring[rows] = enc[off[i]:off[i] + K]
            assert torch.equal(_ring_rows(pool, slot), want_ring), (c, name)
            got, got_fill = pool.window(slot)
            assert got_fill == f1 and torch.equal(got, torch.cat([win[name], enc[off[i]:off[i] + K]])[K:]), (c, name)
            frames[name] += K


# ---- the schedules --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _churn_schedule():
    """tests/test_gpu_vit_stream_pool.py's seeded per-tick subset and order of the open, unfinished streams"""
    rng = np.random.default_rng(7)
    left, ticks, t = list(LENS), [], 0
    while any(left):
        live = [s for s in range(3) if t >= OPEN_AT[s] and left[s] > 0]
        t += 1
        if not live:
            ticks.append(())
            continue
        k = int(rng.integers(1, len(live) + 1))
        pick = [int(s) for s in rng.permutation(live)[:k]]
        for s in pick:
            left[s] -= 1
        ticks.append(tuple(pick))
    return tuple(ticks)


@functools.lru_cache(maxsize=None)
def _ragged_schedule():
    """seeded calls, each a tuple of (stream, count): counts drawn from 1..32 (capped by what the stream has left), a varying subset
    and order of the live streams per call.  Stream 3 is the ghost: the first GHOST frames of video 0 into the slot stream 2 will get,
    closed before stream 2 opens ("open2") - stream 2 starts on a ring full of another stream's rows."""
    rng = np.random.default_rng(11)
    left = list(LENS) + [GHOST]
    opened, calls = {0, 3}, []
    forced = iter([32, 1, 31, 2])                                       # the edge counts, whatever the seed draws besides
    while any(left):
        if left[3] == 0 and 3 in opened:
            opened.remove(3)
            calls.append("open2")
            opened.add(2)
        if len(calls) == 1:
            opened.add(1)
        live = [s for s in sorted(opened) if left[s] > 0]
        n = int(rng.integers(1, len(live) + 1))
        call = []
        for s in (int(v) for v in rng.permutation(live)[:n]):
            k = min(next(forced, None) or int(rng.integers(1, 33)), left[s])
            left[s] -= k
            call.append((s, k))
        calls.append(tuple(call))
    counts = [k for c in calls if c != "open2" for _, k in c]
    assert {1, 2, 31, 32} <= set(counts) and any(2 < k < 31 for k in counts)
    assert {len(c) for c in calls if c != "open2"} >= {1, 2, 3} and 0 < calls.index("open2") < len(calls) - 1
    return tuple(calls)


def _video_of(s):
    return _cuda_videos()[0 if s == 3 else s]


def _replay_ragged(m, slots, one_frame=False, **pool_kw):
    """the ragged schedule through a fresh pool: per stream (3 = the ghost) the logits and argmax as returned, in frame order.
    one_frame: the same frames, one `push` per frame.  slots: the slot of streams 0, 1, 2; the ghost uses stream 2's."""
    pool = m.stream_pool(capacity=8, **pool_kw)
    slot_of = {0: slots[0], 1: slots[1], 2: slots[2], 3: slots[2]}
    at, logits, args, closed = [0, 0, 0, 0], [[], [], [], []], [[], [], [], []], {}
    is_open = set()
    for call in _ragged_schedule():
        if call == "open2":
            closed[3] = pool.close(slot_of[3])
            is_open.discard(3)
            continue
        for s, _ in call:
            if s not in is_open:
                _open_slot(pool, slot_of[s])
                is_open.add(s)
        if one_frame:
            for s, k in call:
                for t in range(at[s], at[s] + k):
                    out, am = pool.push([slot_of[s]], _video_of(s)[0][t:t + 1], _video_of(s)[1][t:t + 1])
                    logits[s].append(out.clone())
                    args[s].append(am.clone())
                at[s] += k
            continue
        rgb = torch.cat([_video_of(s)[0][at[s]:at[s] + k] for s, k in call])
        flow = torch.cat([_video_of(s)[1][at[s]:at[s] + k] for s, k in call])
        counts = [k for _, k in call]
        out, am = pool.push_bursts([slot_of[s] for s, _ in call], counts, rgb, flow)
        assert out.shape == (sum(counts), 86) and am.shape == (sum(counts),)
        for (s, k), o in zip(call, burst_offsets(counts)):
            logits[s].append(out[o:o + k].clone())
            args[s].append(am[o:o + k].clone())
            at[s] += k
    assert at == list(LENS) + [GHOST]
    torch.cuda.synchronize()
    return {"logits": [torch.cat(x) for x in logits], "argmax": [torch.cat(x) for x in args], "pool": pool, "slot_of": slot_of,
            "closed": closed}


@functools.lru_cache(maxsize=None)
def _ragged(layers, dtype):
    return _replay_ragged(_model(layers, dtype), SLOTS_A)


# ---- (c) every count 1 = push, bit for bit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers,dtype", [(1, "fp16"), (2, "fp16"), (1, "bf16")])
def test_bursts_of_one_frame_are_push_bit_for_bit(layers, dtype):
    m = _model(layers, dtype)
    one, burst = m.stream_pool(capacity=8, vote_window=5, max_events=16), m.stream_pool(capacity=8, vote_window=5, max_events=16)
    vids, at = _cuda_videos(), [0, 0, 0]
    for t, pick in enumerate(_churn_schedule()):
        for s in range(3):
            if OPEN_AT[s] == t:
                _open_slot(one, SLOTS_A[s])
                _open_slot(burst, SLOTS_A[s])
        if not pick:
            continue
        rgb = torch.stack([vids[s][0][at[s]] for s in pick])
        flow = torch.stack([vids[s][1][at[s]] for s in pick])
        slots = [SLOTS_A[s] for s in pick]
        o1, a1 = one.push(slots, rgb, flow)
        o2, a2 = burst.push_bursts(slots, 1, rgb, flow) if t % 2 else burst.push_bursts(slots, [1] * len(slots), rgb, flow)
        assert torch.equal(o1, o2) and torch.equal(a1, a2), t
        assert torch.equal(one._block, burst._block), t                 # ring rows, ring words and records of all 8 slots
        for s in pick:
            at[s] += 1
    assert at == list(LENS)
    for s in range(3):
        assert one.close(SLOTS_A[s]) == burst.close(SLOTS_A[s])


# ---- (d) slot numbers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_slot_numbers_do_not_change_the_bits(dtype):
    res = _ragged(1, dtype)
    low = _replay_ragged(_model(1, dtype), SLOTS_B)
    for s in range(4):
        assert torch.equal(low["logits"][s], res["logits"][s]) and torch.equal(low["argmax"][s], res["argmax"][s]), s
    for s in range(3):
        a, b = res["pool"], low["pool"]
        for (a0, a1), (b0, b1) in zip(_slot_bytes(a, SLOTS_A[s]), _slot_bytes(b, SLOTS_B[s])):
            assert torch.equal(a._block[a0:a1], b._block[b0:b1]), s


# ---- (e) the record -------------------------------------------------------------------------------------------------------------------
def test_records_equal_the_host_model_fed_the_devices_own_ids():
    """vote window 5: a burst of up to 32 frames crosses window boundaries up to 7 times"""
    m = _model(1, "fp16")
    res = _replay_ragged(m, SLOTS_A, vote_window=5, max_events=64)
    pool = res["pool"]
    ghost_ids = [int(v) for v in res["argmax"][3].cpu()]
    assert res["closed"][3] == aggregate_online(ghost_ids, 5, n_classes=86)
    n_events = []
    for s in range(3):
        ids = [int(v) for v in res["argmax"][s].cpu()]
        assert len(ids) == LENS[s]
        host = OnlineRecord(5, 86, 64)
        for i in ids:
            host.push(i)
        assert pool.events(SLOTS_A[s]) == host.result(), s             # before the flush: the unfinished window is not voted
        got = pool.close(SLOTS_A[s])
        assert got == aggregate_online(ids, 5, n_classes=86), s
        n_events.append(len(got["pred"]))
    print(f"vote window 5: events per stream {n_events}")
    # a record too small: the overflow bit, as in the one-frame pool
    small = OnlineRecord(5, 86, 2)
    ids0 = [int(v) for v in res["argmax"][0].cpu()]
    for i in ids0:
        small.push(i)
    small.flush()
    assert small.overflow & OVERFLOW_FULL                              # stream 0 has more than two events: the case is live
    full = m.stream_pool(capacity=2, vote_window=5, max_events=2)
    slot = full.open()
    rgb, flow = _cuda_videos()[0]
    for a in range(0, LENS[0], 32):
        b = min(a + 32, LENS[0])
        _, am = full.push_bursts([slot], b - a, rgb[a:b], flow[a:b])
    with pytest.raises(PregoError, match="max_events = 2"):
        full.events(slot)
    with pytest.raises(PregoError, match="max_events = 2"):
        full.close(slot)
    assert full.free == 2                                              # the slot is freed all the same


# ---- (f) against forward_frames and the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("layers", [1, 2])
def test_ragged_bursts_match_forward_frames_and_the_oracle(layers, dtype):
    res = _ragged(layers, dtype)
    frames = _frames(layers, dtype)
    worst = 0.0
    for s in range(4):
        got, ref = res["logits"][s], frames[0 if s == 3 else s][:GHOST if s == 3 else None]
        assert got.shape == ref.shape
        assert torch.equal(res["argmax"][s], got.argmax(1).to(torch.int32))          # the returned argmax is the logits', exactly
        scale = max(1.0, float(ref.abs().max()))
        err = (got - ref).abs().max(dim=1).values
        worst = max(worst, float(err.max()) / scale)
        print(f"layers {layers} {dtype} stream {s}: bursts vs forward_frames max abs err {float(err.max()):.3e} at frame {int(err.argmax())}, "
              f"scale {scale:.2f}")
        assert float(err.max()) < DEV_TIER * scale, (s, int(err.argmax()), float(err.max()))
        if s == 3:
            continue
        ticks, oref = _oracle(layers)[s]
        oscale = max(1.0, float(np.abs(oref).max()))
        oerr = np.abs(got[ticks].cpu().numpy() - oref).max()
        print(f"layers {layers} {dtype} stream {s}: bursts vs oracle {oerr:.3e}, scale {oscale:.2f}")
        assert oerr < ORACLE_TIER * oscale
    # not a promise, a figure: the same frames through one `push` per frame (another GEMM variant where M differs)
    single = _replay_ragged(_model(layers, dtype), SLOTS_A, one_frame=True)
    diff = max(float((single["logits"][s] - res["logits"][s]).abs().max()) for s in range(4))
    print(f"layers {layers} {dtype}: worst bursts-vs-forward_frames {worst:.3e} x scale (tier {DEV_TIER}); bursts vs one push per frame: "
          f"max abs diff {diff:.3e}")
    for s in range(3):                                                   # the ring words agree; the rows come out of GEMMs of different M
        a, b = _slot_bytes(res["pool"], SLOTS_A[s])[1]
        assert torch.equal(res["pool"]._block[a:b], single["pool"]._block[a:b]), s


# ---- (g) variants ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["causal", "no_rgb", "flow_none"])
def test_variants_match_forward_frames(variant):
    m = _model(1, "fp16", WINDOW, "" if variant == "flow_none" else variant)
    rgb, flow = [v[:40] for v in _cuda_videos()[0]]
    if variant == "no_rgb":
        rgb = None
    if variant == "flow_none":
        flow = None
    ref = m.forward_frames(rgb, flow)[0]
    pool = m.stream_pool(capacity=2)
    slot = pool.open()
    got, a = [], 0
    for k in (3, 32, 5):
        got.append(pool.push_bursts([slot], [k], None if rgb is None else rgb[a:a + k], None if flow is None else flow[a:a + k])[0].clone())
        a += k
    got = torch.cat(got)
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    print(f"{variant}: bursts vs forward_frames max abs err {err:.3e}, scale {scale:.2f}")
    assert err < DEV_TIER * scale


# ---- (h) refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched():
    m = _model(1, "fp16")
    lib, dev, h = m._eval_handle()
    vp = C.c_void_p
    cap = 8
    need = lib.prego_vit_stream_pool_bytes(h, cap, 16)
    block = torch.empty(need + 256, dtype=torch.uint8, device="cuda")

    def err():
        return lib.prego_last_error().decode()

    def create(handle, capacity, blk):
        p = vp()
        assert lib.prego_vit_stream_pool_create(C.byref(p), handle, capacity, 7, 16, vp(blk.data_ptr()), blk.numel(), None) == 0, err()
        return p
    p = create(h, cap, block)
    rgb, flow = [v[:40].contiguous() for v in _cuda_videos()[0]]
    wsb = lib.prego_vit_step_pool_bursts_workspace_bytes
    ws_need = wsb(h, 3, 6)
    assert ws_need > 0 and ws_need == lib.prego_vit_step_pool_workspace_bytes(h, 6)          # vit_step_ws on R rows
    for n, R in [(0, 0), (3, 2), (257, 257), (1, 33), (9, 288), (8, 257)]:
        assert wsb(h, n, R) == 0, (n, R)
    assert wsb(h, 8, 256) > 0 and wsb(None, 3, 6) == 0
    ws = torch.empty(ws_need + 256, dtype=torch.uint8, device="cuda")
    out = torch.empty((6, 86), dtype=torch.float32, device="cuda")
    am = torch.empty((6,), dtype=torch.int32, device="cuda")

    def step(handle=h, pool=p, n=3, counts=(1, 3, 2), slots=(1, 4, 6), r=rgb, f=flow, o=out, a=am, w=ws.data_ptr(), wb=ws_need):
        carr = _i32(counts) if counts is not None else None
        sarr = (C.c_int32 * max(len(slots), 1))(*slots) if slots is not None else None
        return lib.prego_vit_step_pool_bursts(handle, pool, n, carr, sarr, vp(r.data_ptr()) if r is not None else None,
                                              vp(f.data_ptr()) if f is not None else None, vp(o.data_ptr()) if o is not None else None,
                                              vp(a.data_ptr()) if a is not None else None, 0, vp(w) if w else None, wb, None)
    assert step() == 0, err()
    torch.cuda.synchronize()
    good = out.clone()
    out.fill_(float("nan"))
    am.fill_(-7)
    ws.fill_(0xA5)
    snap = [t.clone() for t in (block, ws, out.view(torch.int32), am)]
    m32 = _model(1, "fp32")
    h32 = m32._eval_handle()[2]
    bare = vp()
    assert lib.prego_vit_create(C.byref(bare), 2048, 2048, 2048, 1024, 8, 1, WINDOW, 86) == 0
    from prego_amd.registry import build_model
    m12 = build_model(_cfg(1, "fp16", num_classes=12), "cuda:0").eval()
    h12 = m12._eval_handle()[2]
    m16 = build_model(_cfg(1, "fp16", window=16), "cuda:0").eval()     # its weights are whatever the constructor drew: never run
    h16 = m16._eval_handle()[2]
    blk16 = torch.empty(lib.prego_vit_stream_pool_bytes(h16, 4, 16), dtype=torch.uint8, device="cuda")
    p16 = create(h16, 4, blk16)
    big = torch.empty(lib.prego_vit_stream_pool_bytes(h, 300, 16), dtype=torch.uint8, device="cuda")
    p300 = create(h, 300, big)
    torch.cuda.synchronize()
    big_snap, snap16 = big.clone(), blk16.clone()
    EINVAL, EWS = -1, -3
    cases = [
        # what prego_vit_step_pool refuses
        ({"handle": h32}, EINVAL, "fp32-operand handle"),
        ({"handle": bare}, EINVAL, "before set_weights"),
        ({"handle": h12}, EINVAL, "the pool was created for"),
        ({"handle": h16}, EINVAL, "the pool was created for"),
        ({"n": 0, "slots": (), "counts": ()}, EINVAL, "0 slots (1..8"),
        ({"n": 9, "slots": tuple(range(9)), "counts": (1,) * 9}, EINVAL, "9 slots (1..8"),
        ({"pool": p300, "n": 257, "slots": tuple(range(257)), "counts": (1,) * 257}, EINVAL, "257 slots (1..256"),
        ({"slots": (1, 8, 6)}, EINVAL, "slots[1] = 8 is outside the pool"),
        ({"slots": (-1, 4, 6)}, EINVAL, "slots[0] = -1 is outside the pool"),
        ({"slots": (1, 4, 1)}, EINVAL, "slot 1 is named twice"),
        ({"slots": None}, EINVAL, "slots is NULL"),
        ({"w": 0}, EINVAL, "workspace is NULL"),
        ({"w": ws.data_ptr() + 64}, EINVAL, "256-byte aligned"),
        ({"wb": ws_need - 1}, EWS, "workspace"),
        ({"r": None}, EINVAL, "missing input"),
        ({"o": None}, EINVAL, "NULL argument"),
        ({"pool": None}, EINVAL, "NULL argument"),
        # the burst's own
        ({"counts": None}, EINVAL, "counts is NULL"),
        ({"counts": (1, 0, 2)}, EINVAL, "counts[1] = 0 (1..32"),
        ({"counts": (1, 3, -2)}, EINVAL, "counts[2] = -2 (1..32"),
        ({"counts": (33, 3, 2)}, EINVAL, "counts[0] = 33 (1..32"),
        ({"handle": h16, "pool": p16, "n": 1, "slots": (0,), "counts": (17,)}, EINVAL, "counts[0] = 17 (1..16"),
        ({"pool": p300, "n": 9, "slots": tuple(range(9)), "counts": (32,) * 8 + (1,)}, EINVAL, "sum to 257 rows (at most 256"),
        ({"counts": (1, 3, 3)}, EWS, "workspace"),                      # 7 rows in a workspace for 6
    ]
    for kw, code, msg in cases:
        rc = step(**kw)
        assert rc == code and msg in err(), (kw, rc, err())
    torch.cuda.synchronize()
    for name, was, now in zip(("block", "workspace", "out", "argmax"), snap, (block, ws, out.view(torch.int32), am)):
        assert torch.equal(was, now), f"a refused call wrote the {name}"
    assert torch.equal(big, big_snap) and torch.equal(blk16, snap16)
    # the same call goes through afterwards, and continues the streams
    assert step() == 0, err()
    torch.cuda.synchronize()
    assert not torch.equal(out, good) and bool(torch.isfinite(out).all())
    for q in (p, p300, p16):
        lib.prego_vit_stream_pool_destroy(q)
    lib.prego_vit_destroy(bare)
    # the Python surface
    pool = m.stream_pool(capacity=3)
    s0, s1 = pool.open(), pool.open()
    for args, msg in [(([s0, 2], [1, 1], rgb[:2], flow[:2]), "slot 2 is not open"), (([s0, s0], [1, 1], rgb[:2], flow[:2]), "slot 0 is named twice"),
                      (([s0, s1], [1], rgb[:1], flow[:1]), "2 slots, 1 counts"), (([s0], [0], rgb[:1], flow[:1]), r"counts\[0\] = 0"),
                      (([s0], [33], rgb[:33], flow[:33]), r"counts\[0\] = 33"), (([s0], 2, rgb[:3], flow[:2]), "expected rgb"),
                      (([s0], 2, rgb[:2], flow[:3]), "expected flow"), (([s0], 2, None, flow[:2]), "rgb is None")]:
        with pytest.raises(PregoError, match=msg):
            pool.push_bursts(*args)
    nine = m.stream_pool(capacity=9)
    with pytest.raises(PregoError, match="sum to 288 rows"):
        nine.push_bursts([nine.open() for _ in range(9)], 32, rgb, flow)
    assert pool.events(s0)["frames"] == 0 and pool.events(s1)["frames"] == 0      # none of the refused calls reached a record
    out2, am2 = pool.push_bursts([s1, s0], torch.tensor([2, 1]), rgb[:3], flow[:3])      # counts as a tensor
    assert out2.shape == (3, 86) and pool.events(s1)["frames"] == 2 and pool.events(s0)["frames"] == 1
