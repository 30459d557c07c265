"""GPU tests of the Transformer stream pool (ViTEnc.stream_pool -> TransformerStreamPool.push = prego_vit_step_pool; csrc/vit_stream.hip).

What is held exactly (torch.equal): the ring bookkeeping, the token kernel's fp32 rows (one add per element), the vote record (integers),
and the bits of two pools fed the same streams in the same order under different slot numbers.  What is held to a tolerance: a stream's
logits come out of GEMMs whose kernel variant the dispatcher picks by row count, so against `forward_frames` (M = frames of a video) and
against a call with the rows in another order they are compared at the project's own tiers (tests/test_gpu_transformer.py):
  device tier  2e-3 * max(1, scale)  two device routes of the same math (what holds forward_frames against the batched forward)
  oracle tier  1e-2 * max(1, scale)  against oracle_np.vit_forward
The device tier is the gate for the ROUTING (which ring row feeds which token): `test_the_device_tier_prices_a_wrong_window` recomputes
from the oracle alone what an off-by-one window or one stale token does to the logits and fails if any effect is below 3 x that tier."""
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
from prego_amd.aggregate import OVERFLOW_FULL, OnlineRecord, aggregate, aggregate_online   # noqa: E402
from prego_amd.config import assembly101_cfg                       # noqa: E402

WINDOW = 32
DEV_TIER, ORACLE_TIER = 2e-3, 1e-2
LENS, OPEN_AT = (70, 45, 20), (0, 3, 10)          # the ring wraps twice, wraps once, never fills
SLOTS_A, SLOTS_B = (5, 0, 6), (1, 2, 3)
ORACLE_TICKS = (0, 1, 2, 30, 31, 32, 33, 63, 64, 65)               # and each stream's last


def _cfg(layers=1, dtype="fp16", window=WINDOW, **kw):
    return assembly101_cfg(model="Transformer", window_size=window, patch_dim=1, num_heads=8, attn_dropout_rate=0.0, dropout=0.0,
                           num_layers=layers, compute_dtype=dtype, **kw)


@functools.lru_cache(maxsize=None)
def _sd(layers, window=WINDOW, no_rgb=False):
    return W.vit_state_dict(_cfg(layers, window=window, no_rgb=no_rgb), 20)


@functools.lru_cache(maxsize=None)
def _videos(n_frames=LENS):
    """(rgb, flow) numpy [L, 2048] per stream"""
    return tuple((W.tsn_features((L, 2048), 50 + i, "vs.rgb"), W.tsn_features((L, 2048), 50 + i, "vs.flow")) for i, L in enumerate(n_frames))


def _model(layers=1, dtype="fp16", window=WINDOW, **kw):
    from prego_amd.registry import build_model
    import prego_amd.transformer  # noqa: F401
    m = build_model(_cfg(layers, dtype, window, **kw), "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _sd(layers, window, bool(kw.get("no_rgb", False))).items()})
    return m.eval()


def _windows(x, ticks, window=WINDOW):
    """explicit zero-fronted windows of one video ending at `ticks` (dataset.py:53-55 at stride 1)"""
    pad = np.concatenate([np.zeros((window - 1, x.shape[1]), np.float32), x])
    return np.stack([pad[t:t + window] for t in ticks])


def _oracle_ticks(L):
    return sorted({t for t in ORACLE_TICKS if t < L} | {L - 1})


@functools.lru_cache(maxsize=None)
def _oracle(layers):
    """per stream: (ticks, logits [len(ticks), C]) of oracle_np.vit_forward on the explicit windows; computed once per depth"""
    out = []
    for (rgb, flow), L in zip(_videos(), LENS):
        ticks = _oracle_ticks(L)
        out.append((ticks, O.vit_forward(_sd(layers), _windows(rgb, ticks), _windows(flow, ticks), 8, num_layers=layers)["logits"][:, 0]))
    return out


@functools.lru_cache(maxsize=None)
def _schedule():
    """seeded per-tick subset and order of the open, unfinished streams: a list of tuples of stream numbers; a stream opens at OPEN_AT"""
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
    assert {len(p) for p in ticks if p} == {1, 2, 3}                 # n_active runs through 1, 2 and 3
    return tuple(ticks)


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


def _replay(m, slots, reverse=False, ring_checks=False, **pool_kw):
    """the churn schedule through a fresh pool: per stream the logits [L, C] and argmax [L] as pushed, plus (ring_checks) the failures
    of the ring properties after every push"""
    pool = m.stream_pool(capacity=8, **pool_kw)
    vids = [(torch.from_numpy(r).cuda(), torch.from_numpy(f).cuda()) for r, f in _videos()]
    bias = m.linear_encoding.bias.detach().float()
    at, logits, args, bad, prev = [0, 0, 0], [[], [], []], [[], [], []], [], {}
    for t, pick in enumerate(_schedule()):
        for s in range(3):
            if OPEN_AT[s] == t:
                _open_slot(pool, slots[s])
        if not pick:
            continue
        pick = pick[::-1] if reverse else pick
        rgb = torch.stack([vids[s][0][at[s]] for s in pick])
        flow = torch.stack([vids[s][1][at[s]] for s in pick])
        before = pool._block.clone() if ring_checks else None
        out, am = pool.push([slots[s] for s in pick], rgb, flow)
        for i, s in enumerate(pick):
            logits[s].append(out[i].clone())
            args[s].append(am[i].clone())
            at[s] += 1
        if not ring_checks:
            continue
        after = pool._block
        for slot in range(8):                                        # slots not named: byte-identical, ring rows, ring words and record
            if slot in [slots[s] for s in pick]:
                continue
            for a, b in _slot_bytes(pool, slot):
                if not torch.equal(before[a:b], after[a:b]):
                    bad.append(f"tick {t}: slot {slot}, not named, changed in bytes [{a}, {b})")
        for s in pick:
            rows, fill = pool.window(slots[s])
            if fill != min(at[s], WINDOW):
                bad.append(f"tick {t}: stream {s} fill {fill} after {at[s]} frames")
            if s in prev and not torch.equal(rows[:-1], prev[s][1:]):
                bad.append(f"tick {t}: stream {s}: the window did not shift by one row")
            if fill < WINDOW and not torch.equal(rows[:WINDOW - fill], bias.expand(WINDOW - fill, -1)):
                bad.append(f"tick {t}: stream {s}: rows in front of the stream are not the encoding bias")
            if at[s] == 1 and fill == 1 and WINDOW > 1 and torch.equal(rows[-1], bias):
                bad.append(f"tick {t}: stream {s}: the newest row is the bias, not an encoded frame")
            prev[s] = rows
    assert at == list(LENS)
    torch.cuda.synchronize()
    return {"logits": [torch.stack(x) for x in logits], "argmax": [torch.stack(x) for x in args], "bad": bad, "pool": pool}


@functools.lru_cache(maxsize=None)
def _churn(layers, dtype):
    m = _model(layers, dtype)
    res = _replay(m, SLOTS_A, ring_checks=True)
    res["model"] = m
    res["frames"] = [m.forward_frames(torch.from_numpy(r).cuda(), torch.from_numpy(f).cuda())[0] for r, f in _videos()]
    return res


# ---- the routing gate, from the oracle alone ------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [1, 2])
def test_the_device_tier_prices_a_wrong_window(layers):
    """Before any kernel output is looked at: what a wrong window does to the logits, from oracle_np.vit_forward alone.  Per stream, on
    at most 12 sampled ticks: the window one frame late (off by one), and one stale token - the row a ring would still hold from
    `window` frames earlier or, where the stream is younger than that, from the slot's previous stream - at positions 0, window // 2
    and window - 1.  Every effect must be at least 3 x the device tier, or that tier could not tell a wrong ring row from rounding."""
    sd = _sd(layers)
    vids = _videos()
    worst = {}
    for s, ((rgb, flow), L) in enumerate(zip(vids, LENS)):
        other = vids[(s + 1) % 3]
        ticks = sorted({int(t) for t in np.linspace(1, L - 1, 6)})
        wr, wf = _windows(rgb, ticks), _windows(flow, ticks)
        cases = {"right": (wr, wf), "off by one": (_windows(rgb, [t - 1 for t in ticks]), _windows(flow, [t - 1 for t in ticks]))}
        for pos in (0, WINDOW // 2, WINDOW - 1):
            sr, sf = wr.copy(), wf.copy()
            for i, t in enumerate(ticks):
                f = t - WINDOW + 1 + pos - WINDOW                      # the frame the ring row held one lap earlier
                src = (rgb, flow, f) if f >= 0 else (other[0], other[1], (t + pos) % len(other[0]))
                sr[i, pos], sf[i, pos] = src[0][src[2]], src[1][src[2]]
            cases[f"stale token {pos}"] = (sr, sf)
        logit = {k: O.vit_forward(sd, a, b, 8, num_layers=layers, dt=np.float32)["logits"][:, 0] for k, (a, b) in cases.items()}
        scale = float(np.abs(logit["right"]).max())
        for k in cases:
            if k != "right":
                eff = np.abs(logit[k] - logit["right"]).max(axis=1)
                worst[k] = min(worst.get(k, np.inf), float(eff.min()) / (DEV_TIER * max(1.0, scale)))
    print(f"layers {layers}: smallest effect of a wrong window, in device tiers: " + ", ".join(f"{k} {v:.1f}" for k, v in worst.items()))
    assert all(v >= 3.0 for v in worst.values()), worst


# ---- 1. churn against both references ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("layers", [1, 2])
def test_churn_matches_forward_frames_and_the_oracle(layers, dtype):
    res = _churn(layers, dtype)
    worst_dev = worst_or = 0.0
    for s in range(3):
        got, ref = res["logits"][s], res["frames"][s]
        assert got.shape == (LENS[s], 86)
        assert torch.equal(res["argmax"][s], got.argmax(1).to(torch.int32))          # the returned argmax is the logits', exactly
        scale = max(1.0, float(ref.abs().max()))
        err = (got - ref).abs().max(dim=1).values
        worst_dev = max(worst_dev, float(err.max()) / scale)
        print(f"layers {layers} {dtype} stream {s}: push vs forward_frames max abs err {float(err.max()):.3e} at tick {int(err.argmax())}, scale {scale:.2f}")
        assert float(err.max()) < DEV_TIER * scale, (s, int(err.argmax()), float(err.max()))
        ticks, oref = _oracle(layers)[s]
        oscale = max(1.0, float(np.abs(oref).max()))
        oerr = np.abs(got[ticks].cpu().numpy() - oref).max()
        ferr = np.abs(ref[ticks].cpu().numpy() - oref).max()
        worst_or = max(worst_or, float(oerr) / oscale)
        print(f"layers {layers} {dtype} stream {s}: vs oracle: push {oerr:.3e}, forward_frames {ferr:.3e}, scale {oscale:.2f}")
        assert oerr < ORACLE_TIER * oscale and ferr < ORACLE_TIER * oscale
    print(f"layers {layers} {dtype}: worst push-vs-forward_frames {worst_dev:.3e} x scale (tier {DEV_TIER}), worst vs oracle {worst_or:.3e} x scale")


# ---- 2. ring exactness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
@pytest.mark.parametrize("layers", [1, 2])
def test_ring_bookkeeping_is_exact(layers, dtype):
    """after every push of the churn: window(slot) shifted by exactly one row, fill == min(frames, 32), bias rows in front of the
    stream, and every slot the call did not name byte-identical (ring rows, ring words, record)"""
    bad = _churn(layers, dtype)["bad"]
    assert not bad, bad[:5]


# ---- 3. the token kernel's x, exactly ---------------------------------------------------------------------------------------------
def test_ring_tokens_x_is_exact():
    dbg = _lib.load_debug()                       # prego_debug_vit_ring_tokens: only in libprego_amd_debug.so
    m = _model(2, "fp16")
    pool = m.stream_pool(capacity=8)
    sa, sb = _open_slot(pool, 2), _open_slot(pool, 7)
    (ra, fa), (rb, fb) = [(torch.from_numpy(r).cuda(), torch.from_numpy(f).cuda()) for r, f in _videos()[:2]]
    pe = m.position_encoding.pe.weight.detach().float()
    cls = m.cls_token.detach().float().reshape(1, -1)
    x = torch.empty((2, WINDOW + 1, m.embedding_dim), dtype=torch.float32, device="cuda")
    for t in range(51):
        if t < LENS[1]:
            pool.push([sa, sb], torch.stack([ra[t], rb[t]]), torch.stack([fa[t], fb[t]]))
        else:
            pool.push([sa], ra[t:t + 1], fa[t:t + 1])                 # stream b stays at its last frame
        if t not in (0, 31, 32, 50):
            continue
        want = {s: torch.cat([pool.window(s)[0] + pe[:WINDOW], cls + pe[WINDOW:]]) for s in (sa, sb)}
        for order in ([sa, sb], [sb, sa]):
            x.fill_(float("nan"))
            rc = dbg.prego_debug_vit_ring_tokens(pool.p, 2, (C.c_int32 * 2)(*order), C.c_void_p(x.data_ptr()), None)
            assert rc == 0, dbg.prego_last_error()
            torch.cuda.synchronize()
            for i, s in enumerate(order):
                assert torch.equal(x[i], want[s]), (t, order, s)


# ---- 4. slot independence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_slot_numbers_do_not_change_the_bits_and_order_stays_inside_the_tier(dtype):
    res = _churn(1, dtype)
    low = _replay(res["model"], SLOTS_B)
    for s in range(3):
        assert torch.equal(low["logits"][s], res["logits"][s]) and torch.equal(low["argmax"][s], res["argmax"][s]), s
    rev = _replay(res["model"], SLOTS_A, reverse=True)
    exact = True
    for s in range(3):
        scale = max(1.0, float(res["frames"][s].abs().max()))
        err = float((rev["logits"][s] - res["logits"][s]).abs().max())
        exact = exact and err == 0.0
        assert err < DEV_TIER * scale, (s, err)
    print(f"{dtype}: rows in reversed `slots` order were {'bit-identical' if exact else 'within the device tier, not bit-identical'}")


# ---- 5. close / reopen: the stale-row case ----------------------------------------------------------------------------------------
def test_a_reopened_slot_sees_nothing_of_the_stream_before():
    m = _model(1, "fp16")
    pool = m.stream_pool(capacity=4)
    (ra, fa), (rb, fb) = [(torch.from_numpy(r).cuda(), torch.from_numpy(f).cuda()) for r, f in _videos()[:2]]
    slot = pool.open()
    for t in range(50):
        pool.push([slot], ra[t:t + 1], fa[t:t + 1])
    assert pool.window(slot)[1] == WINDOW
    pool.close(slot)
    assert pool.open() == slot                                         # the same ring rows, still holding stream a's frames
    ref = m.forward_frames(rb, fb)[0]
    scale = max(1.0, float(ref.abs().max()))
    bias = m.linear_encoding.bias.detach().float()
    rows, fill = pool.window(slot)
    assert fill == 0 and torch.equal(rows, bias.expand(WINDOW, -1))
    worst = 0.0
    for t in range(LENS[1]):
        out, _ = pool.push([slot], rb[t:t + 1], fb[t:t + 1])
        worst = max(worst, float((out[0] - ref[t]).abs().max()))
        if t in (0, 10, 30):
            rows, fill = pool.window(slot)
            assert fill == t + 1 and torch.equal(rows[:WINDOW - fill], bias.expand(WINDOW - fill, -1))
    print(f"reopened slot vs forward_frames of the new video: max abs err {worst:.3e}, scale {scale:.2f}")
    assert worst < DEV_TIER * scale


# ---- 6. votes -----------------------------------------------------------------------------------------------------------------------
def test_votes_equal_the_host_model_fed_the_devices_own_ids():
    m = _model(1, "fp16")
    pool = m.stream_pool(capacity=4, vote_window=7, max_events=64)
    full = m.stream_pool(capacity=4, vote_window=7, max_events=2)
    rgb, flow = [torch.from_numpy(a).cuda() for a in _videos()[0]]
    slot, fslot = pool.open(), full.open()
    ids, host = [], OnlineRecord(7, 86, 64)
    for t in range(LENS[0]):
        _, am = pool.push([slot], rgb[t:t + 1], flow[t:t + 1])
        full.push([fslot], rgb[t:t + 1], flow[t:t + 1])
        ids.append(int(am[0]))
        host.push(ids[-1])
        if t in (5, 6, 20, 48):                                        # inside the first window, at its end, mid-stream
            assert pool.events(slot) == host.result(), t
    got = pool.close(slot)
    assert got == aggregate_online(ids, 7, n_classes=86)
    want = aggregate({"v": {"pred": ids, "gt": [0] * len(ids)}}, window_size=7)["v"]
    assert got == {"pred": want["pred"], "changes_pred": want["changes_pred"]}
    print(f"vote window 7 over {len(ids)} frames: {len(got['pred'])} events")
    small = OnlineRecord(7, 86, 2)
    for i in ids:
        small.push(i)
    small.flush()
    assert small.overflow & OVERFLOW_FULL                              # the stream has more than two events: the case is live
    with pytest.raises(PregoError, match="max_events = 2"):
        full.close(fslot)
    assert full.free == 4                                              # the slot is freed all the same


# ---- 7. variants --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["causal", "no_rgb", "flow_none"])
def test_variants_match_forward_frames(variant):
    kw = {"causal": {"causal_attention": True}, "no_rgb": {"no_rgb": True}, "flow_none": {}}[variant]
    m = _model(1, "fp16", **kw)
    rgb, flow = [torch.from_numpy(a[:40]).cuda() for a in _videos()[0]]
    if variant == "no_rgb":
        rgb = None
    if variant == "flow_none":
        flow = None
    ref = m.forward_frames(rgb, flow)[0]
    pool = m.stream_pool(capacity=2)
    slot = pool.open()
    got = torch.stack([pool.push([slot], None if rgb is None else rgb[t:t + 1], None if flow is None else flow[t:t + 1])[0][0].clone()
                       for t in range(40)])
    scale = max(1.0, float(ref.abs().max()))
    err = float((got - ref).abs().max())
    print(f"{variant}: push vs forward_frames max abs err {err:.3e}, scale {scale:.2f}")
    assert err < DEV_TIER * scale


def test_window_128_three_streams():
    m = _model(1, "fp16", window=128)
    vids = [(torch.from_numpy(W.tsn_features((140, 2048), 60 + i, "vs128.rgb")).cuda(),
             torch.from_numpy(W.tsn_features((140, 2048), 60 + i, "vs128.flow")).cuda()) for i in range(3)]
    pool = m.stream_pool(capacity=5)
    slots = [_open_slot(pool, s) for s in (4, 1, 2)]
    got = torch.stack([pool.push(slots, torch.stack([v[0][t] for v in vids]), torch.stack([v[1][t] for v in vids]))[0].clone()
                       for t in range(140)])                           # [140, 3, C]
    for s in range(3):
        ref = m.forward_frames(*vids[s])[0]
        scale = max(1.0, float(ref.abs().max()))
        err = float((got[:, s] - ref).abs().max())
        print(f"window 128 stream {s}: max abs err {err:.3e}, scale {scale:.2f}")
        assert err < DEV_TIER * scale
        assert pool.window(slots[s])[1] == 128


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_untouched():
    m = _model(1, "fp16")
    lib, dev, h = m._eval_handle()
    vp = C.c_void_p
    cap = 8
    need = lib.prego_vit_stream_pool_bytes(h, cap, 16)
    assert need >= cap * WINDOW * 2048 * 4 and lib.prego_vit_stream_pool_bytes(h, 0, 16) == 0 and lib.prego_vit_stream_pool_bytes(h, cap, 0) == 0
    assert lib.prego_vit_stream_pool_bytes(h, 2 ** 31 - 1, 1 << 20) > 2 ** 31 - 1        # large pools are sized, not capped
    block = torch.empty(need + 256, dtype=torch.uint8, device="cuda")

    def err():
        return lib.prego_last_error().decode()

    def create(capacity=cap, vote_window=7, max_events=16, ptr=block.data_ptr(), nbytes=need, handle=h):
        p = vp()
        rc = lib.prego_vit_stream_pool_create(C.byref(p), handle, capacity, vote_window, max_events, vp(ptr) if ptr else None, nbytes, None)
        return rc, p
    for kw, msg in [({"vote_window": 0}, "vote_window 0"), ({"max_events": 0}, "max_events 0"), ({"capacity": 0}, "capacity 0"),
                    ({"ptr": 0}, "bytes"), ({"nbytes": need - 1}, "need"), ({"ptr": block.data_ptr() + 64}, "256-byte aligned"),
                    ({"handle": None}, "handle is NULL")]:
        rc, p = create(**kw)
        assert rc == -1 and not p.value and msg in err(), (kw, err())
    rc, p = create()
    assert rc == 0
    torch.cuda.synchronize()
    assert int(block[:need].max()) == 0                                # create zeroes the block: every slot is an empty stream
    # a few frames in, so that the block is not all zero
    rgb, flow = [torch.from_numpy(a[:3]).cuda() for a in _videos()[0]]
    ws_need = lib.prego_vit_step_pool_workspace_bytes(h, 3)
    assert ws_need > 0 and lib.prego_vit_step_pool_workspace_bytes(h, 0) == 0 and lib.prego_vit_step_pool_workspace_bytes(h, 257) == 0
    ws = torch.empty(ws_need + 256, dtype=torch.uint8, device="cuda")
    out = torch.empty((3, 86), dtype=torch.float32, device="cuda")
    am = torch.empty((3,), dtype=torch.int32, device="cuda")

    def step(handle=h, pool=p, n=3, slots=(1, 4, 6), r=rgb, f=flow, o=out, a=am, w=ws.data_ptr(), wb=ws_need):
        arr = (C.c_int32 * max(len(slots), 1))(*slots) if slots is not None else None
        return lib.prego_vit_step_pool(handle, pool, n, arr, vp(r.data_ptr()) if r is not None else None,
                                       vp(f.data_ptr()) if f is not None else None, vp(o.data_ptr()) if o is not None else None,
                                       vp(a.data_ptr()) if a is not None else None, 0, vp(w) if w else None, wb, None)
    assert step() == 0, err()
    torch.cuda.synchronize()
    good = out.clone()
    out.fill_(float("nan"))
    am.fill_(-7)
    ws.fill_(0xA5)
    snap = [t.clone() for t in (block, ws, out.view(torch.int32), am)]
    # other handles: fp32 operands, no weights yet, another class count
    m32 = _model(1, "fp32")
    h32 = m32._eval_handle()[2]
    bare = vp()
    assert lib.prego_vit_create(C.byref(bare), 2048, 2048, 2048, 1024, 8, 1, WINDOW, 86) == 0
    from prego_amd.registry import build_model
    m12 = build_model(_cfg(1, "fp16", num_classes=12), "cuda:0").eval()
    h12 = m12._eval_handle()[2]
    mw = build_model(_cfg(1, "fp16", window=64), "cuda:0").eval()
    hw = mw._eval_handle()[2]
    big = torch.empty(lib.prego_vit_stream_pool_bytes(h, 300, 1), dtype=torch.uint8, device="cuda")
    rc, p300 = create(capacity=300, max_events=1, ptr=big.data_ptr(), nbytes=big.numel())
    assert rc == 0
    torch.cuda.synchronize()
    big_snap = big.clone()
    EINVAL, EWS = -1, -3
    cases = [
        ({"handle": h32}, EINVAL, "fp32-operand handle"),
        ({"handle": bare}, EINVAL, "before set_weights"),
        ({"handle": h12}, EINVAL, "the pool was created for"),
        ({"handle": hw}, EINVAL, "the pool was created for"),
        ({"n": 0, "slots": ()}, EINVAL, "0 slots (1..8"),
        ({"n": 9, "slots": tuple(range(9))}, EINVAL, "9 slots (1..8"),
        ({"pool": p300, "n": 257, "slots": tuple(range(257))}, EINVAL, "257 slots (1..256"),
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
    ]
    for kw, code, msg in cases:
        rc = step(**kw)
        assert rc == code and msg in err(), (kw, rc, err())
    for fn in (lib.prego_vit_stream_pool_flush, lib.prego_vit_stream_pool_reset):
        assert fn(p, 1, (C.c_int32 * 1)(8), None) == EINVAL and "outside the pool" in err()
        assert fn(p, 2, (C.c_int32 * 2)(3, 3), None) == EINVAL and "named twice" in err()
    ptr, nb = vp(), C.c_size_t()
    assert lib.prego_vit_stream_pool_record(p, 8, C.byref(ptr), C.byref(nb)) == EINVAL
    assert lib.prego_vit_stream_pool_window(p, -1, vp(out.data_ptr()), None, None) == EINVAL
    torch.cuda.synchronize()
    for name, was, now in zip(("block", "workspace", "out", "argmax"), snap, (block, ws, out.view(torch.int32), am)):
        assert torch.equal(was, now), f"a refused call wrote the {name}"
    assert torch.equal(big, big_snap)
    # the same call goes through afterwards, and continues the streams
    assert step() == 0, err()
    torch.cuda.synchronize()
    assert not torch.equal(out, good) and bool(torch.isfinite(out).all())      # frame 2 of the three streams, not frame 1 again
    for q in (p, p300):
        lib.prego_vit_stream_pool_destroy(q)
    lib.prego_vit_destroy(bare)
    # the Python surface
    with pytest.raises(PregoError, match="fp32"):
        m32.stream_pool(capacity=2)
    pool = m.stream_pool(capacity=3)
    s0 = pool.open()
    with pytest.raises(PregoError, match="slot 1 is not open"):
        pool.push([s0, 1], rgb[:2], flow[:2])
    with pytest.raises(PregoError, match="slot 0 is named twice"):
        pool.push([s0, s0], rgb[:2], flow[:2])
    with pytest.raises(PregoError, match="expected rgb"):
        pool.push([s0], rgb[:2], flow[:1])
    m.compute_dtype = "fp32"
    try:
        with pytest.raises(PregoError, match="fp32"):
            pool.push([s0], rgb[:1], flow[:1])
    finally:
        m.compute_dtype = "fp16"
    assert pool.events(s0)["frames"] == 0                              # none of the refused pushes reached the record
