"""The ragged streaming step (prego_miniroad_step_ragged / _anticipation, MiniRoadEngine.step_ragged, MROAD / MROADA.step_ragged;
csrc/stream_frames.hip: frames_recur_ragged):
  1. exactly, against the saturated-gate automaton, after EVERY call: logits, argmax (ties included), the state, anticipation logits and
     argmax, every stream at its own position, for the shapes of tests/helpers/step_ragged_cases.py, both operand types, with the
     anticipation head and trunk-only;
  2. `step_frames`' bits on real weights: every row and the state of two consecutive ragged calls against one `step_frames` call per group
     of equal count; all counts equal against a single `step_frames` call; the same streams in another order give the same rows;
  3. contracts: nullable outputs, repeat calls with reused buffers, softmax rows, the counts array overwritten as soon as the call returns;
  4. the workspace: nothing written past workspace_bytes, one byte less is refused with nothing written;
  5. refusals through raw ctypes, each with its message, nothing written;
  6. no allocation and no host wait inside the call."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import _lib                                       # noqa: E402
from prego_amd._lib import PregoError                            # noqa: E402
from prego_amd.config import anticipation_cfg, assembly101_cfg  # noqa: E402
from prego_amd.engine import MiniRoadEngine                      # noqa: E402
from prego_amd.stream_pool import pack_bursts, unpack_bursts     # noqa: E402
from tests import test_gpu_step_wide as TW                       # noqa: E402  its references and engines are computed once and shared
from tests.helpers import ant_step_cases as S                    # noqa: E402
from tests.helpers import step_ragged_cases as SR                # noqa: E402
from tests.helpers import step_wide_cases as SW                  # noqa: E402

DEV = "cuda:0"
EINVAL = -1
_REF = {}


# ---- 1. the automaton ------------------------------------------------------------------------------------------------------------------
def _ref(src, cid):
    """(case, sd on the device, per-stream features [T_s, d], Result): one reference per case, computed once and left unchanged"""
    if src == "wide":
        case, sd, n, T, x, res = TW._ref(cid)
        return case, sd, list(x), res
    if "straggler" not in _REF:
        case, sd, feats, res = SR.straggler_reference(DEV)
        assert SW.trunk_ties(res) > 0 and S.ant_ties(res) > 0, "no tie in the reference"
        _REF["straggler"] = (case, {k: v.to(DEV) for k, v in sd.items()}, [r for r, _ in feats], res)
    return _REF["straggler"]


EXACT = [(sid, dt, ant) for sid in SR.SHAPES for dt in ("bf16", "fp16") for ant in (True, False)]


@pytest.mark.parametrize("sid,dtype,ant", EXACT, ids=[f"{s}-{d}-{'ant' if a else 'trunk'}" for s, d, a in EXACT])
def test_ragged_calls_equal_the_automaton(sid, dtype, ant):
    src, cid, streams, calls = SR.SHAPES[sid]
    case, sd, x, res = _ref(src, cid)
    L, Cn, n = case.ant_len, case.n_classes, len(streams)
    e = MiniRoadEngine(case.d_rgb, case.d_flow, case.emb, case.hid, Cn, DEV, dtype)
    e.set_weights(sd)
    if ant:
        e.set_anticipation(sd[TW.A_KEYS[0]], sd[TW.A_KEYS[1]], L)
    h = torch.zeros((n, case.hid), device=DEV)
    pos = [0] * n
    for c, counts in enumerate(calls):
        R = sum(counts)
        rgb, got_counts = pack_bursts([x[s][pos[i]:pos[i] + k] for i, (s, k) in enumerate(zip(streams, counts))])
        assert got_counts == list(counts)
        rows, last = SR.reference_rows(res.offs, streams, pos, counts)
        rows, last = torch.tensor(rows, device=DEV), torch.tensor(last, device=DEV)
        got = e.step_ragged(rgb, None, counts, h, softmax=False, want_ant=ant)
        assert len(got) == (4 if ant else 2)
        lg, am = got[0], got[1]
        assert lg.shape == (R, Cn) and am.shape == (R,) and am.dtype == torch.int32
        assert torch.equal(lg.to(torch.float64), res.logits[rows]), f"call {c}: logits"
        assert torch.equal(am, res.argmax[rows].view(R)), f"call {c}: argmax"
        assert torch.equal(h, res.h[0][last].to(torch.float32)), f"call {c}: state"
        if ant:
            al, aa = got[2], got[3]
            assert al.shape == (R, L, Cn) and aa.shape == (R, L) and aa.dtype == torch.int32
            assert torch.equal(al.to(torch.float64), res.ant_logits[rows]), f"call {c}: anticipation logits"
            assert torch.equal(aa, res.ant_argmax[rows]), f"call {c}: anticipation argmax"
        pos = [p + k for p, k in zip(pos, counts)]
    e.check()


# ---- 2. step_frames' bits on real weights -------------------------------------------------------------------------------------------------
def _frames_in_groups(e, rgb, flow, counts, h, softmax, ant):
    """the route a caller has without the ragged call: one step_frames per group of equal count, on packed rows gathered into [n_g, K, d].
    h [n, H] is advanced in place; returns the outputs scattered back into packed order"""
    off, outs = SR.offsets(counts), None
    for K, members in SR.groups_of_equal_count(counts).items():
        rows = torch.tensor([off[i] + t for i in members for t in range(K)], device=DEV)
        mi = torch.tensor(members, device=DEV)
        hg = h[mi].contiguous()
        o = e.step_frames(None if rgb is None else rgb[rows].view(len(members), K, -1).contiguous(),
                          None if flow is None else flow[rows].view(len(members), K, -1).contiguous(), hg, softmax=softmax, want_ant=ant)
        h[mi] = hg
        if outs is None:
            outs = [torch.empty((sum(counts),) + tuple(t.shape[2:]), dtype=t.dtype, device=DEV) for t in o]
        for dst, t in zip(outs, o):
            dst[rows] = t.reshape((len(members) * K,) + tuple(t.shape[2:]))
    return outs


def _inputs(inputs, R, seed):
    return (None if inputs == "no_rgb" else TW._feat((R, 2048), seed), None if inputs == "rgb" else TW._feat((R, 2048), seed + 10))


_C37 = (SR.seeded_counts(37, 1, 6, 37), SR.seeded_counts(37, 1, 6, 38))
BITS = [(name, cs) + v for name, cs in (("n5", ((3, 1, 5, 1, 2), (2, 4, 1, 1, 6))), ("n37", _C37)) for v in TW.VARIANTS]


@pytest.mark.parametrize("name,calls,dtype,L,inputs,softmax,ant", BITS,
                         ids=[f"{nm}-{d}-L{l}-{i}-{'probs' if s else 'logits'}-{'ant' if a else 'trunk'}" for nm, c, d, l, i, s, a in BITS])
def test_every_row_has_step_frames_bits_on_real_weights(name, calls, dtype, L, inputs, softmax, ant):
    e = TW._real_engine(dtype, L, no_rgb=inputs == "no_rgb", ant=ant)
    n = len(calls[0])
    assert calls[0] != calls[1] and len(set(calls[0])) >= 4 and len(set(calls[1])) >= 4
    hr, hg = TW._state(n), TW._state(n)
    for c, counts in enumerate(calls):                        # the second call starts from the state the first one left
        R = sum(counts)
        rgb, flow = _inputs(inputs, R, 30 + c)
        want = _frames_in_groups(e, rgb, flow, counts, hg, softmax, ant)
        got = e.step_ragged(rgb, flow, list(counts), hr, softmax=softmax, want_ant=ant)
        assert len(got) == len(want) == (4 if ant else 2)
        for nm, g, w in zip(("out", "argmax", "ant_out", "ant_argmax"), got, want):
            assert g.shape == w.shape and torch.equal(g, w), f"call {c}: {nm}"
        assert torch.equal(hr, hg), f"call {c}: state"
    assert not torch.equal(hr, TW._state(n))
    e.check()


@pytest.mark.parametrize("n,K", [(16, 4), (7, 1), (8, 32)], ids=["n16-K4", "n7-K1", "n8-K32"])
def test_all_counts_equal_is_step_frames(n, K):
    e = TW._real_engine("bf16", 3)
    rgb, flow = TW._feat((n, K, 2048), 41), TW._feat((n, K, 2048), 42)
    hf, hr = TW._state(n), TW._state(n)
    want = e.step_frames(rgb, flow, hf)
    got = e.step_ragged(rgb.view(n * K, -1), flow.view(n * K, -1), torch.full((n,), K, dtype=torch.int64), hr)
    for nm, g, w in zip(("out", "argmax", "ant_out", "ant_argmax"), got, want):
        assert torch.equal(g.view(w.shape), w), nm            # byte for byte the [n, K, ...] layout
    assert torch.equal(hr, hf)
    e.check()


def test_rows_do_not_depend_on_the_order_or_the_company_of_the_streams():
    e = TW._real_engine("fp16", 3)
    counts = [3, 1, 5, 1, 2, 6, 2, 4, 1, 3, 2, 5, 1, 1, 4, 2, 3, 6, 1]      # 19 streams: a tile and a tail
    n = len(counts)
    bursts = [TW._feat((k, 2048), 700 + s) for s, k in enumerate(counts)]
    h0 = TW._state(n)
    base_h = h0.clone()
    base = [unpack_bursts(t, counts) for t in e.step_ragged(pack_bursts(bursts)[0], None, counts, base_h)]
    g = torch.Generator().manual_seed(5)
    for order in (list(range(n))[::-1], torch.randperm(n, generator=g).tolist(), sorted(range(n), key=lambda s: counts[s])):
        oc = [counts[s] for s in order]
        h = h0[torch.tensor(order, device=DEV)].contiguous()
        got = [unpack_bursts(t, oc) for t in e.step_ragged(pack_bursts([bursts[s] for s in order])[0], None, oc, h)]
        for j in range(4):
            assert all(torch.equal(got[j][i], base[j][s]) for i, s in enumerate(order)), (order, j)
        assert torch.equal(h, base_h[torch.tensor(order, device=DEV)])
    # a stream alone, and among others with other counts
    for members in ([2], [2, 0], [5, 2, 13]):
        mc = [counts[s] for s in members]
        h = h0[torch.tensor(members, device=DEV)].contiguous()
        got = [unpack_bursts(t, mc) for t in e.step_ragged(pack_bursts([bursts[s] for s in members])[0], None, mc, h)]
        for j in range(4):
            assert all(torch.equal(got[j][i], base[j][s]) for i, s in enumerate(members)), (members, j)
        assert torch.equal(h, base_h[torch.tensor(members, device=DEV)])
    e.check()


# ---- 3. / 4. contracts and the workspace, through the C ABI ---------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class _Call:
    """one raw call of prego_miniroad_step_ragged_anticipation on fresh poisoned buffers; the counts array is overwritten as soon as the
    call has returned, before any synchronisation"""

    def __init__(self, e, counts, L=3, Cn=86, hid=1024):
        self.e, self.counts, self.n, self.R, self.L, self.Cn = e, list(counts), len(counts), sum(counts), L, Cn
        R = max(self.R, 1)
        self.rgb, self.flow, self.h0 = TW._feat((R, 2048), 51), TW._feat((R, 2048), 52), torch.tanh(TW._feat((self.n, hid), 53) - 0.5)
        self.need = e.lib.prego_miniroad_step_ragged_workspace_bytes(e.h, self.n, self.R)

    def __call__(self, want=(True, True, True, True), flags=1, ws_bytes=None, fn="prego_miniroad_step_ragged_anticipation", n_streams=None,
                 counts=None, counts_null=False, state=True, ws_null=False, ws_off=0):
        n, L, Cn = self.n, self.L, self.Cn
        R = max(self.R, 1)
        ws_bytes = self.need if ws_bytes is None else ws_bytes
        h = self.h0.clone()
        o, a = torch.full((R, Cn), float("nan"), device=DEV), torch.full((R,), -7, dtype=torch.int32, device=DEV)
        ao, aa = torch.full((R, L, Cn), float("nan"), device=DEV), torch.full((R, L), -7, dtype=torch.int32, device=DEV)
        canary = 4096
        ws = torch.full((max(ws_bytes, 0) + canary,), 0xA5, dtype=torch.uint8, device=DEV)
        assert ws.data_ptr() % 256 == 0
        bufs = [_p(t) if w else None for t, w in zip((o, a, ao, aa), want)]
        lib = self.e.lib
        ns = n if n_streams is None else n_streams
        cs = list(self.counts if counts is None else counts)
        cs += [1] * max(0, ns - len(cs))
        arr = None if counts_null else (C.c_int32 * len(cs))(*cs)
        wp = None if ws_null else C.c_void_p(ws.data_ptr() + ws_off)
        if fn.endswith("anticipation"):
            rc = lib.prego_miniroad_step_ragged_anticipation(self.e.h, ns, arr, _p(self.rgb), _p(self.flow), _p(h) if state else None, *bufs,
                                                             flags, wp, ws_bytes, None)
        else:
            rc = lib.prego_miniroad_step_ragged(self.e.h, ns, arr, _p(self.rgb), _p(self.flow), _p(h) if state else None, *bufs[:2], flags, wp,
                                                ws_bytes, None)
        if arr is not None:
            for i in range(len(cs)):                              # the caller's array is the caller's again
                arr[i] = 31 - (i % 31)
        torch.cuda.synchronize()
        assert bool((ws[max(ws_bytes, 0):] == 0xA5).all()), "written past workspace_bytes"
        self.ws = ws
        return rc, h, o, a, ao, aa

    def untouched(self, res):
        rc, h, o, a, ao, aa = res
        return (torch.equal(h, self.h0) and bool(torch.isnan(o).all()) and bool(torch.isnan(ao).all()) and bool((a == -7).all())
                and bool((aa == -7).all()) and bool((self.ws == 0xA5).all()))


COUNTS = (2, 5, 1, 3, 1, 4, 2)                                 # 7 streams, 18 rows, four launches


def test_repeat_calls_nullable_outputs_softmax_rows_argmax_and_the_counts_array():
    e = TW._real_engine("bf16", 3)
    call = _Call(e, COUNTS)
    full = call()
    assert full[0] == 0 and not torch.equal(full[1], call.h0)
    for t in full[2:]:
        assert not (torch.isnan(t).any() if t.is_floating_point() else (t == -7).any())
    # the array was overwritten right after the call returned: the results are those of a caller who keeps it (the engine's route)
    h = call.h0.clone()
    kept = e.step_ragged(call.rgb, call.flow, COUNTS, h)
    assert all(torch.equal(x, y) for x, y in zip(full[2:], kept)) and torch.equal(full[1], h)
    again = call()
    for x, y in zip(full[1:], again[1:]):
        assert torch.equal(x, y), "two identical calls"
    for i in range(4):                                        # each output NULL on its own: the others and the state keep their bits
        want = tuple(j != i for j in range(4))
        res = call(want)
        assert res[0] == 0 and torch.equal(res[1], full[1])
        for j in range(4):
            if j == i:
                assert bool(torch.isnan(res[2 + j]).all()) if j in (0, 2) else bool((res[2 + j] == -7).all())
            else:
                assert torch.equal(res[2 + j], full[2 + j])
    res = call((False, False, False, False))                  # the state alone
    assert res[0] == 0 and torch.equal(res[1], full[1])
    res = call((True, True, False, False))                    # the head is not launched: the trunk's bits
    assert res[0] == 0 and torch.equal(res[1], full[1]) and torch.equal(res[2], full[2]) and torch.equal(res[3], full[3])
    trunk = call(fn="prego_miniroad_step_ragged")
    assert trunk[0] == 0 and all(torch.equal(x, y) for x, y in zip(trunk[1:4], full[1:4]))
    err_p = float((full[2].double().sum(-1) - 1).abs().max())
    err_a = float((full[4].double().sum(-1) - 1).abs().max())
    print(f"softmax rows: |sum - 1| <= {err_p:.3e} (trunk), {err_a:.3e} (anticipation)")
    assert err_p < 1e-6 and err_a < 1e-6                      # what test_gpu_step_wide.py allows step_wide
    raw = call(flags=0)
    assert torch.equal(raw[5], raw[4].argmax(-1).to(torch.int32)) and torch.equal(raw[3], raw[2].argmax(-1).to(torch.int32))
    assert torch.equal(raw[5], full[5]) and torch.equal(raw[3], full[3])
    e.check()


def test_repeat_calls_through_the_engine_reuse_their_buffers():
    e = TW._real_engine("bf16", 3)
    counts = [4, 1, 2, 6, 3, 1]
    rgb, h1, h2 = TW._feat((sum(counts), 2048), 81), TW._state(6), TW._state(6)
    first = [t.clone() for t in e.step_ragged(rgb, None, counts, h1)]
    bufs = [torch.empty_like(t) for t in first]
    got = e.step_ragged(rgb, None, torch.tensor(counts), h2, out=bufs[0], argmax=bufs[1], ant_out=bufs[2], ant_argmax=bufs[3])
    assert all(g is b for g, b in zip(got, bufs)) and all(torch.equal(g, f) for g, f in zip(got, first)) and torch.equal(h1, h2)
    e.check()


def test_workspace_exact_size_and_one_byte_less():
    e = TW._real_engine("bf16", 3)
    lib = e.lib
    call = _Call(e, COUNTS)
    q = lib.prego_miniroad_step_ragged_workspace_bytes
    assert call.need > 0 and q(e.h, 7, 19) > call.need and q(e.h, 8, 18) > call.need
    assert q(e.h, 6, 18) == lib.prego_miniroad_step_frames_workspace_bytes(e.h, 6, 3)      # n and R only; all counts equal: step_frames' size
    for n, R in ((0, 1), (1, 0), (5, 4), (257, 257), (1, 257), (200, 257)):
        assert q(e.h, n, R) == 0, (n, R)
    assert q(e.h, 8, 256) > 0 and q(e.h, 256, 256) > 0 and q(e.h, 1, 1) > 0
    ok = call()                                               # the canary behind exactly workspace_bytes is checked inside
    assert ok[0] == 0 and bool((call.ws[:call.need] != 0xA5).any())
    for short in (call.need - 1, 0):
        res = call(ws_bytes=short)
        assert res[0] == EINVAL and "workspace" in lib.prego_miniroad_last_error(e.h).decode()
        assert f"{call.need}" in lib.prego_miniroad_last_error(e.h).decode()
        assert call.untouched(res)
    e.check()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi():
    def err(e):
        return e.lib.prego_miniroad_last_error(e.h).decode()
    e = TW._real_engine("bf16", 3)
    call = _Call(e, COUNTS)
    for kw, msg in ((dict(counts_null=True), "n_frames is NULL"),
                    (dict(counts=(2, 5, 0, 3, 1, 4, 2)), "n_frames[2] = 0 frames (1..32 per stream and call)"),
                    (dict(counts=(2, 5, 1, 3, 1, 4, 33)), "n_frames[6] = 33 frames (1..32 per stream and call)"),
                    (dict(counts=(2, -1, 1, 3, 1, 4, 2)), "n_frames[1] = -1 frames"),
                    (dict(n_streams=0), "0 streams (1..256 per call)"), (dict(n_streams=257), "257 streams (1..256 per call)"),
                    (dict(n_streams=9, counts=(32,) * 8 + (1,)), "9 streams with 257 frames in all (at most 256 rows per call: use forward() with h0 / h_last)"),
                    (dict(n_streams=129, counts=(2,) * 129), "129 streams with 258 frames in all (at most 256 rows per call"),
                    (dict(state=False), "h_state is NULL"),
                    (dict(ws_null=True), "workspace"), (dict(ws_off=16), "256-byte aligned")):
        for fn in ("prego_miniroad_step_ragged_anticipation", "prego_miniroad_step_ragged"):
            res = call(fn=fn, **kw)
            assert res[0] == EINVAL and msg in err(e), (kw, err(e))
            assert call.untouched(res), kw
    assert call()[0] == 0                                     # the handle survives
    e = TW._real_engine("bf16", 3, ant=False)
    call = _Call(e, COUNTS)
    res = call()
    assert res[0] == EINVAL and "step_anticipation before set_anticipation" in err(e) and call.untouched(res)
    assert call(fn="prego_miniroad_step_ragged")[0] == 0      # the trunk needs no set_anticipation
    e = TW._real_engine("fp32", 3)
    call = _Call(e, COUNTS)
    res = call()
    assert res[0] == EINVAL and "bf16 / fp16 handles" in err(e) and call.untouched(res)
    e = TW._real_engine("bf16", 3, hid=512)
    call = _Call(e, COUNTS, hid=512)
    res = call()
    assert res[0] == EINVAL and "hidden_dim 1024" in err(e) and call.untouched(res)
    e = MiniRoadEngine(2048, 2048, 2048, 1024, 86, DEV, "bf16")
    call = _Call(e, COUNTS)
    res = call(fn="prego_miniroad_step_ragged")
    assert res[0] == EINVAL and "before set_weights" in err(e) and call.untouched(res)


def test_engine_and_model_surface():
    e = TW._real_engine("bf16", 3, ant=False)
    with pytest.raises(PregoError, match="before set_anticipation"):
        e.step_ragged(TW._feat((5, 2048), 6), None, [2, 3], torch.zeros((2, 1024), device=DEV), want_ant=True)
    with pytest.raises(PregoError, match=r"n_frames\[1\] = 33 frames"):
        e.step_ragged(TW._feat((34, 2048), 6), None, [1, 33], torch.zeros((2, 1024), device=DEV))
    with pytest.raises(PregoError, match="258 frames in all"):
        e.step_ragged(TW._feat((258, 2048), 6), None, [2] * 129, torch.zeros((129, 1024), device=DEV))
    with pytest.raises(PregoError, match=r"expected packed frames as \[sum\(counts\) = 5, d\]"):
        e.step_ragged(TW._feat((2, 3, 2048), 6), None, [2, 3], torch.zeros((2, 1024), device=DEV))
    with pytest.raises(PregoError, match="counts is a sequence of ints or a 1-d CPU int tensor"):
        e.step_ragged(TW._feat((5, 2048), 6), None, torch.tensor([2, 3], device=DEV), torch.zeros((2, 1024), device=DEV))
    for eng in (TW._real_engine("fp32", 3), TW._real_engine("bf16", 3, hid=512)):
        with pytest.raises(PregoError, match="the streaming kernels are built for"):
            eng.step_ragged(TW._feat((5, 2048), 6), None, [2, 3], torch.zeros((2, eng.dims[3]), device=DEV))
    import prego_amd.model  # noqa: F401
    from prego_amd.registry import build_model
    for L, n_out in ((0, 2), (3, 4)):
        cfg = anticipation_cfg(assembly101_cfg(), L) if L else assembly101_cfg()
        m = build_model(dict(cfg, compute_dtype="bf16"), DEV)
        m.eval()
        counts = [3, 1, 2, 3, 1, 2]
        R = sum(counts)
        rgb, flow, hr, hg = TW._feat((R, 2048), 61), TW._feat((R, 2048), 62), TW._state(6), TW._state(6)
        got = m.step_ragged(rgb, flow, counts, hr)
        want = _frames_in_groups(m.engine(), rgb, flow, counts, hg, True, bool(L))
        assert len(got) == n_out and all(torch.equal(g, w) for g, w in zip(got, want)) and torch.equal(hr, hg)
        m.check()


# ---- 6. no allocation, no host wait ----------------------------------------------------------------------------------------------------
def test_step_ragged_allocates_nothing_and_waits_for_nothing():
    dbg = _lib.load_debug()
    e = TW._real_engine("bf16", 8, lib=dbg)
    counts = [8, 1, 3, 5, 2, 7, 4, 6] * 2
    rgb, h = TW._feat((sum(counts), 2048), 8), torch.zeros((16, 1024), device=DEV)
    bufs = e.step_ragged(rgb, None, counts, h, want_ant=True)
    e.check()

    def alloc_counts():
        a, w = C.c_int64(), C.c_int64()
        assert dbg.prego_debug_alloc_count(C.byref(a), C.byref(w)) == 0
        return a.value, w.value
    n0 = alloc_counts()
    e.step_ragged(rgb, None, counts, h, out=bufs[0], argmax=bufs[1], want_ant=True, ant_out=bufs[2], ant_argmax=bufs[3])
    assert alloc_counts() == n0                              # no device allocation and no host wait inside the call
    e.check()
