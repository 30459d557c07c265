"""The multi-frame streaming step (prego_miniroad_step_frames / _anticipation, MiniRoadEngine.step_frames, MROAD / MROADA.step_frames;
csrc/stream_frames.hip):
  1. exactly, against the saturated-gate automaton, after EVERY burst: logits, argmax (ties included), the state, anticipation logits and
     argmax, for the shapes of tests/helpers/step_frames_cases.py, both operand types, with the anticipation head and trunk-only;
  2. `step_wide`'s bits on real weights: every frame of two consecutive bursts against `step_wide` driven frame by frame with the state
     carried (n = 3 against calls in which the three streams ride with two filler rows: the unfused LayerNorm route);
  3. contracts: nullable outputs, repeat calls with reused buffers, softmax rows;
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
from tests import test_gpu_step_wide as TW                       # noqa: E402  its references and engines are computed once and shared
from tests.helpers import ant_step_cases as S                    # noqa: E402
from tests.helpers import step_frames_cases as SF                # noqa: E402
from tests.helpers import step_wide_cases as SW                  # noqa: E402

DEV = "cuda:0"
EINVAL = -1
_REF = {}


# ---- 1. the automaton ------------------------------------------------------------------------------------------------------------------
def _ref(src, cid):
    """(case, sd on the device, streams, frames, features [n, T, d], Result): one reference per case, computed once and left unchanged"""
    if src == "wide":
        return TW._ref(cid)
    if cid not in _REF:
        case, sd, T, feats, res = S.reference(cid, DEV)
        assert SW.trunk_ties(res) > 0 and S.ant_ties(res) > 0, "no tie in the reference"
        _REF[cid] = (case, {k: v.to(DEV) for k, v in sd.items()}, S.N_STREAMS, T, torch.stack([r for r, _ in feats]), res)
    return _REF[cid]


EXACT = [(sid, dt, ant) for sid in SF.SHAPES for dt in ("bf16", "fp16") for ant in (True, False)]


@pytest.mark.parametrize("sid,dtype,ant", EXACT, ids=[f"{s}-{d}-{'ant' if a else 'trunk'}" for s, d, a in EXACT])
def test_bursts_equal_the_automaton(sid, dtype, ant):
    src, cid, n, bursts = SF.SHAPES[sid]
    case, sd, n_ref, T, x, res = _ref(src, cid)
    assert n <= n_ref and sum(bursts) <= T
    L, Cn = case.ant_len, case.n_classes
    e = MiniRoadEngine(case.d_rgb, case.d_flow, case.emb, case.hid, Cn, DEV, dtype)
    e.set_weights(sd)
    if ant:
        e.set_anticipation(sd[TW.A_KEYS[0]], sd[TW.A_KEYS[1]], L)
    h = torch.zeros((n, case.hid), device=DEV)
    want_l, want_a, want_h = (t.view(n_ref, T, -1)[:n] for t in (res.logits, res.argmax, res.h[0]))
    want_al, want_aa = res.ant_logits.view(n_ref, T, L, Cn)[:n], res.ant_argmax.view(n_ref, T, L)[:n]
    at = 0
    for K in bursts:
        got = e.step_frames(x[:n, at:at + K].contiguous(), None, h, softmax=False, want_ant=ant)
        assert len(got) == (4 if ant else 2)
        lg, am = got[0], got[1]
        assert lg.shape == (n, K, Cn) and am.shape == (n, K) and am.dtype == torch.int32
        assert torch.equal(lg.to(torch.float64), want_l[:, at:at + K]), f"frames {at}..: logits"
        assert torch.equal(am, want_a[:, at:at + K, 0]), f"frames {at}..: argmax"
        assert torch.equal(h, want_h[:, at + K - 1].to(torch.float32)), f"frames {at}..: state"
        if ant:
            al, aa = got[2], got[3]
            assert al.shape == (n, K, L, Cn) and aa.shape == (n, K, L) and aa.dtype == torch.int32
            assert torch.equal(al.to(torch.float64), want_al[:, at:at + K]), f"frames {at}..: anticipation logits"
            assert torch.equal(aa, want_aa[:, at:at + K]), f"frames {at}..: anticipation argmax"
        at += K
    e.check()


# ---- 2. step_wide's bits on real weights ------------------------------------------------------------------------------------------------
def _wide_frame_by_frame(e, rgb, flow, h, softmax, ant, fill=0):
    """step_wide on frame t of every stream, t = 0 .. K - 1, the state carried in h [n + fill, H]; rgb / flow [n + fill, K, d].  Returns the
    outputs stacked on a K axis and the state after every frame"""
    K = (rgb if rgb is not None else flow).shape[1]
    outs, states = [], []
    for t in range(K):
        o = e.step_wide(None if rgb is None else rgb[:, t].contiguous(), None if flow is None else flow[:, t].contiguous(), h,
                        softmax=softmax, want_ant=ant)
        outs.append([v.clone() for v in o])
        states.append(h.clone())
    return [torch.stack(ts, dim=1) for ts in zip(*outs)], states


BITS = [(n, K, fill) + v for (n, K, fill) in ((5, 3, 0), (37, 6, 0), (3, 5, 2)) for v in TW.VARIANTS]


@pytest.mark.parametrize("n,K,fill,dtype,L,inputs,softmax,ant", BITS,
                         ids=[f"n{n}-K{K}-{d}-L{l}-{i}-{'probs' if s else 'logits'}-{'ant' if a else 'trunk'}" for n, K, f, d, l, i, s, a in BITS])
def test_every_frame_has_step_wides_bits_on_real_weights(n, K, fill, dtype, L, inputs, softmax, ant):
    e = TW._real_engine(dtype, L, no_rgb=inputs == "no_rgb", ant=ant)
    hw = TW._state(n + fill)                                  # the filler rows ride along in step_wide only: 5 rows, the unfused route
    hf = hw[:n].clone()
    for burst in range(2):                                    # the second burst starts from the state the first one left
        rgb = None if inputs == "no_rgb" else TW._feat((n + fill, K, 2048), 10 + burst)
        flow = None if inputs == "rgb" else TW._feat((n + fill, K, 2048), 20 + burst)
        want, states = _wide_frame_by_frame(e, rgb, flow, hw, softmax, ant, fill)
        got = e.step_frames(None if rgb is None else rgb[:n].contiguous(), None if flow is None else flow[:n].contiguous(), hf,
                            softmax=softmax, want_ant=ant)
        assert len(got) == len(want) == (4 if ant else 2)
        for name, g, w in zip(("out", "argmax", "ant_out", "ant_argmax"), got, want):
            assert g.shape == w[:n].shape and torch.equal(g, w[:n]), f"burst {burst}: {name}"
        assert torch.equal(hf, hw[:n]), f"burst {burst}: state"
        # the state after EVERY frame: a burst cut short at frame t leaves step_wide's state of frame t
        for t in (0, K // 2):
            hc = (TW._state(n + fill)[:n] if burst == 0 else prev).clone()
            e.step_frames(None if rgb is None else rgb[:n, :t + 1].contiguous(), None if flow is None else flow[:n, :t + 1].contiguous(), hc,
                          softmax=softmax, want_ant=False)
            assert torch.equal(hc, states[t][:n]), f"burst {burst}: state after frame {t}"
        prev = hf.clone()
    assert not torch.equal(hf, TW._state(n + fill)[:n])
    e.check()


# ---- 3. / 4. contracts and the workspace, through the C ABI ---------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class _Call:
    """one raw call of prego_miniroad_step_frames_anticipation on fresh poisoned buffers"""

    def __init__(self, e, n, K, L=3, Cn=86, hid=1024):
        self.e, self.n, self.K, self.L, self.Cn = e, n, K, L, Cn
        self.rgb, self.flow, self.h0 = TW._feat((n, K, 2048), 51), TW._feat((n, K, 2048), 52), torch.tanh(TW._feat((n, hid), 53) - 0.5)
        self.need = e.lib.prego_miniroad_step_frames_workspace_bytes(e.h, n, K)

    def __call__(self, want=(True, True, True, True), flags=1, ws_bytes=None, fn="prego_miniroad_step_frames_anticipation", n_streams=None,
                 n_frames=None, state=True, ws_null=False, ws_off=0):
        n, K, L, Cn = self.n, self.K, self.L, self.Cn
        ws_bytes = self.need if ws_bytes is None else ws_bytes
        h = self.h0.clone()
        o, a = torch.full((n, K, Cn), float("nan"), device=DEV), torch.full((n, K), -7, dtype=torch.int32, device=DEV)
        ao, aa = torch.full((n, K, L, Cn), float("nan"), device=DEV), torch.full((n, K, L), -7, dtype=torch.int32, device=DEV)
        canary = 4096
        ws = torch.full((max(ws_bytes, 0) + canary,), 0xA5, dtype=torch.uint8, device=DEV)
        assert ws.data_ptr() % 256 == 0
        bufs = [_p(t) if w else None for t, w in zip((o, a, ao, aa), want)]
        lib = self.e.lib
        ns, nf = n if n_streams is None else n_streams, K if n_frames is None else n_frames
        wp = None if ws_null else C.c_void_p(ws.data_ptr() + ws_off)
        if fn.endswith("anticipation"):
            rc = lib.prego_miniroad_step_frames_anticipation(self.e.h, ns, nf, _p(self.rgb), _p(self.flow), _p(h) if state else None, *bufs,
                                                             flags, wp, ws_bytes, None)
        else:
            rc = lib.prego_miniroad_step_frames(self.e.h, ns, nf, _p(self.rgb), _p(self.flow), _p(h) if state else None, *bufs[:2], flags, wp,
                                                ws_bytes, None)
        torch.cuda.synchronize()
        assert bool((ws[max(ws_bytes, 0):] == 0xA5).all()), "written past workspace_bytes"
        self.ws = ws
        return rc, h, o, a, ao, aa

    def untouched(self, res):
        rc, h, o, a, ao, aa = res
        return (torch.equal(h, self.h0) and bool(torch.isnan(o).all()) and bool(torch.isnan(ao).all()) and bool((a == -7).all())
                and bool((aa == -7).all()) and bool((self.ws == 0xA5).all()))


def test_repeat_calls_nullable_outputs_softmax_rows_and_argmax():
    e = TW._real_engine("bf16", 3)
    call = _Call(e, 7, 5)
    full = call()
    assert full[0] == 0 and not torch.equal(full[1], call.h0)
    for t in full[2:]:
        assert not (torch.isnan(t).any() if t.is_floating_point() else (t == -7).any())
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
    trunk = call(fn="prego_miniroad_step_frames")
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
    n, K = 6, 4
    rgb, h1, h2 = TW._feat((n, K, 2048), 81), TW._state(n), TW._state(n)
    first = [t.clone() for t in e.step_frames(rgb, None, h1)]
    bufs = [torch.empty_like(t) for t in first]
    got = e.step_frames(rgb, None, h2, out=bufs[0], argmax=bufs[1], ant_out=bufs[2], ant_argmax=bufs[3])
    assert all(g is b for g, b in zip(got, bufs)) and all(torch.equal(g, f) for g, f in zip(got, first)) and torch.equal(h1, h2)
    e.check()


def test_workspace_exact_size_and_one_byte_less():
    e = TW._real_engine("bf16", 3)
    lib = e.lib
    call = _Call(e, 7, 5)
    assert call.need > 0 and lib.prego_miniroad_step_frames_workspace_bytes(e.h, 7, 6) > call.need
    for n, K in ((0, 1), (1, 0), (1, 33), (257, 1), (129, 2), (9, 32)):
        assert lib.prego_miniroad_step_frames_workspace_bytes(e.h, n, K) == 0, (n, K)
    assert lib.prego_miniroad_step_frames_workspace_bytes(e.h, 8, 32) > 0 and lib.prego_miniroad_step_frames_workspace_bytes(e.h, 256, 1) > 0
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
    call = _Call(e, 5, 3)
    for kw, msg in ((dict(n_frames=0), "0 frames per stream (1..32 per call)"), (dict(n_frames=33), "33 frames per stream (1..32 per call)"),
                    (dict(n_streams=257, n_frames=1), "257 streams x 1 frames = 257 rows (at most 256 per call"),
                    (dict(n_streams=129, n_frames=2), "= 258 rows (at most 256 per call"),
                    (dict(n_streams=0), "0 streams (1..256 per call)"), (dict(state=False), "h_state is NULL"),
                    (dict(ws_null=True), "workspace"), (dict(ws_off=16), "256-byte aligned")):
        for fn in ("prego_miniroad_step_frames_anticipation", "prego_miniroad_step_frames"):
            res = call(fn=fn, **kw)
            assert res[0] == EINVAL and msg in err(e), (kw, err(e))
            assert call.untouched(res), kw
    assert call()[0] == 0                                     # the handle survives
    e = TW._real_engine("bf16", 3, ant=False)
    call = _Call(e, 5, 3)
    res = call()
    assert res[0] == EINVAL and "step_anticipation before set_anticipation" in err(e) and call.untouched(res)
    assert call(fn="prego_miniroad_step_frames")[0] == 0      # the trunk needs no set_anticipation
    e = TW._real_engine("fp32", 3)
    call = _Call(e, 5, 3)
    res = call()
    assert res[0] == EINVAL and "bf16 / fp16 handles" in err(e) and call.untouched(res)
    e = TW._real_engine("bf16", 3, hid=512)
    call = _Call(e, 5, 3, hid=512)
    res = call()
    assert res[0] == EINVAL and "hidden_dim 1024" in err(e) and call.untouched(res)
    e = MiniRoadEngine(2048, 2048, 2048, 1024, 86, DEV, "bf16")
    call = _Call(e, 5, 3)
    res = call(fn="prego_miniroad_step_frames")
    assert res[0] == EINVAL and "before set_weights" in err(e) and call.untouched(res)


def test_engine_and_model_surface():
    e = TW._real_engine("bf16", 3, ant=False)
    with pytest.raises(PregoError, match="before set_anticipation"):
        e.step_frames(TW._feat((5, 3, 2048), 6), None, torch.zeros((5, 1024), device=DEV), want_ant=True)
    with pytest.raises(PregoError, match="33 frames"):
        e.step_frames(TW._feat((2, 33, 2048), 6), None, torch.zeros((2, 1024), device=DEV))
    with pytest.raises(PregoError, match="258 rows"):
        e.step_frames(TW._feat((129, 2, 2048), 6), None, torch.zeros((129, 1024), device=DEV))
    with pytest.raises(PregoError, match=r"expected frames as \[n, K, d\]"):
        e.step_frames(TW._feat((5, 2048), 6), None, torch.zeros((5, 1024), device=DEV))
    for eng in (TW._real_engine("fp32", 3), TW._real_engine("bf16", 3, hid=512)):
        with pytest.raises(PregoError, match="the streaming kernels are built for"):
            eng.step_frames(TW._feat((5, 3, 2048), 6), None, torch.zeros((5, eng.dims[3]), device=DEV))
    import prego_amd.model  # noqa: F401
    from prego_amd.registry import build_model
    for L, n_out in ((0, 2), (3, 4)):
        cfg = anticipation_cfg(assembly101_cfg(), L) if L else assembly101_cfg()
        m = build_model(dict(cfg, compute_dtype="bf16"), DEV)
        m.eval()
        n, K = 6, 3
        rgb, flow, hf, hs = TW._feat((n, K, 2048), 61), TW._feat((n, K, 2048), 62), TW._state(n), TW._state(n)
        got = m.step_frames(rgb, flow, hf)
        want = [torch.stack(ts, dim=1) for ts in zip(*[m.step_wide(rgb[:, t].contiguous(), flow[:, t].contiguous(), hs) for t in range(K)])]
        assert len(got) == n_out and all(torch.equal(g, w) for g, w in zip(got, want)) and torch.equal(hf, hs)
        m.check()


# ---- 6. no allocation, no host wait ----------------------------------------------------------------------------------------------------
def test_step_frames_allocates_nothing_and_waits_for_nothing():
    dbg = _lib.load_debug()
    e = TW._real_engine("bf16", 8, lib=dbg)
    n, K = 16, 8
    rgb, h = TW._feat((n, K, 2048), 8), torch.zeros((n, 1024), device=DEV)
    bufs = e.step_frames(rgb, None, h, want_ant=True)
    e.check()

    def counts():
        a, w = C.c_int64(), C.c_int64()
        assert dbg.prego_debug_alloc_count(C.byref(a), C.byref(w)) == 0
        return a.value, w.value
    n0 = counts()
    e.step_frames(rgb, None, h, out=bufs[0], argmax=bufs[1], want_ant=True, ant_out=bufs[2], ant_argmax=bufs[3])
    assert counts() == n0                                    # no device allocation and no host wait inside the call
    e.check()
