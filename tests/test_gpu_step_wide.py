"""The wide streaming step (prego_miniroad_step_wide / _anticipation, MiniRoadEngine.step_wide, MROAD / MROADA.step_wide; csrc/stream_wide.hip):
  1. exactly, against the saturated-gate automaton, after EVERY frame: logits, argmax, state, anticipation logits, anticipation argmax
     (ties included), for 17 .. 256 streams per call, both operand types, with the anticipation head and trunk-only;
  2. `step`'s bits on real weights: 37 streams against `step` on rows [0:16], [16:32], [32:37], three frames with the state carried - which
     carries `step`'s parity with the reference (g12 fixtures, oracle tests) over to the wide path;
  3. independence: a stream's bits depend neither on the number of streams in the call nor on its place in it;
  4. contracts: repeat calls, nullable outputs, softmax rows, argmax;
  5. the workspace: nothing written past workspace_bytes, one byte less is refused with nothing written;
  6. refusals through raw ctypes, each with its message, nothing written;
  7. no allocation and no host wait inside the call."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import _lib                                       # noqa: E402
from prego_amd import weights as W                               # noqa: E402
from prego_amd._lib import PregoError                            # noqa: E402
from prego_amd.config import anticipation_cfg, assembly101_cfg  # noqa: E402
from prego_amd.engine import MiniRoadEngine                      # noqa: E402
from tests.helpers import ant_step_cases as S                    # noqa: E402
from tests.helpers import step_wide_cases as SW                  # noqa: E402

DEV = "cuda:0"
A_KEYS = ("anticipation_layer.0.weight", "anticipation_layer.0.bias")
EINVAL = -1
_REF, _SD, _ENG = {}, {}, {}


# ---- 1. the automaton ------------------------------------------------------------------------------------------------------------------
def _ref(cid):
    """one reference per case, computed once and left unchanged; the weights stay on the device for every engine of the case"""
    if cid not in _REF:
        case, sd, n, T, feats, res = SW.reference(cid, DEV)
        assert SW.trunk_ties(res) > 0 and S.ant_ties(res) > 0, "no tie in the reference"
        _REF[cid] = (case, {k: v.to(DEV) for k, v in sd.items()}, n, T, torch.stack([r for r, _ in feats]), res)
    return _REF[cid]


EXACT = [(cid, dt, ant) for cid in SW.CASES for dt in ("bf16", "fp16") for ant in (True, False)]


@pytest.mark.parametrize("cid,dtype,ant", EXACT, ids=[f"{c}-n{SW.CASES[c][0]}-{d}-{'ant' if a else 'trunk'}" for c, d, a in EXACT])
def test_wide_equals_the_automaton(cid, dtype, ant):
    case, sd, n, T, x, res = _ref(cid)
    L, Cn = case.ant_len, case.n_classes
    e = MiniRoadEngine(case.d_rgb, case.d_flow, case.emb, case.hid, Cn, DEV, dtype)
    e.set_weights(sd)
    if ant:
        e.set_anticipation(sd[A_KEYS[0]], sd[A_KEYS[1]], L)
    h = torch.zeros((n, case.hid), device=DEV)
    want_l, want_a, want_h = (t.view(n, T, -1) for t in (res.logits, res.argmax, res.h[0]))
    want_al, want_aa = res.ant_logits.view(n, T, L, Cn), res.ant_argmax.view(n, T, L)
    for t in range(T):
        got = e.step_wide(x[:, t].contiguous(), None, h, softmax=False, want_ant=ant)
        assert len(got) == (4 if ant else 2)
        lg, am = got[0], got[1]
        assert lg.shape == (n, Cn) and am.shape == (n,) and am.dtype == torch.int32
        assert torch.equal(lg.to(torch.float64), want_l[:, t]), f"frame {t}: logits"
        assert torch.equal(am, want_a[:, t, 0]), f"frame {t}: argmax"
        assert torch.equal(h, want_h[:, t].to(torch.float32)), f"frame {t}: state"
        if ant:
            al, aa = got[2], got[3]
            assert al.shape == (n, L, Cn) and aa.shape == (n, L) and aa.dtype == torch.int32
            assert torch.equal(al.to(torch.float64), want_al[:, t]), f"frame {t}: anticipation logits"
            assert torch.equal(aa, want_aa[:, t]), f"frame {t}: anticipation argmax"
    e.check()


# ---- 2. step's bits on real weights ------------------------------------------------------------------------------------------------------
def _sd(L, no_rgb=False):
    if (L, no_rgb) not in _SD:
        cfg = anticipation_cfg(assembly101_cfg(no_rgb=no_rgb), L)
        _SD[(L, no_rgb)] = {k: torch.from_numpy(v).to(DEV) for k, v in W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0).items()}
    return _SD[(L, no_rgb)]


def _real_engine(dtype="bf16", L=3, no_rgb=False, ant=True, lib=None, hid=1024):
    """engines on real-sized weights, one per configuration for the whole module (a handle holds no state between calls)"""
    key = (dtype, L, no_rgb, ant, lib is not None, hid)
    if key not in _ENG:
        if hid == 1024:
            sd = _sd(L, no_rgb)
        else:
            cfg = anticipation_cfg(assembly101_cfg(hidden_dim=hid), L)
            sd = {k: torch.from_numpy(v).to(DEV) for k, v in W.miniroad_a_state_dict(cfg, 20).items()}
        e = MiniRoadEngine(0 if no_rgb else 2048, 2048, 2048, hid, 86, DEV, dtype, lib=lib)
        e.set_weights(sd)
        if ant:
            e.set_anticipation(sd[A_KEYS[0]], sd[A_KEYS[1]], L)
        _ENG[key] = e
    return _ENG[key]


def _feat(shape, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn(shape, device="cuda", generator=g).clamp_(min=0)


def _state(n, seed=3):
    return torch.tanh(_feat((n, 1024), seed) - 0.5)


def _step_in_groups(e, rgb, flow, h, softmax, ant):
    """what a caller has without the wide step: `step` on 16-row views; h is updated in place through the views"""
    outs = []
    for a in range(0, h.shape[0], 16):
        b = min(a + 16, h.shape[0])
        outs.append(e.step(None if rgb is None else rgb[a:b], None if flow is None else flow[a:b], h[a:b], softmax=softmax, want_ant=ant))
    return [torch.cat(ts) for ts in zip(*outs)]


# (operand type, anticipation_length, inputs, softmax, anticipation head)
VARIANTS = [("bf16", 3, "rgb+flow", True, True), ("bf16", 8, "rgb", False, True), ("fp16", 3, "rgb", True, True),
            ("fp16", 8, "rgb+flow", False, True), ("bf16", 3, "no_rgb", True, True), ("fp16", 8, "no_rgb", False, True),
            ("bf16", 3, "rgb+flow", True, False), ("fp16", 3, "rgb", False, False)]


@pytest.mark.parametrize("dtype,L,inputs,softmax,ant", VARIANTS, ids=[f"{d}-L{l}-{i}-{'probs' if s else 'logits'}-{'ant' if a else 'trunk'}" for d, l, i, s, a in VARIANTS])
def test_wide_equals_step_on_real_weights(dtype, L, inputs, softmax, ant):
    n = 37
    e = _real_engine(dtype, L, no_rgb=inputs == "no_rgb", ant=ant)
    hw, hs = _state(n), _state(n)
    for t in range(3):
        rgb = None if inputs == "no_rgb" else _feat((n, 2048), 10 + t)
        flow = None if inputs == "rgb" else _feat((n, 2048), 20 + t)
        got = e.step_wide(rgb, flow, hw, softmax=softmax, want_ant=ant)
        want = _step_in_groups(e, rgb, flow, hs, softmax, ant)
        assert len(got) == len(want) == (4 if ant else 2)
        for name, g, w in zip(("out", "argmax", "ant_out", "ant_argmax"), got, want):
            assert g.shape == w.shape and torch.equal(g, w), f"frame {t}: {name}"
        assert torch.equal(hw, hs), f"frame {t}: state"
    assert not torch.equal(hw, _state(n))
    e.check()


@pytest.mark.parametrize("n", [3, 16])
def test_up_to_16_streams_the_wide_call_is_step(n):
    """n <= 16: step's own launches (the fused LayerNorm at n = 3), no workspace"""
    e = _real_engine("bf16", 3)
    assert e.lib.prego_miniroad_step_wide_workspace_bytes(e.h, n) == 0
    rgb, flow = _feat((n, 2048), 31), _feat((n, 2048), 32)
    hw, hs = _state(n), _state(n)
    for g, w in zip(e.step_wide(rgb, flow, hw, want_ant=True), e.step(rgb, flow, hs, want_ant=True)):
        assert torch.equal(g, w)
    assert torch.equal(hw, hs)
    e.check()


# ---- 3. independence -------------------------------------------------------------------------------------------------------------------
def test_a_streams_bits_depend_on_neither_the_width_nor_the_place():
    e = _real_engine("bf16", 3)
    N, n = 144, 37
    rgb, flow, h0 = _feat((N, 2048), 41), _feat((N, 2048), 42), _state(N, 43)
    hN = h0.clone()
    big = [t.clone() for t in e.step_wide(rgb, flow, hN, want_ant=True)]
    hn = h0[:n].clone()
    small = e.step_wide(rgb[:n].contiguous(), flow[:n].contiguous(), hn, want_ant=True)
    for g, w in zip(small, big):
        assert torch.equal(g, w[:n]), "rows 0..36 of the 144-stream call"
    assert torch.equal(hn, hN[:n])
    perm = torch.randperm(N, device=DEV, generator=torch.Generator(device="cuda").manual_seed(44))
    assert not torch.equal(perm, torch.arange(N, device=DEV))
    hp = h0[perm].contiguous()
    moved = e.step_wide(rgb[perm].contiguous(), flow[perm].contiguous(), hp, want_ant=True)
    for g, w in zip(moved, big):
        assert torch.equal(g, w[perm]), "a permutation of the streams permutes every output"
    assert torch.equal(hp, hN[perm])
    e.check()


# ---- 4. / 5. contracts and the workspace, through the C ABI -------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class _Call:
    """one raw call of prego_miniroad_step_wide_anticipation on fresh poisoned buffers"""

    def __init__(self, e, n, L=3, Cn=86, hid=1024):
        self.e, self.n, self.L, self.Cn = e, n, L, Cn
        self.rgb, self.flow, self.h0 = _feat((n, 2048), 51), _feat((n, 2048), 52), torch.tanh(_feat((n, hid), 53) - 0.5)
        self.need = e.lib.prego_miniroad_step_wide_workspace_bytes(e.h, n)

    def __call__(self, want=(True, True, True, True), flags=1, ws_bytes=None, lib=None, fn="prego_miniroad_step_wide_anticipation",
                 n_streams=None, state=True):
        n, L, Cn = self.n, self.L, self.Cn
        ws_bytes = self.need if ws_bytes is None else ws_bytes
        h = self.h0.clone()
        o, a = torch.full((n, Cn), float("nan"), device=DEV), torch.full((n,), -7, dtype=torch.int32, device=DEV)
        ao, aa = torch.full((n, L, Cn), float("nan"), device=DEV), torch.full((n, L), -7, dtype=torch.int32, device=DEV)
        canary = 4096
        ws = torch.full((max(ws_bytes, 0) + canary,), 0xA5, dtype=torch.uint8, device=DEV)
        assert ws.data_ptr() % 256 == 0
        bufs = [_p(t) if w else None for t, w in zip((o, a, ao, aa), want)]
        lib = lib or self.e.lib
        ns = n if n_streams is None else n_streams
        if fn.endswith("anticipation"):
            rc = lib.prego_miniroad_step_wide_anticipation(self.e.h, ns, _p(self.rgb), _p(self.flow), _p(h) if state else None, *bufs, flags,
                                                           _p(ws), ws_bytes, None)
        else:
            rc = lib.prego_miniroad_step_wide(self.e.h, ns, _p(self.rgb), _p(self.flow), _p(h) if state else None, *bufs[:2], flags, _p(ws),
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
    e = _real_engine("bf16", 3)
    call = _Call(e, 37)
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
    res = call((True, True, False, False))                    # the head is not launched: the trunk's bits
    assert res[0] == 0 and torch.equal(res[1], full[1]) and torch.equal(res[2], full[2]) and torch.equal(res[3], full[3])
    trunk = call(fn="prego_miniroad_step_wide")
    assert trunk[0] == 0 and all(torch.equal(x, y) for x, y in zip(trunk[1:4], full[1:4]))
    err_p = float((full[2].double().sum(-1) - 1).abs().max())
    err_a = float((full[4].double().sum(-1) - 1).abs().max())
    print(f"softmax rows: |sum - 1| <= {err_p:.3e} (trunk), {err_a:.3e} (anticipation)")
    assert err_p < 1e-6 and err_a < 1e-6
    raw = call(flags=0)
    assert torch.equal(raw[5], raw[4].argmax(-1).to(torch.int32)) and torch.equal(raw[3], raw[2].argmax(-1).to(torch.int32))
    assert torch.equal(raw[5], full[5]) and torch.equal(raw[3], full[3])
    assert float((torch.softmax(raw[4], -1) - full[4]).abs().max()) < 1e-5
    e.check()


def test_workspace_exact_size_and_one_byte_less():
    e = _real_engine("bf16", 3)
    call = _Call(e, 37)
    assert call.need > 0 and call.need == e.lib.prego_miniroad_step_wide_workspace_bytes(e.h, 37)
    assert e.lib.prego_miniroad_step_wide_workspace_bytes(e.h, 144) > call.need
    assert e.lib.prego_miniroad_step_wide_workspace_bytes(e.h, 257) == 0
    ok = call()                                               # the canary behind exactly workspace_bytes is checked inside
    assert ok[0] == 0 and bool((call.ws[:call.need] != 0xA5).any())
    for short in (call.need - 1, 0):
        res = call(ws_bytes=short)
        assert res[0] == EINVAL and "workspace" in e.lib.prego_miniroad_last_error(e.h).decode()
        assert f"{call.need}" in e.lib.prego_miniroad_last_error(e.h).decode()
        assert call.untouched(res)
    h = call.h0.clone()
    rc = e.lib.prego_miniroad_step_wide(e.h, 37, _p(call.rgb), None, _p(h), None, None, 1, None, call.need, None)
    torch.cuda.synchronize()
    assert rc == EINVAL and "workspace" in e.lib.prego_miniroad_last_error(e.h).decode() and torch.equal(h, call.h0)
    e.check()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi():
    def err(e):
        return e.lib.prego_miniroad_last_error(e.h).decode()
    e = _real_engine("bf16", 3)
    call = _Call(e, 37)
    for bad in (0, 257):
        res = call(n_streams=bad)
        assert res[0] == EINVAL and f"{bad} streams (1..256 per call)" in err(e) and call.untouched(res)
    res = call(state=False)
    assert res[0] == EINVAL and "h_state is NULL" in err(e) and call.untouched(res)
    e = _real_engine("bf16", 3, ant=False)
    call = _Call(e, 37)
    res = call()
    assert res[0] == EINVAL and "step_anticipation before set_anticipation" in err(e) and call.untouched(res)
    assert call(fn="prego_miniroad_step_wide")[0] == 0       # the handle survives, and the trunk needs no set_anticipation
    e = _real_engine("fp32", 3)
    call = _Call(e, 37)
    res = call()
    assert res[0] == EINVAL and "bf16 / fp16 handles" in err(e) and call.untouched(res)
    e = _real_engine("bf16", 3, hid=512)
    call = _Call(e, 37, hid=512)
    res = call()
    assert res[0] == EINVAL and "hidden_dim 1024" in err(e) and call.untouched(res)
    e = MiniRoadEngine(2048, 2048, 2048, 1024, 86, DEV, "bf16")
    call = _Call(e, 37)
    res = call(fn="prego_miniroad_step_wide")
    assert res[0] == EINVAL and "before set_weights" in err(e) and call.untouched(res)


def test_engine_and_model_surface():
    e = _real_engine("bf16", 3, ant=False)
    with pytest.raises(PregoError, match="before set_anticipation"):
        e.step_wide(_feat((37, 2048), 6), None, torch.zeros((37, 1024), device=DEV), want_ant=True)
    with pytest.raises(PregoError, match="257 streams"):
        e.step_wide(_feat((257, 2048), 6), None, torch.zeros((257, 1024), device=DEV))
    import prego_amd.model  # noqa: F401
    from prego_amd.registry import build_model
    for L, n_out in ((0, 2), (3, 4)):
        cfg = anticipation_cfg(assembly101_cfg(), L) if L else assembly101_cfg()
        m = build_model(dict(cfg, compute_dtype="bf16"), DEV)
        m.eval()
        n = 20
        rgb, flow, hw, hs = _feat((n, 2048), 61), _feat((n, 2048), 62), _state(n), _state(n)
        got = m.step_wide(rgb, flow, hw)
        want = [torch.cat(ts) for ts in zip(m.step(rgb[:16], flow[:16], hs[:16]), m.step(rgb[16:], flow[16:], hs[16:]))]
        assert len(got) == n_out and all(torch.equal(g, w) for g, w in zip(got, want)) and torch.equal(hw, hs)
        m.check()


def test_fp32_engine_takes_the_general_forward_as_step_does():
    e = _real_engine("fp32", 3)
    n = 5
    rgb, hw, hs = _feat((n, 2048), 71), _state(n), _state(n)
    for g, w in zip(e.step_wide(rgb, None, hw, want_ant=True), e.step(rgb, None, hs, want_ant=True)):
        assert torch.equal(g, w)
    assert torch.equal(hw, hs)
    e.check()


# ---- 7. no allocation, no host wait ----------------------------------------------------------------------------------------------------
def test_step_wide_allocates_nothing_and_waits_for_nothing():
    dbg = _lib.load_debug()
    e = _real_engine("bf16", 8, lib=dbg)
    n = 144
    rgb, h = _feat((n, 2048), 8), torch.zeros((n, 1024), device=DEV)
    bufs = e.step_wide(rgb, None, h, want_ant=True)
    e.check()

    def counts():
        a, w = C.c_int64(), C.c_int64()
        assert dbg.prego_debug_alloc_count(C.byref(a), C.byref(w)) == 0
        return a.value, w.value
    n0 = counts()
    e.step_wide(rgb, None, h, out=bufs[0], argmax=bufs[1], want_ant=True, ant_out=bufs[2], ant_argmax=bufs[3])
    assert counts() == n0                                    # no device allocation and no host wait inside the call
    e.check()
