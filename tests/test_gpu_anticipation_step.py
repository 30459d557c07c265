"""MiniROADA streaming (prego_miniroad_step_anticipation / MiniRoadEngine.step(want_ant=True) / MROADA.step; csrc/stream_ant.hip):
  1. exactly, against the saturated-gate automaton: logits, argmax, anticipation logits, anticipation argmax (ties included: the first
     maximal class wins) and the state after EVERY streamed frame, with torch.equal;
  2. against the reference's own outputs (tests/golden/g12_mroada_eval_*), at the tiers and the argmax-margin rule of
     tests/test_gpu_anticipation.py;
  3. contracts: the trunk's outputs are prego_miniroad_step's bits, nullable outputs, repeat calls give the same bits, softmax rows sum to 1;
  4. refusals through raw ctypes, each with its message, nothing written;
  5. no allocation inside the call."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import _lib                                       # noqa: E402
from prego_amd import weights as W                               # noqa: E402
from prego_amd._lib import PregoError                            # noqa: E402
from prego_amd.config import anticipation_cfg, assembly101_cfg  # noqa: E402
from prego_amd.engine import MiniRoadEngine                      # noqa: E402
from tests.helpers import ant_step_cases as S                    # noqa: E402
from tests.helpers import gru_automaton as A                     # noqa: E402

DEV = "cuda:0"
G = os.path.join(os.path.dirname(__file__), "golden")
TOL = {"bf16": 1e-2, "fp16": 3e-3}
A_KEYS = ("anticipation_layer.0.weight", "anticipation_layer.0.bias")
EINVAL = -1
_REF = {}


def _ref(cid):
    """one reference per case, computed once and left unchanged; the weights stay on the device for every engine of the case"""
    if cid not in _REF:
        case, sd, T, feats, res = S.reference(cid, DEV)
        _REF[cid] = (case, {k: v.to(DEV) for k, v in sd.items()}, T, torch.stack([r for r, _ in feats]), res)
    return _REF[cid]


def _engine(case, sd, dtype, lib=None):
    e = MiniRoadEngine(case.d_rgb, case.d_flow, case.emb, case.hid, case.n_classes, DEV, dtype, lib=lib)
    e.set_weights(sd)
    e.set_anticipation(sd[A_KEYS[0]], sd[A_KEYS[1]], case.ant_len)
    return e


def _stream_equals_automaton(cid, n, dtype):
    case, sd, T, x, res = _ref(cid)
    L, Cn = case.ant_len, case.n_classes
    assert S.ant_ties(res) > 0, "no tie in the reference"
    e = _engine(case, sd, dtype)
    h = torch.zeros((n, case.hid), device=DEV)
    want_l, want_a, want_h = (t.view(16, T, -1)[:n] for t in (res.logits, res.argmax, res.h[0]))
    want_al, want_aa = res.ant_logits.view(16, T, L, Cn)[:n], res.ant_argmax.view(16, T, L)[:n]
    for t in range(T):
        lg, am, al, aa = e.step(x[:n, t].contiguous(), None, h, softmax=False, want_ant=True)
        assert lg.shape == (n, Cn) and am.shape == (n,) and al.shape == (n, L, Cn) and aa.shape == (n, L) and aa.dtype == torch.int32
        assert torch.equal(lg.to(torch.float64), want_l[:, t]), f"frame {t}: logits"
        assert torch.equal(am, want_a[:, t, 0]), f"frame {t}: argmax"
        assert torch.equal(al.to(torch.float64), want_al[:, t]), f"frame {t}: anticipation logits"
        assert torch.equal(aa, want_aa[:, t]), f"frame {t}: anticipation argmax"
        assert torch.equal(h, want_h[:, t].to(torch.float32)), f"frame {t}: state"
    e.check()


EXACT = [(cid, n, dt) for cid, c in S.CASES.items() for n in c[5] for dt in ("bf16", "fp16")]


@pytest.mark.parametrize("cid,n,dtype", EXACT, ids=[f"{c}-n{n}-{d}" for c, n, d in EXACT])
def test_streaming_equals_the_automaton(cid, n, dtype):
    """n streams fed frame by frame: three launches up to 4 streams and four above in the trunk, 16 and 8 output features per workgroup in
    the hidden product (L = 3 halves the tile), 1 / 2 / 6 class tiles in the head"""
    _stream_equals_automaton(cid, n, dtype)


def test_fp32_engine_streams_through_the_general_forward():
    _stream_equals_automaton("L4-C12", 3, "fp32")


# ---- 2. the reference's outputs ------------------------------------------------------------------------------------------------------
def _model(cfg, sd, dtype):
    import prego_amd.model  # noqa: F401
    from prego_amd.registry import build_model
    m = build_model(dict(cfg, compute_dtype=dtype), DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.eval()
    return m


FIX = [(t, 1024, l, d) for t in ("plain", "peaky") for l in (1, 4, 8) for d in ("bf16", "fp16")] + \
      [(t, 512, 8, "bf16") for t in ("plain", "peaky")]


@pytest.mark.parametrize("tag,H,L,dtype", FIX, ids=[f"{t}-h{h}-L{l}-{d}" for t, h, l, d in FIX])
def test_fixture_parity_streamed(tag, H, L, dtype):
    """the 256 frames of the g12 fixtures, one stream, one frame per call (hidden_dim 512: the general forward)"""
    g = np.load(os.path.join(G, f"g12_mroada_eval_{tag}_h{H}_L{L}.npz"))
    cfg = anticipation_cfg(assembly101_cfg(hidden_dim=H), L)
    sd = W.miniroad_a_state_dict(cfg, 20, head_gain=float(g["head_gain"]), ant_gain=float(g["ant_gain"]))
    m = _model(cfg, sd, dtype)
    rgb = torch.from_numpy(W.tsn_features((1, 256, 2048), 20, "g12.rgb")).cuda()[0]
    h = torch.zeros((1, H), device=DEV)
    ps, ants, aargs = [], [], []
    for t in range(256):
        p, _, a, aa = m.step(rgb[t:t + 1], None, h)
        ps.append(p.clone()); ants.append(a.clone()); aargs.append(aa.clone())
    m.check()
    p, a, aa = torch.cat(ps).cpu().numpy(), torch.cat(ants).cpu().numpy(), torch.cat(aargs).cpu().numpy()
    assert p.shape == (256, 86) and a.shape == (256, L, 86) and aa.shape == (256, L)
    tol = TOL[dtype]
    err_p = float(np.abs(p - g["probs"]).max())
    err_a = float(np.abs(a[g["sample_idx"]] - g["ant_sample"]).max())
    print(f"{tag} h{H} L{L} {dtype}: max |dprob| {err_p:.3e}, anticipation {err_a:.3e} (tier {tol})")
    assert err_p < tol
    assert err_a < tol
    mism = a.argmax(-1) != g["ant_argmax"]
    assert not np.any(mism & (g["ant_margin"] > 2 * tol)), f"anticipation argmax differs on {int(np.sum(mism & (g['ant_margin'] > 2 * tol)))} pairs"
    assert np.array_equal(aa, a.argmax(-1))


# ---- 3. contracts --------------------------------------------------------------------------------------------------------------------
def _real_engine(dtype="bf16", L=4, lib=None, hid=1024, ant=True):
    cfg = anticipation_cfg(assembly101_cfg(hidden_dim=hid), L)
    sd = {k: torch.from_numpy(v).to(DEV) for k, v in W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0).items()}
    e = MiniRoadEngine(2048, 2048, 2048, hid, 86, DEV, dtype, lib=lib)
    e.set_weights(sd)
    if ant:
        e.set_anticipation(sd[A_KEYS[0]], sd[A_KEYS[1]], L)
    return e


def _feat(shape, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn(shape, device="cuda", generator=g).clamp_(min=0)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def test_trunk_bits_nullable_outputs_and_repeatability():
    n, L, Cn = 5, 4, 86
    e = _real_engine(L=L)
    lib = e.lib
    rgb, flow = _feat((n, 2048), 1), _feat((n, 2048), 2)
    h0 = torch.tanh(_feat((n, 1024), 3) - 0.5)

    def plain():
        h, o, a = h0.clone(), torch.empty((n, Cn), device=DEV), torch.empty((n,), dtype=torch.int32, device=DEV)
        assert lib.prego_miniroad_step(e.h, n, _p(rgb), _p(flow), _p(h), _p(o), _p(a), 1, None) == 0
        return h, o, a

    def ant(want_out=True, want_arg=True, flags=1):
        h, o, a = h0.clone(), torch.empty((n, Cn), device=DEV), torch.empty((n,), dtype=torch.int32, device=DEV)
        ao = torch.full((n, L, Cn), float("nan"), device=DEV)
        aa = torch.full((n, L), -7, dtype=torch.int32, device=DEV)
        assert lib.prego_miniroad_step_anticipation(e.h, n, _p(rgb), _p(flow), _p(h), _p(o), _p(a), _p(ao) if want_out else None,
                                                    _p(aa) if want_arg else None, flags, None) == 0
        return h, o, a, ao, aa
    ref = plain()
    e.check()
    full = ant()
    for x, y in zip(ref, ant(False, False)[:3]):
        assert torch.equal(x, y), "both anticipation outputs NULL: the trunk's bits"
    for x, y in zip(ref, full[:3]):
        assert torch.equal(x, y), "anticipation outputs set: the trunk's bits"
    assert not torch.isnan(full[3]).any() and int(full[4].min()) >= 0 and int(full[4].max()) < Cn
    only_out, only_arg = ant(True, False), ant(False, True)
    assert torch.equal(only_out[3], full[3]) and bool((only_out[4] == -7).all())
    assert torch.equal(only_arg[4], full[4]) and bool(torch.isnan(only_arg[3]).all())
    again = ant()
    for x, y in zip(full, again):
        assert torch.equal(x, y), "two identical calls"
    assert float((full[3].sum(-1) - 1).abs().max()) < 1e-4 and float((full[1].sum(-1) - 1).abs().max()) < 1e-4
    assert torch.equal(full[4], A.first_argmax(full[3])) and torch.equal(full[2], A.first_argmax(full[1]))
    raw = ant(flags=0)                                       # logits: their softmax is the probabilities
    assert float((torch.softmax(raw[3], -1) - full[3]).abs().max()) < 1e-5
    e.check()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------
def _err(lib, h):
    return lib.prego_miniroad_last_error(h).decode()


def test_refusals_through_the_c_abi():
    lib = _lib.load()
    n, L, Cn = 2, 4, 86
    rgb = _feat((17, 2048), 5)

    def call(e, n_streams=n, hid=1024, state=True):
        h = torch.full((17, hid), 0.25, device=DEV)
        o = torch.full((17, Cn), float("nan"), device=DEV)
        a = torch.full((17,), -7, dtype=torch.int32, device=DEV)
        ao = torch.full((17, L, Cn), float("nan"), device=DEV)
        aa = torch.full((17, L), -7, dtype=torch.int32, device=DEV)
        rc = lib.prego_miniroad_step_anticipation(e.h, n_streams, _p(rgb), None, _p(h) if state else None, _p(o), _p(a), _p(ao), _p(aa), 1, None)
        torch.cuda.synchronize()
        # nothing was launched: no output and no state element has changed
        assert bool(torch.isnan(o).all()) and bool(torch.isnan(ao).all()) and bool((a == -7).all()) and bool((aa == -7).all())
        assert bool((h == 0.25).all())
        return rc, _err(lib, e.h)
    e = _real_engine(L=L, ant=False)
    rc, msg = call(e)
    assert rc == EINVAL and "step_anticipation before set_anticipation" in msg
    e = _real_engine(L=L)
    for bad in (0, 17):
        rc, msg = call(e, n_streams=bad)
        assert rc == EINVAL and f"{bad} streams" in msg
    rc, msg = call(e, state=False)
    assert rc == EINVAL and "h_state is NULL" in msg
    # the handle survives: a valid call works
    h = torch.zeros((n, 1024), device=DEV)
    out = e.step(rgb[:n].contiguous(), None, h, want_ant=True)
    e.check()
    assert not torch.isnan(out[2]).any()
    rc, msg = call(_real_engine("fp32", L=L))
    assert rc == EINVAL and "bf16 / fp16 handles" in msg
    rc, msg = call(_real_engine(L=L, hid=512), hid=512)
    assert rc == EINVAL and "hidden_dim 1024" in msg


def test_model_refuses_17_streams_and_engine_refuses_before_set_anticipation():
    cfg = anticipation_cfg(assembly101_cfg(), 4)
    m = _model(cfg, W.miniroad_a_state_dict(cfg, 20), "bf16")
    with pytest.raises(PregoError, match="17 streams"):
        m.step(_feat((17, 2048), 6), None, torch.zeros((17, 1024), device=DEV))
    out = m.step(_feat((16, 2048), 6), None, torch.zeros((16, 1024), device=DEV))
    m.check()
    assert out[2].shape == (16, 4, 86) and out[3].shape == (16, 4)
    e = _real_engine(ant=False)
    with pytest.raises(PregoError, match="before set_anticipation"):
        e.step(_feat((1, 2048), 6), None, torch.zeros((1, 1024), device=DEV), want_ant=True)


# ---- 5. no allocation ------------------------------------------------------------------------------------------------------------------
def test_step_anticipation_allocates_nothing():
    dbg = _lib.load_debug()
    e = _real_engine(L=8, lib=dbg)
    n = 4
    rgb, h = _feat((n, 2048), 8), torch.zeros((n, 1024), device=DEV)
    bufs = e.step(rgb, None, h, want_ant=True)
    e.check()

    def counts():
        a, w = C.c_int64(), C.c_int64()
        assert dbg.prego_debug_alloc_count(C.byref(a), C.byref(w)) == 0
        return a.value, w.value
    n0 = counts()
    e.step(rgb, None, h, out=bufs[0], argmax=bufs[1], want_ant=True, ant_out=bufs[2], ant_argmax=bufs[3])
    assert counts() == n0                                    # no device allocation and no host wait inside the call
    e.check()
