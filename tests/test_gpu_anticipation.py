"""GPU tests of MiniROADA inference (model/rnn/rnn.py:113-136): the fused anticipation head (csrc/ant_head.hip) through
prego_miniroad_forward_anticipation, against the reference's outputs (tests/golden/g12_*), and its contracts: MROAD's logits untouched,
the same bits whichever pass ran, h0 / h_last chaining, no allocation inside the call, refusals with a message.
Tolerance tiers and the argmax-margin rule are those of tests/test_gpu_miniroad.py."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from prego_amd import weights as W                               # noqa: E402
from prego_amd._lib import PregoError                            # noqa: E402
from prego_amd.config import anticipation_cfg, assembly101_cfg  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
TOL = {"bf16": 1e-2, "fp16": 3e-3, "fp32": 1e-3}


def _with_env(name, value, fn):
    old = os.environ.get(name)
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value
    try:
        return fn()
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def _model(cfg, sd, dtype, split=None):
    import prego_amd.model  # noqa: F401
    from prego_amd.registry import build_model
    m = build_model(dict(cfg, compute_dtype=dtype), "cuda:0")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.eval()
    _with_env("PREGO_SPLIT_PASS", split, m.engine)
    return m


def _check_ant(got, ref_sample, idx, ref_argmax, ref_margin, dtype, exact, what):
    tol = TOL[dtype]
    err = float(np.abs(got[idx] - ref_sample).max())
    assert err < tol, f"{what}: max |dprob| {err:.3e} >= {tol}"
    mism = got.argmax(-1) != ref_argmax
    safe = np.ones_like(mism) if exact else ref_margin > (1e-5 if dtype == "fp32" else 2 * tol)
    assert not np.any(mism & safe), f"{what}: anticipation argmax differs on {int(np.sum(mism & safe))} (frame, step) pairs"
    return err


CASES = [(t, h, l) for t in ("plain", "peaky") for h, l in ((1024, 1), (1024, 4), (1024, 8), (512, 8))]


@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("tag,H,L", CASES)
def test_fixture_parity(dtype, tag, H, L):
    g = np.load(os.path.join(G, f"g12_mroada_eval_{tag}_h{H}_L{L}.npz"))
    cfg = anticipation_cfg(assembly101_cfg(hidden_dim=H), L)
    sd = W.miniroad_a_state_dict(cfg, 20, head_gain=float(g["head_gain"]), ant_gain=float(g["ant_gain"]))
    m = _model(cfg, sd, dtype)
    rgb = torch.from_numpy(W.tsn_features((1, 256, 2048), 20, "g12.rgb")).cuda()
    with torch.no_grad():
        o = m(rgb, torch.zeros_like(rgb))
    m.check()
    p, a = o["logits"][0].cpu().numpy(), o["anticipation_logits"][0].cpu().numpy()
    assert p.shape == (256, 86) and a.shape == (256, L, 86)
    assert float(np.abs(p - g["probs"]).max()) < TOL[dtype]
    # fp32 is held to the reference's argmax on EVERY (frame, step) of the peaky fixtures.  The plain fixtures (random-init weights)
    # have top-1 / top-2 margins down to 9e-9, below fp32's own rounding of a 1 024-term dot product (~1e-7 relative): no fp32
    # implementation that sums in another order than torch's CPU GEMM can be held to them, so there the margin rule applies (1e-5)
    exact = dtype == "fp32" and tag == "peaky"
    _check_ant(a, g["ant_sample"], g["sample_idx"], g["ant_argmax"], g["ant_margin"], dtype, exact, f"{tag} h{H} L{L} {dtype}")
    # the ragged path with argmax outputs: the same numbers, argmax of the probabilities (first max)
    outs, args, _, ants, aargs = m.forward_clips([rgb[0]], None, want_ant=True)
    m.check()
    assert torch.equal(ants[0], o["anticipation_logits"][0]) and torch.equal(outs[0], o["logits"][0])
    assert np.array_equal(aargs[0].cpu().numpy(), ants[0].cpu().numpy().argmax(-1))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_long_clip_sampled_frames(dtype):
    g = np.load(os.path.join(G, "g12_mroada_longT_4096.npz"))
    cfg = anticipation_cfg(assembly101_cfg(), 8)
    sd = W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0)
    m = _model(cfg, sd, dtype)
    rgb = torch.from_numpy(W.tsn_features((4096, 2048), 20, "g12.rgb.4096")[None]).cuda()
    _, _, _, ants, _ = m.forward_clips([rgb[0]], None, want_ant=True)
    m.check()
    _check_ant(ants[0].cpu().numpy(), g["ant_sample"], g["sample_idx"], g["ant_argmax"], g["ant_margin"], dtype, False, f"longT {dtype}")


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_logits_equal_miniroad_bit_for_bit(dtype):
    cfg = anticipation_cfg(assembly101_cfg(), 4)
    sd = W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0)
    ma = _model(cfg, sd, dtype)
    trunk = {k: v for k, v in sd.items() if not k.startswith("anticipation_layer")}
    m0 = _model(assembly101_cfg(), trunk, dtype)
    rgb = [torch.from_numpy(W.tsn_features((T, 2048), 7, f"ant.{T}")).cuda() for T in (300, 17, 1000)]
    o0, a0, _ = m0.forward_clips(rgb)
    o1, a1, _, _, _ = ma.forward_clips(rgb, want_ant=True)
    m0.check(); ma.check()
    for x, y in zip(o0 + a0, o1 + a1):
        assert torch.equal(x, y)


def _feat(shape, seed, dtype=torch.float32):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn(shape, device="cuda", generator=g).clamp_(min=0).to(dtype)


def test_pass_independence_split_chunked_resident_repeat():
    """the same bits from the split pass, the chunked pass with the once-per-pass head (resident buffer) and the chunked pass with the
    per-chunk head (no resident buffer), and across repeated calls: a ragged batch of 64 clips, >= 262 144 frames"""
    cfg = anticipation_cfg(assembly101_cfg(), 4)
    sd = W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0)
    g = torch.Generator().manual_seed(5)
    lens = [int(x) for x in torch.randint(3900, 4400, (64,), generator=g)]
    assert sum(lens) >= 262144
    rgb = [_feat((T, 2048), 300 + i, torch.float16) for i, T in enumerate(lens)]

    def run(m):
        r = m.forward_clips(rgb, want_ant=True)
        m.check()
        return r, m.engine().pass_info()
    ms = _model(cfg, sd, "fp16", "3")
    run(ms)                                         # placement (the handle's first call is chunked)
    (o_s, a_s, _, ant_s, aa_s), info = run(ms)
    assert info["mode"] == 3, info
    (o_s2, _, _, ant_s2, aa_s2), info = run(ms)
    assert info["mode"] == 3
    mc = _model(cfg, sd, "fp16", "0")
    (o_c, a_c, _, ant_c, aa_c), info = run(mc)
    assert info["mode"] == 0 and mc.engine()._res is not None
    eng = mc.engine()
    assert eng.lib.prego_miniroad_set_resident(eng.h, None, 0) == 0
    eng._res = torch.empty(1 << 40, dtype=torch.uint8, device="meta")        # the engine must not register a buffer again
    lens_arr = (C.c_int32 * len(lens))(*lens)
    need = eng.lib.prego_miniroad_resident_bytes(eng.h, len(lens), lens_arr, 1 | 4)
    assert need > 0 and sum(lens) >= 4 * eng.rows_per_chunk          # the run above took the once-per-pass head (resident buffer)
    (o_p, _, _, ant_p, aa_p), info = run(mc)
    assert info["mode"] == 0
    for i in range(len(lens)):
        for other in (ant_s2, ant_c, ant_p):
            assert torch.equal(ant_s[i], other[i]), i
        for other in (aa_s2, aa_c, aa_p):
            assert torch.equal(aa_s[i], other[i]), i
        for other in (o_s2, o_c, o_p):
            assert torch.equal(o_s[i], other[i]), i
    # MROADA's logits in the split pass equal MROAD's split pass (the classifier launch there is behind the anticipation change)
    trunk = {k: v for k, v in sd.items() if not k.startswith("anticipation_layer")}
    m0 = _model(assembly101_cfg(), trunk, "fp16", "3")
    m0.forward_clips(rgb)
    o0, a0, _ = m0.forward_clips(rgb)
    m0.check()
    assert m0.engine().pass_info()["mode"] == 3
    for i in range(len(lens)):
        assert torch.equal(o0[i], o_s[i]) and torch.equal(a0[i], a_s[i]), i


def test_h0_h_last_chaining_equals_one_call():
    cfg = anticipation_cfg(assembly101_cfg(), 8)
    sd = W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0)
    m = _model(cfg, sd, "fp32")
    eng = m.engine()
    rgb = [_feat((T, 2048), 40 + i) for i, T in enumerate((700, 333, 96))]
    _, _, hl, ant, _ = eng.forward_ragged(rgb, None, want_h_last=True, want_ant=True)
    cut = [250, 100, 50]
    _, _, h1, ant1, _ = eng.forward_ragged([r[:c] for r, c in zip(rgb, cut)], None, want_h_last=True, want_ant=True)
    _, _, h2, ant2, _ = eng.forward_ragged([r[c:] for r, c in zip(rgb, cut)], None, h0=h1, want_h_last=True, want_ant=True)
    eng.check()
    for i in range(3):
        assert torch.allclose(torch.cat([ant1[i], ant2[i]]), ant[i], rtol=0, atol=1e-5)
    assert torch.allclose(h2, hl, rtol=0, atol=1e-5)


def test_forward_anticipation_allocates_nothing():
    from prego_amd import _lib
    from prego_amd.engine import MiniRoadEngine
    dbg = _lib.load_debug()
    cfg = anticipation_cfg(assembly101_cfg(), 8)
    sd = {k: torch.from_numpy(v) for k, v in W.miniroad_a_state_dict(cfg, 20).items()}
    eng = MiniRoadEngine(2048, 2048, 2048, 1024, 86, "cuda:0", "bf16", lib=dbg)
    eng.set_weights(sd)
    eng.set_anticipation(sd["anticipation_layer.0.weight"], sd["anticipation_layer.0.bias"], 8)
    rgb = [_feat((T, 2048), 70 + i) for i, T in enumerate((900, 64, 333))]
    eng.forward_ragged(rgb, None, want_ant=True)
    eng.check()

    def counts():
        a, w = C.c_int64(), C.c_int64()
        assert dbg.prego_debug_alloc_count(C.byref(a), C.byref(w)) == 0
        return a.value
    n0 = counts()
    eng.forward_ragged(rgb, None, want_ant=True)
    eng.check()
    assert counts() == n0


def test_refusals():
    from prego_amd import _lib
    from prego_amd.engine import MiniRoadEngine
    w = torch.zeros((4 * 1024, 1024), device="cuda")
    b = torch.zeros((4 * 1024,), device="cuda")
    e = MiniRoadEngine(2048, 0, 2048, 1024, 86, "cuda:0", "fp16x2")
    with pytest.raises(PregoError, match="fp16x2"):
        e.set_anticipation(w, b, 4)
    e2 = MiniRoadEngine(2048, 0, 2048, 1024, 86, "cuda:0", "bf16", num_layers=2)
    with pytest.raises(PregoError, match="num_layers"):
        e2.set_anticipation(w, b, 4)
    e3 = MiniRoadEngine(2048, 0, 2048, 1024, 86, "cuda:0", "bf16")
    lib = _lib.load()
    for L in (0, 33):
        assert lib.prego_miniroad_set_anticipation(e3.h, L, C.c_void_p(w.data_ptr()), C.c_void_p(b.data_ptr()), None) != 0
        assert b"anticipation_length" in lib.prego_miniroad_last_error(e3.h)
    with pytest.raises(PregoError, match="before set_anticipation"):
        e3.forward_ragged([torch.zeros((8, 2048), device="cuda")], None, want_ant=True)
    # C > 128 never reaches the head: a handle of more classes is refused at creation (the same limit as the classifier)
    with pytest.raises(PregoError, match="num_classes"):
        MiniRoadEngine(2048, 0, 2048, 1024, 129, "cuda:0", "bf16")
    cfg = anticipation_cfg(assembly101_cfg(), 4)
    with pytest.raises(PregoError):
        _model(dict(cfg, num_layers=2), {}, "bf16")


class _Log:
    def info(self, *a, **k):
        pass


def test_oad_ant_loss_value_and_gradient():
    import prego_amd.loss  # noqa: F401
    from prego_amd.registry import CRITERIONS
    g = np.load(os.path.join(G, "g12_ant_loss.npz"))
    cfg = anticipation_cfg(assembly101_cfg(num_classes=5), 3)
    logits = torch.from_numpy(W.normal((3, 4, 3, 5), 7, "loss.logits")).cuda().requires_grad_(True)
    target = torch.from_numpy((W.uniform01((3, 4, 5), 7, "loss.t") > 0.6).astype(np.float32)).cuda()
    ant_t = torch.from_numpy((W.uniform01((3, 3, 5), 7, "loss.at") > 0.6).astype(np.float32)).cuda()
    crit = CRITERIONS["ANTICIPATION"](cfg)
    assert crit.reduction == "sum"
    loss = crit({"anticipation_logits": logits}, target, ant_t)
    loss.backward()
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-4 * max(1.0, abs(float(g["loss"])))
    assert np.abs(logits.grad.cpu().numpy() - g["grad"]).max() < 1e-5


def test_ant_evaluate_end_to_end(tmp_path):
    """EVAL["ANTICIPATION"] over the *_ANTICIPATION data layer: MiniROADA batched through forward_clips with the device AP, and the
    stand-in model through the per-batch path with the device AP, against the reference's ANT_Evaluate"""
    import json
    import prego_amd.data  # noqa: F401
    import prego_amd.evaluate  # noqa: F401
    from prego_amd.registry import DATA_LAYERS, EVAL
    from scripts.gen_golden_anticipation import StandIn, make_tree
    ref = json.load(open(os.path.join(G, "g12_ant_eval.json")))
    cfg = dict(make_tree(str(tmp_path)), metric="AP")
    loader = torch.utils.data.DataLoader(DATA_LAYERS[cfg["data_name"]](cfg, "test"), batch_size=1, shuffle=False)
    for dtype, tol in (("fp32", 1e-3), ("bf16", 2e-2)):
        sd = W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0)
        m = _model(cfg, sd, dtype)
        ev = EVAL["ANTICIPATION"](cfg)
        mean = ev(m, loader, _Log(), "cuda:0")
        assert abs(mean - ref["mroada_AP"]["mean"]) < tol, (dtype, mean)
        got = [ev.result[f"anticipation_{l + 1}"]["mean_AP"] for l in range(3)]
        assert np.allclose(got, ref["mroada_AP"]["steps"], rtol=0, atol=tol), dtype
    ev = EVAL["ANTICIPATION"](cfg)
    mean = ev(StandIn().cuda().eval(), loader, _Log(), "cuda:0")
    assert abs(mean - ref["standin_AP"]["mean"]) < 1e-5
