"""GPU: Evaluate's device feature cache (cfg['eval_cache_device'], prego_amd/eval_cache.py) and its conversion kernel
(prego_cast_features, csrc/feature_cache.hip).  The first call with the switch on runs from the loader and leaves the features in HBM in
the form the next forward reads; later calls on the same loader never touch it again.  Every comparison here is exact: the kernel
applies the pack kernels' conversion, and a clip's result does not depend on how a call is batched or which pass runs it."""
import ctypes as C
import json
import logging
import os

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import weights as W                        # noqa: E402
from prego_amd.config import epic_tent_cfg                # noqa: E402

LENS = [1, 40, 137, 300, 513]                             # 991 frames
D = 2048
_T16 = {"fp16": torch.float16, "bf16": torch.bfloat16}


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------
_SPECIALS = [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 65504.0, -65504.0, 65520.0, -65520.0, 1e6, -1e6, 3e38, -3e38]
# the last shape is past one sweep of the grid on a 256-CU device (8 workgroups of 256 lanes per CU, 8 elements per lane): there the
# grid-stride loop runs a third, partial time
_SHAPES = [(1, 64), (3, 2048), (257, 1024), (8, 99991), (8, 2 * 2048 * 256 + 77)]
_inputs = {}


def _input(shape):
    """seeded normals at three scales, side by side, with the special values planted; built once per shape"""
    if shape not in _inputs:
        g = torch.Generator().manual_seed(shape[0] * 1000003 + shape[1])
        xs = []
        for scale in (1.0, 1e-6, 1e4):
            x = torch.randn(shape, generator=g) * scale
            flat = x.view(-1)
            step = flat.numel() // len(_SPECIALS)
            flat[::step][:len(_SPECIALS)] = torch.tensor(_SPECIALS)
            xs.append(x)
        x = torch.stack(xs)
        assert not torch.isnan(x).any()
        _inputs[shape] = (x, {"bf16": x.to(torch.bfloat16).view(torch.int16), "fp16": x.clamp(-65504, 65504).to(torch.float16).view(torch.int16)})
    return _inputs[shape]


def _cast(lib, src, dst, n, code):
    return lib.prego_cast_features(C.c_void_p(src), C.c_void_p(dst), n, code, C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("shape", _SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cast_kernel_gives_torchs_bits(shape, dtype):
    from prego_amd import _lib
    lib = _lib.load()
    x, want = _input(shape)
    src = x.cuda()
    dst = torch.empty(x.shape, dtype=_T16[dtype], device="cuda")
    code = _lib.PREGO_F16 if dtype == "fp16" else _lib.PREGO_BF16
    assert _cast(lib, src.data_ptr(), dst.data_ptr(), src.numel(), code) == 0
    got = dst.cpu().view(torch.int16)
    bad = (got != want[dtype]).nonzero()
    assert bad.numel() == 0, (len(bad), [(x[tuple(i)].item(), hex(got[tuple(i)].item() & 0xFFFF), hex(want[dtype][tuple(i)].item() & 0xFFFF)) for i in bad[:8]])


def test_cast_kernel_refusals_leave_dst_untouched():
    from prego_amd import _lib
    lib = _lib.load()
    src = torch.ones(4096, device="cuda")
    dst = torch.full((4096,), 0x5A5A, dtype=torch.int16, device="cuda")
    s, d, bf = src.data_ptr(), dst.data_ptr(), _lib.PREGO_BF16
    assert _cast(lib, s, d, 0, bf) == 0                                          # nothing to do is not an error
    for what, args in {"NULL src": (None, d, 64, bf), "NULL dst": (s, None, 64, bf), "negative n": (s, d, -8, bf), "n % 8": (s, d, 12, bf),
                       "misaligned src": (s + 4, d, 64, bf), "misaligned dst": (s, d + 2, 64, bf), "fp32 dtype": (s, d, 64, _lib.PREGO_F32),
                       "fp16x2 dtype": (s, d, 64, _lib.PREGO_F16X2), "unknown dtype": (s, d, 64, 9),
                       "overlap": (s, s + 64, 64, bf)}.items():
        assert _cast(lib, *args) == -1, what
        assert b"cast_features" in lib.prego_last_error()
    torch.cuda.synchronize()
    assert bool((dst == 0x5A5A).all()) and bool((src == 1).all())


# ---- the evaluator ---------------------------------------------------------------------------------------------------------------
class _Loader:
    """what the reference's test DataLoader yields (batch dim 1, vid as a 1-tuple), pinned as with pin_memory=True; counts its iterations"""

    def __init__(self, with_flow=False, feature_dtype=torch.float32, seed=21):
        self.items, self.iterations = [], 0
        for i, T in enumerate(LENS):
            rgb = torch.from_numpy(W.tsn_features((T, D), seed, f"ec.rgb.{i}")).to(feature_dtype)[None].pin_memory()
            if with_flow and i != 2:                                 # video 2 ships no flow even then: its cache entry keeps None
                flow = torch.from_numpy(W.tsn_features((T, D), seed, f"ec.flow.{i}")).to(feature_dtype)[None].pin_memory()
            else:
                flow = torch.zeros(1, 1, D, dtype=feature_dtype).expand(1, T, D)
            tgt = torch.zeros(1, T, 12)
            tgt[0, torch.arange(T), (torch.arange(T) // 41 + i) % 12] = 1
            self.items.append((rgb, flow, tgt.pin_memory(), (f"v{i}",), torch.tensor([0]), torch.tensor([T])))

    def __iter__(self):
        self.iterations += 1
        return iter(self.items)


@pytest.fixture(scope="module")
def state_dicts():
    cfg = epic_tent_cfg()
    return {seed: {k: torch.from_numpy(v) for k, v in W.miniroad_state_dict(cfg, seed, head_gain=8.0).items()} for seed in (20, 23)}


def _setup(tmp_path, name, sd, **extra):
    from prego_amd.registry import build_model, build_eval
    import prego_amd.model, prego_amd.evaluate  # noqa: F401
    vl = os.path.join(tmp_path, "video_list.json")
    json.dump({"EPIC-TENT-O": {"class_index": [f"c{i}" for i in range(12)]}}, open(vl, "w"))
    cfg = epic_tent_cfg(eval="dummy.pth", video_list_path=vl, eval_output_dir=os.path.join(tmp_path, name), **extra)
    model = build_model(cfg, "cuda:0")
    model.load_state_dict(sd)
    return build_eval(cfg), model, os.path.join(tmp_path, name, "output_miniROAD.json")


def _call(ev, model, loader, out):
    """one Evaluate call: (mAP as a float, the output file's bytes, every video's probabilities in forward_clips' order)"""
    probs = []
    orig = model.forward_clips

    def spy(*a, **k):
        r = orig(*a, **k)
        probs.extend(r[0])
        return r
    model.forward_clips = spy
    try:
        mAP = float(ev(model, loader, logging.getLogger("t"), "cuda:0"))
    finally:
        del model.forward_clips
    return mAP, open(out, "rb").read(), probs


def _same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and len(a[2]) == len(b[2]) == len(LENS)
    for p, q in zip(a[2], b[2]):
        assert torch.equal(p, q)


def _bytes(dtype, with_flow):
    """features in the kept type + one int32 class id per frame (the one-hot targets' device form)"""
    frames = sum(LENS) + (sum(LENS) - LENS[2] if with_flow else 0)
    return frames * D * (4 if dtype == "fp32" else 2) + 4 * sum(LENS)


@pytest.mark.parametrize("host16", [False, True], ids=["fp32_features", "16bit_features"])
@pytest.mark.parametrize("with_flow", [False, True], ids=["zero_flow", "flow"])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_second_call_runs_from_the_cache_and_equals_the_first(tmp_path, state_dicts, dtype, with_flow, host16):
    ev, model, out = _setup(str(tmp_path), "o", state_dicts[20], compute_dtype=dtype, eval_cache_device=True)
    loader = _Loader(with_flow, _T16[dtype] if host16 else torch.float32)
    casts = []
    from prego_amd import _lib
    lib = _lib.load()
    real = lib.prego_cast_features
    try:
        lib.prego_cast_features = lambda *a: (casts.append(a[2]), real(*a))[1]
        first = _call(ev, model, loader, out)
    finally:
        lib.prego_cast_features = real
    assert ev.last_source == "loader" and loader.iterations == 1
    # 16-bit host features are kept as they arrived; fp32 ones go through the kernel once per tensor
    assert sorted(casts) == ([] if host16 else sorted([T * D for T in LENS] + ([T * D for i, T in enumerate(LENS) if i != 2] if with_flow else [])))
    second = _call(ev, model, loader, out)
    assert ev.last_source == "cache" and loader.iterations == 1
    info = ev.cache_info()
    assert info["enabled"] is True and info["state"] == "filled" and info["reason"] is None
    assert (info["videos"], info["frames"], info["dtype"], info["bytes"]) == (5, 991, dtype, _bytes(dtype, with_flow))
    _same(first, second)
    assert json.loads(second[1]).keys() == {f"v{i}" for i in range(5)}
    assert ev.last_fps and ev.last_fps > 0 and set(ev.last_device_argmax) == {f"v{i}" for i in range(5)}


def test_fp32_engine_keeps_fp32_features(tmp_path, state_dicts):
    ev, model, out = _setup(str(tmp_path), "o", state_dicts[20], compute_dtype="fp32", eval_cache_device=True)
    loader = _Loader(with_flow=True)
    first = _call(ev, model, loader, out)
    assert ev.last_source == "loader"
    second = _call(ev, model, loader, out)
    assert ev.last_source == "cache" and loader.iterations == 1
    info = ev.cache_info()
    assert (info["state"], info["videos"], info["frames"], info["dtype"], info["bytes"]) == ("filled", 5, 991, "fp32", _bytes("fp32", True))
    _same(first, second)


def test_cache_holds_features_not_results(tmp_path, state_dicts):
    ev, model, out = _setup(str(tmp_path), "o", state_dicts[20], eval_cache_device=True)
    loader = _Loader()
    first = _call(ev, model, loader, out)
    model.load_state_dict(state_dicts[23])
    second = _call(ev, model, loader, out)
    assert ev.last_source == "cache" and loader.iterations == 1
    ev0, model0, out0 = _setup(str(tmp_path), "fresh", state_dicts[23])
    fresh = _call(ev0, model0, _Loader(), out0)
    assert ev0.last_source == "loader" and ev0.cache_info()["enabled"] is False
    _same(second, fresh)
    assert second[1] != first[1]


def test_budget_decides_whether_a_set_is_cached_never_what_it_scores(tmp_path, state_dicts):
    need = _bytes("fp16", True)
    ref = None
    for name, limit, cached in (("free", None, True), ("short", need - 1, False), ("exact", need, True)):
        extra = {} if limit is None else {"eval_cache_max_bytes": limit}
        ev, model, out = _setup(str(tmp_path), name, state_dicts[20], eval_cache_device=True, **extra)
        loader = _Loader(with_flow=True)
        first = _call(ev, model, loader, out)
        second = _call(ev, model, loader, out)
        ref = ref or first
        _same(first, ref)
        _same(second, ref)
        info = ev.cache_info()
        if cached:
            assert ev.last_source == "cache" and loader.iterations == 1 and info["state"] == "filled" and info["bytes"] == need
        else:
            assert ev.last_source == "loader" and loader.iterations == 2
            assert info["state"] == "disabled" and info["bytes"] == 0 and info["videos"] == 0 and "budget" in info["reason"]


def test_cache_belongs_to_one_loader_object(tmp_path, state_dicts):
    ev, model, out = _setup(str(tmp_path), "o", state_dicts[20], eval_cache_device=True)
    a, b = _Loader(), _Loader()
    ref = _call(ev, model, a, out)
    _same(_call(ev, model, a, out), ref)
    assert ev.last_source == "cache"
    _same(_call(ev, model, b, out), ref)                     # the same videos in another object: refilled from it
    assert ev.last_source == "loader" and (a.iterations, b.iterations) == (1, 1)
    _same(_call(ev, model, b, out), ref)
    assert ev.last_source == "cache" and b.iterations == 1
    ev.drop_cache()
    assert ev.cache_info()["state"] == "empty" and ev.cache_info()["bytes"] == 0
    _same(_call(ev, model, b, out), ref)
    assert ev.last_source == "loader" and b.iterations == 2
    plain = list(b.items)                                    # a plain list as the loader (no weak reference to it): keyed by identity
    _same(_call(ev, model, plain, out), ref)
    assert ev.last_source == "loader"
    _same(_call(ev, model, plain, out), ref)
    assert ev.last_source == "cache"


def test_cached_call_at_the_split_pass_threshold(tmp_path, state_dicts):
    """the smallest size at which a cached call (one resident forward over the whole set) may take another pass than the filling call
    (two parts by length): all three calls must write the same file and score the same mAP whichever pass ran"""
    g = torch.Generator().manual_seed(7)
    lens = [int(x) for x in torch.randint(5470, 5560, (48,), generator=g)]
    if sum(lens) % 256 == 0:
        lens[0] += 1
    assert sum(lens) >= 262144 and sum(lens) % 256 != 0
    gd = torch.Generator(device="cuda")
    items = []
    for i, T in enumerate(lens):
        gd.manual_seed(4000 + i)
        tgt = torch.zeros(1, T, 12)
        tgt[0, torch.arange(T), (torch.arange(T) // 97 + i) % 12] = 1
        items.append((torch.randn((1, T, D), device="cuda", generator=gd).clamp_(min=0), torch.zeros(1, 1, D).expand(1, T, D), tgt,
                      (f"v{i}",), torch.tensor([0]), torch.tensor([T])))
    ev, model, out = _setup(str(tmp_path), "o", state_dicts[20], assume_zero_flow=True, eval_cache_device=True)
    res = []
    for call in range(3):
        mAP = float(ev(model, items, logging.getLogger("t"), "cuda:0"))
        res.append((mAP, open(out, "rb").read()))
        print(f"call {call + 1}: source {ev.last_source}, pass {model.engine().pass_info()}, mAP {mAP:.6f}")
        assert ev.last_source == ("loader" if call == 0 else "cache")
    assert res[0] == res[1] == res[2]
    info = ev.cache_info()
    assert (info["videos"], info["frames"], info["dtype"]) == (48, sum(lens), "fp16")
