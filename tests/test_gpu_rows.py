"""GPU tests of the element-wise and small-reduction kernels of the training steps (csrc/train.hip, rowwise.hip, vit_train.hip, vit.hip,
optim.hip), each launched ALONE through the entry points of include/prego_amd_debug.h (csrc/rows_debug.cpp), which call the launch_*
functions of csrc/kernels.h as the training steps do.

Exact tests ask for bit equality with the fp64 reference on EVERY element (input families of tests/helpers/rows_exact.py for which any
summation order and any FMA contraction give the same bits; the claim itself is tested on the CPU, tests/test_rows_reference_cpu.py).
Bounded tests assert err <= bound with the per-element worst-case bounds derived in that module; the largest err / bound seen on an
MI355X stands in each such test's docstring.  Every output lies in a canary-filled allocation (exactly the documented block may change),
inputs carry NaN wherever the entry's contract says nothing is read.

  kernel (launcher)                     instantiations / paths reached                                             held
  ln_relu_rows (launch_ln_relu, _x2)    fp32->fp32/bf16/fp16, bf16->bf16, fp16->fp16, x2; MAXV 4 and 8; grid-stride; arm   bounded; mean, zero pattern exact
  ln_relu_bwd_rows + colsum_stage2      MAXV 8 and 16; relu 0/1; accumulate; dYb; dropout                           exact at E = 2^k, dY bounded else
  colsum_stage1<float / bf16>, stage2   1 .. 17 partial blocks, uneven slices, nb up to 33                            exact
  transpose_convert                     four type pairs, Mpad = M and padded, ld_src > N                            exact
  gather_dlogits, build_hprev           fp32 and bf16, ragged plan 5 / 3 / 1, C < Cpad and C = Cpad                   exact
  relu_mask, pad_convert, f32_to_bf16   below and above the grid caps; fp32 / bf16 / saturating fp16                  exact
  gru_bwd_step<float / bf16>            t = 0 and t > 0, na_next 0 / na - 1 / na                                     exact
  gelu_bwd, mask_convert                n = 4, 1020, 8192 workgroups + 1 vector; one and two masks; no fp32 output   bounded / exact
  vit_head, vit_head_bwd1/2             C 1 .. 600 (bwd above 128 after its fix, C > E), argmax tie                  bounded; dy, g_lnb, g_hb exact
  vit_tokens, vit_tokens_bwd            B 1 / 3, T 1 / 8, p 0 / 0.1                                                 exact (g_pe bounded at p 0.1)
  oad_loss                              C 1 .. 128, 1 .. 33 clips, ragged T, the serial path (4097 clips)             bounded; leading rows exact zero
  adamw                                 vector, partial-vector and scalar (unaligned view) paths, 25 tensors          bounded"""
import ctypes as ct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.helpers import gemm_exact as gx  # noqa: E402
from tests.helpers import rows_exact as rx  # noqa: E402

PREGO_EINVAL = -1
SEED, ROW0 = 0x5EED5EED5, 7
T32, TBF, TF16 = rx.T32, rx.TBF, rx.TF16
TT = rx.TORCH_TYPE


def _lib():
    from prego_amd import _lib
    return _lib.load_debug()


_KEEP = []          # every device buffer a call was given stays allocated until the test ends (a freed temporary's block would be handed out again)


@pytest.fixture(autouse=True)
def _release_buffers():
    yield
    _KEEP.clear()


@pytest.fixture(scope="module", autouse=True)
def _return_cached_memory():
    """the largest cases here take blocks of a few hundred MB each: hand them back to the device when the module is done, so that the
    tests that run after it find the allocator as small as they would without this file"""
    yield
    _KEEP.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _vp(x):
    if isinstance(x, torch.Tensor):
        _KEEP.append(x)
    return ct.c_void_p(x if isinstance(x, int) else (x.data_ptr() if x is not None else None))


def _s():
    return _vp(torch.cuda.current_stream().cuda_stream)


def _gen(*k):
    return np.random.default_rng([99, *[int(x) for x in k]])


def _ok(lib, rc):
    torch.cuda.synchronize()
    assert rc == 0, lib.prego_last_error()


def dev(x, typ=T32):
    """numpy fp64 / fp32 or torch values -> a contiguous device tensor of the type"""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.float64).astype(np.float32)))
    return t.to(torch.float32).to(TT[typ]).cuda().contiguous()


class Guarded:
    """rows x cols of values inside a NaN-filled allocation: GUARD rows of NaN before and behind, NaN in columns cols .. ld-1"""

    def __init__(self, vals, ld=None, typ=T32):
        vals = dev(vals, typ)
        vals = vals.reshape(1, -1) if vals.dim() < 2 else vals.reshape(-1, vals.shape[-1])
        R, Cn = vals.shape
        self.ld = ld or Cn
        self.buf = torch.full(((2 * gx.GUARD + R) * self.ld,), float("nan"), dtype=TT[typ], device="cuda")
        self.buf.view(-1, self.ld)[gx.GUARD:gx.GUARD + R, :Cn] = vals
        self.vals = vals
        _KEEP.append(self)

    def ptr(self, row=0):
        return self.buf.data_ptr() + (gx.GUARD + row) * self.ld * self.buf.element_size()


def out(M, N, typ=T32, ld=None):
    return gx.make_output(M, N, ld or N, TT[typ], "cuda")


def np64(t):
    return t.detach().to(torch.float64).cpu().numpy()


def exact(o, want, what):
    """the block equals `want` bit for bit and nothing else of the allocation changed"""
    assert o.canary_elsewhere(), f"{what}: an element outside the documented block was written"
    rx.assert_exact(o.block().cpu(), want if isinstance(want, torch.Tensor) else rx.t32(want).to(o.buf.dtype), what)


def within(o, ref64, bound64, what, typ=T32):
    assert o.canary_elsewhere(), f"{what}: an element outside the documented block was written"
    return rx.assert_within(np64(o.block()), ref64, rx.store_bound(ref64, bound64, typ), what)


# ================================================================================================ ln_relu_rows
_LN_PAIRS = [(T32, T32), (T32, TBF), (T32, TF16), (TBF, TBF), (TF16, TF16)]
_LN_E = [512, 1536, 2048, 2560, 4096]
_LN_R = [1, 3, 4, 5, 67]
_LN_CASES = [(E, _LN_R[(i + j) % 5], it, ot, (i * 5 + j) % 2 == 0, (i * 5 + j) // 2 % 2, 0.2 if (i * 5 + j) % 3 == 0 else 0.0)
             for i, E in enumerate(_LN_E) for j, (it, ot) in enumerate(_LN_PAIRS)]


def _ln_call(lib, it, ot, Y, gamma, beta, R, E, o, stats, p, relu, arm=(0, 0, 0, None, None), row0=ROW0):
    return lib.prego_debug_ln_relu(it, ot, _vp(Y), _vp(gamma), _vp(beta), R, E, 1e-5, _vp(o), _vp(stats), p, SEED, row0, relu, arm[0], arm[1], arm[2],
                                   _vp(arm[3]), _vp(arm[4]), _s())


@pytest.mark.parametrize("E,R,it,ot,keep,relu,p", _LN_CASES, ids=lambda v: str(v))
def test_ln_relu_rows_within_derived_bound(E, R, it, ot, keep, relu, p):
    """Every (in, out) type pair launch_ln_relu reaches, MAXV = 4 (E <= 2048) and MAXV = 8, partial last row blocks.  out and
    stats[2r + 1] (rstd) within rows_exact.ln_forward_bounds; stats[2r] (mean) bit-exact where E is a power of two; dropped elements are
    exact zeros at the positions of hash(seed, (row0_abs + r) E + c), kept ones are not.
    Largest err / bound seen on an MI355X (gfx950, ROCm 7.2, 2026-10-21): out 0.21 with fp32 rows out, 0.9997 (bf16) and 0.999 (fp16) with
    16-bit rows out (there half an ulp of the store is nearly all of the bound, and a tie uses all of it); mean 5.1e-3, rstd 4.6e-2."""
    lib = _lib()
    Y64, g64, b64 = rx.ln_inputs(R, E, _gen(E, R, it, ot), it)
    Y, gam, bet = Guarded(Y64, typ=it), dev(g64), dev(b64)
    o = out(R, E, ot)
    st = out(R, 2) if keep else None
    _ok(lib, _ln_call(lib, it, ot, Y.ptr(), gam, bet, R, E, o.ptr(), st.ptr() if keep else None, p, relu))
    ref, mu, rstd = rx.ln_relu_ref(Y64, g64, b64, 1e-5, relu, p, SEED, ROW0)
    if ot == TF16:
        ref = np.clip(ref, -rx.F16_MAX, rx.F16_MAX)
    scale = float(rx.drop_scale(p))
    bound, d_mu, d_rstd, _ = rx.ln_forward_bounds(Y64, g64, b64, float(np.float32(1e-5)), E // 64 + 6, scale)
    kept = rx.keep_mask(SEED, ROW0 * E, R * E, p).reshape(R, E)
    got = np64(o.block())
    assert (got[~kept] == 0).all(), "a dropped element is not zero"
    assert (got[kept & (np.abs(ref) > 2 * rx.store_bound(ref, bound, ot))] != 0).all(), "a kept element was dropped"
    within(o, ref, np.where(kept, bound, 0.0), "out", ot)
    if keep:
        assert st.canary_elsewhere()
        s = np64(st.block())
        if E & (E - 1) == 0:
            assert rx.exact32(mu) and (s[:, 0] == mu).all(), "mean of dyadic rows at a power-of-two E"
        rx.assert_within(s[:, 0], mu, d_mu, "stats mean")
        rx.assert_within(s[:, 1], rstd, d_rstd, "stats rstd")


@pytest.mark.parametrize("E,R", [(512, 5), (2560, 3)])
def test_ln_relu_x2_split_rows_within_derived_bound(E, R):
    """launch_ln_relu_x2 (MAXV 4 and 8): out [R][2E] fp16 = [hi | lo]; hi + lo against the fp32 bound + 2^-22 |ref| + 2^-24 (two fp16
    roundings of a value and of its remainder; fp16's subnormal spacing).  Largest err / bound on an MI355X (ROCm 7.2, 2026-10-21): 0.24."""
    lib = _lib()
    Y64, g64, b64 = rx.ln_inputs(R, E, _gen(E, R))
    Y, gam, bet = Guarded(Y64), dev(g64), dev(b64)
    o = out(R, 2 * E, TF16)
    _ok(lib, lib.prego_debug_ln_relu_x2(_vp(Y.ptr()), _vp(gam), _vp(bet), R, E, 1e-5, _vp(o.ptr()), _s()))
    ref, _, _ = rx.ln_relu_ref(Y64, g64, b64, 1e-5, 1, 0.0, 0, 0)
    bound = rx.ln_forward_bounds(Y64, g64, b64, float(np.float32(1e-5)), E // 64 + 6)[0]
    assert o.canary_elsewhere()
    got = np64(o.block())
    rx.assert_within(got[:, :E] + got[:, E:], ref, bound + 2.0 ** -22 * np.abs(ref) + 2.0 ** -24, "hi + lo")
    hi = rx.convert(rx.t32(ref), TF16).to(torch.float64).numpy()
    assert (np.abs(got[:, :E] - hi) <= rx.ulp16(ref, TF16) + bound).all(), "hi is not the fp16 value of the row"


def test_ln_relu_rows_grid_stride_over_65541_rows():
    """4 x 16384 + 5 rows of E = 512, bf16 in and out: the grid is capped at 16384 workgroups, so every wave takes a second row.  The rows
    repeat a block of 61 distinct rows (no dropout: a row's result depends on the row alone), compared on the device against the bound of
    test_ln_relu_rows_within_derived_bound (bf16 rows out: the ratio there, 0.9997, is the store's half ulp)."""
    lib = _lib()
    R, E, P = 4 * 16384 + 5, 512, 61
    Y64, g64, b64 = rx.ln_inputs(P, E, _gen(1), TBF)
    idx = torch.arange(R, device="cuda") % P
    Y = dev(Y64, TBF)[idx].contiguous()
    gam, bet = dev(g64), dev(b64)
    o = out(R, E, TBF)
    _ok(lib, _ln_call(lib, TBF, TBF, Y, gam, bet, R, E, o.ptr(), None, 0.0, 1))
    ref, _, _ = rx.ln_relu_ref(Y64, g64, b64, 1e-5, 1, 0.0, 0, 0)
    bound = rx.store_bound(ref, rx.ln_forward_bounds(Y64, g64, b64, float(np.float32(1e-5)), E // 64 + 6)[0], TBF)
    assert o.canary_elsewhere()
    got = o.block().to(torch.float64)
    err = (got - torch.from_numpy(ref).cuda()[idx]).abs()
    assert bool(torch.isfinite(got).all()) and bool((err <= torch.from_numpy(bound).cuda()[idx]).all())
    assert bool((o.block()[:P].view(torch.int16)[idx % P] == o.block().view(torch.int16)).all()), "equal rows gave different bits"


def test_ln_relu_rows_rearms_the_recurrence_on_the_side():
    """with a GruArm: words [0, W) of the exchange buffers hold the tag pattern, [W, 2W) zero, the first 16 rendezvous words zero - and
    nothing beyond either (kernels.h: GruArm, gru_arm_desc)"""
    lib = _lib()
    hid, G, R, E = 512, 1, 5, 512
    nbytes = lib.prego_debug_gru_hx_offset(10, 2, 0, hid, G, 0)
    W = nbytes // 8
    assert nbytes > 0 and nbytes % 32 == 0
    pad = 64
    hx = torch.full((pad + 2 * W + pad,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    sync = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    Y64, g64, b64 = rx.ln_inputs(R, E, _gen(2))
    o = out(R, E, TBF)
    _ok(lib, _ln_call(lib, T32, TBF, dev(Y64), dev(g64), dev(b64), R, E, o.ptr(), None, 0.0, 1, arm=(1, hid, G, hx.data_ptr() + pad * 4, sync)))
    assert bool((hx[:pad] == 0x5A5A5A5A).all()) and bool((hx[pad + 2 * W:] == 0x5A5A5A5A).all()), "written outside the exchange buffers"
    assert bool((hx[pad:pad + W] == 0x40004000).all()) and bool((hx[pad + W:pad + 2 * W] == 0).all())
    assert bool((sync[:16] == 0).all()) and bool((sync[16:] == 0x5A5A5A5A).all())
    ref = rx.ln_relu_ref(Y64, g64, b64, 1e-5, 1, 0.0, 0, 0)[0]
    within(o, ref, rx.ln_forward_bounds(Y64, g64, b64, float(np.float32(1e-5)), E // 64 + 6)[0], "out beside the arm", TBF)


@pytest.mark.parametrize("why,kw", [("E % 512", dict(E=768)), ("E > 4096", dict(E=4608)), ("bf16 -> fp32", dict(it=TBF, ot=T32)),
                                    ("fp16 -> bf16", dict(it=TF16, ot=TBF)), ("nrows 0", dict(R=0))])
def test_ln_relu_refusals_launch_nothing(why, kw):
    lib = _lib()
    E, R, it, ot = kw.get("E", 512), kw.get("R", 4), kw.get("it", T32), kw.get("ot", T32)
    o = out(4, 4608, T32)
    Y = torch.zeros(4 * 4608, device="cuda")
    rc = _ln_call(lib, it, ot, Y, Y, Y, R, E, o.ptr(), None, 0.0, 1)
    torch.cuda.synchronize()
    assert rc == PREGO_EINVAL and o.untouched(), why


# ================================================================================================ ln_relu_bwd
_LNB_E = [256, 768, 2048, 2304, 4096]
_LNB_R = [1, 3, 4, 5, 66]
_LNB_V = [(1, 0, 0.0, 1), (1, 1, 0.2, 1), (0, 0, 0.2, 0), (0, 1, 0.0, 0)]          # relu, accumulate, p, dYb given
_LNB_CASES = [(E, _LNB_R[(i + j) % 5], *_LNB_V[j]) for i, E in enumerate(_LNB_E) for j in range(4)]


@pytest.mark.parametrize("E,R,relu,acc,p,with_b", _LNB_CASES, ids=lambda v: str(v))
def test_ln_relu_bwd_exact_at_powers_of_two_bounded_elsewhere(E, R, relu, acc, p, with_b):
    """MAXV = 8 and MAXV = 16 (E > 2048: 64 KiB of LDS), partial last row block, the partials summed by launch_colsum_stage2 over 2E columns.
    At E in {256, 2048, 4096} dY, its bf16 copy, dgamma, dbeta and the accumulate path are bit-exact (rows_exact.ln_bwd_is_exact holds on the
    instance); at E in {768, 2304} the row means do not divide: dY against rows_exact.ln_bwd_dy_bound, dgamma / dbeta still exact.  The mask
    is the forward's, on the same (seed, row0_abs).  Largest err / bound on an MI355X (gfx950, ROCm 7.2, 2026-10-21): dY 0.43, dYb 0.9999
    (the bf16 store's half ulp)."""
    lib = _lib()
    a = rx.ln_bwd_inputs(R, E, _gen(E, R, relu, acc))
    dY = out(R, E)
    dY.block()[:] = dev(a["prior"])
    dYb = out(R, E, TBF) if with_b else None
    nb = (R + 3) // 4
    part, dgb = out(nb, 2 * E), out(1, 2 * E, ld=2 * E + 8)
    ins = [Guarded(a[k]) for k in ("dE", "Y")]
    _ok(lib, lib.prego_debug_ln_relu_bwd(_vp(ins[0].ptr()), _vp(ins[1].ptr()), _vp(dev(a["stats"])), _vp(dev(a["gamma"])), _vp(dev(a["beta"])), R, E, p,
                                         SEED, ROW0, _vp(dY.ptr()), _vp(dYb.ptr() if with_b else None), _vp(part.ptr()), _vp(dgb.ptr()), relu, acc, _s()))
    want_dY, dgam, dbet, pre = rx.ln_bwd_ref(a, relu, p, SEED, ROW0, acc)
    assert part.canary_elsewhere()
    exact(dgb, np.concatenate([dgam, dbet])[None], "dgamma | dbeta")
    if E & (E - 1) == 0:
        assert rx.ln_bwd_is_exact(a, relu, p, SEED, ROW0, acc)
        exact(dY, want_dY, "dY")
        if with_b:
            exact(dYb, gx.expected_bf16(torch.from_numpy(want_dY)), "dYb")
    else:
        bound = rx.ln_bwd_dy_bound(a, relu, p, SEED, ROW0, acc)
        within(dY, want_dY, bound, "dY")
        if with_b:
            within(dYb, want_dY, bound, "dYb", TBF)
            rx.assert_exact(dYb.block().cpu(), dY.block().cpu().to(torch.bfloat16), "dYb is the bf16 of the stored dY")


@pytest.mark.parametrize("why,E,R", [("E % 256", 384 + 64, 4), ("E > 4096", 4352, 4), ("nrows 0", 256, 0)])
def test_ln_relu_bwd_refusals_launch_nothing(why, E, R):
    lib = _lib()
    z = torch.zeros(4 * 4352, device="cuda")
    dY = out(4, 4352)
    rc = lib.prego_debug_ln_relu_bwd(_vp(z), _vp(z), _vp(z), _vp(z), _vp(z), R, E, 0.0, 0, 0, _vp(dY.ptr()), None, _vp(z), _vp(z), 1, 0, _s())
    torch.cuda.synchronize()
    assert rc == PREGO_EINVAL and dY.untouched() and float(z.abs().sum()) == 0, why


# ================================================================================================ column sums
@pytest.mark.parametrize("M", [1, 63, 64, 65, 1030])
@pytest.mark.parametrize("N", [1, 64, 65, 300])
def test_colsum_exact_integer(M, N):
    """fp32 and bf16 rows; 1030 rows = 17 partial blocks, so stage 2's 16 slices are uneven (2 partials each, the last ones empty)"""
    lib = _lib()
    src64 = rx.int_matrix(M, N, _gen(M, N))
    for bf in (0, 1):
        src = Guarded(src64, typ=TBF if bf else T32)
        part, o = out((M + 63) // 64, N), out(1, N, ld=N + 8)
        _ok(lib, lib.prego_debug_colsum(bf, _vp(src.ptr()), M, N, _vp(part.ptr()), _vp(o.ptr()), _s()))
        assert part.canary_elsewhere()
        exact(o, rx.colsum_ref(src64)[None], f"colsum bf16={bf}")


@pytest.mark.parametrize("nb", [1, 15, 16, 17, 33])
def test_colsum_stage2_exact_integer(nb):
    lib = _lib()
    N = 65
    p64 = rx.int_matrix(nb, N, _gen(nb), 127) * 1024
    part, o = Guarded(p64), out(1, N, ld=N + 8)
    _ok(lib, lib.prego_debug_colsum_stage2(_vp(part.ptr()), nb, N, _vp(o.ptr()), _s()))
    exact(o, p64.sum(0)[None], "stage 2")


# ================================================================================================ transpose_convert
@pytest.mark.parametrize("M", [1, 31, 32, 33, 70])
@pytest.mark.parametrize("N", [1, 32, 33, 100])
def test_transpose_convert_exact(M, N):
    """all four type pairs, Mpad = M and M rounded up to 64, ld_src > N: the pad columns of dst are zero, rows of src past M and its pad
    columns are NaN and never read; bf16 stores round to nearest even (ties, subnormals, signed zeros among the values)"""
    lib = _lib()
    ld = gx.round_up(N, 8) + 8
    vals = torch.from_numpy(rx.finite_values(M * N, _gen(M, N), TBF)).view(M, N)
    for ib in (0, 1):
        src = Guarded(vals, ld, TBF if ib else T32)
        for ob in (0, 1):
            for Mpad in (M, gx.round_up(M, 64)):
                o = out(N, Mpad, TBF if ob else T32)
                _ok(lib, lib.prego_debug_transpose_convert(ib, ob, _vp(src.ptr()), M, N, ld, _vp(o.ptr()), Mpad, _s()))
                exact(o, rx.transpose_ref(src.vals.float().cpu(), M, N, Mpad, TBF if ob else T32), f"in bf16={ib} out bf16={ob} Mpad={Mpad}")


# ================================================================================================ gather_dlogits, build_hprev
_LENS = [3, 5, 1]          # the caller's order; the plan sorts them to 5, 3, 1


@pytest.mark.parametrize("C,Cpad", [(86, 128), (128, 128)])
@pytest.mark.parametrize("bf", [0, 1])
def test_gather_dlogits_exact(C, Cpad, bf):
    lib = _lib()
    rowoff, order, rows = rx.plan_rows(_LENS)
    typ = TBF if bf else T32
    dl = [torch.from_numpy(rx.finite_values(T * C, _gen(C, i), TBF)).view(T, C) for i, T in enumerate(_LENS)]
    g = [Guarded(d) for d in dl]
    ptrs = torch.tensor([x.ptr() for x in g], dtype=torch.int64, device="cuda")
    o = out(len(rows), Cpad, typ)
    _ok(lib, lib.prego_debug_gather_dlogits(bf, _vp(ptrs), _vp(torch.from_numpy(rowoff).cuda()), _vp(torch.from_numpy(order).cuda()), max(_LENS), len(rows),
                                            C, Cpad, _vp(o.ptr()), _s()))
    exact(o, rx.gather_dlogits_ref(dl, _LENS, C, Cpad, typ), "gathered rows")


@pytest.mark.parametrize("H", [64, 300])
@pytest.mark.parametrize("bf", [0, 1])
def test_build_hprev_exact(H, bf):
    lib = _lib()
    rowoff, order, rows = rx.plan_rows(_LENS)
    typ = TBF if bf else T32
    n = len(rows)
    Hraw = torch.from_numpy(rx.finite_values(n * H, _gen(H), TBF)).view(n, H)
    src, o = Guarded(Hraw), out(n, H, typ)
    _ok(lib, lib.prego_debug_build_hprev(bf, _vp(src.ptr()), _vp(torch.from_numpy(rowoff).cuda()), max(_LENS), n, H, _vp(o.ptr()), _s()))
    want = rx.build_hprev_ref(Hraw, _LENS, typ)
    assert float(want[:3].float().abs().sum()) == 0          # t = 0 rows
    exact(o, want, "h_{t-1} rows")


@pytest.mark.parametrize("n", [1, 1000, 256 * 4096 + 3])
def test_relu_mask_exact(n):
    """the grid is capped at 4096 workgroups: the largest n runs the stride loop.  Hraw holds +-0 (gradient 0) among the values"""
    lib = _lib()
    g = _gen(n)
    d, h = rx.finite_values(n, g), g.standard_normal(n).astype(np.float32)
    h[::7] = 0.0
    h[3::7] = -0.0
    dd, hh, o = Guarded(d), Guarded(h), out(1, n)
    _ok(lib, lib.prego_debug_relu_mask(_vp(dd.ptr()), _vp(hh.ptr()), n, _vp(o.ptr()), _s()))
    exact(o, torch.from_numpy(np.where(h > 0, d, np.float32(0)))[None], "masked gradient")


# ================================================================================================ gru_bwd_step
_GRU_CASES = sorted({(H, na, nn, t) for H in (64, 512) for na in (1, 3) for nn in (0, na - 1, na) for t in (0, 2)})


@pytest.mark.parametrize("H,na,na_next,t", _GRU_CASES)
def test_gru_bwd_step_exact(H, na, na_next, t):
    """carry_z_out, dGI, dGH and both operand copies (fp32 and bf16) bit for bit.  Rows outside [row_t, row_t + na) of every input are NaN,
    as are rows b >= na_next of carry_z_in / dhpart; at t = 0 Hraw is all NaN (hprev = 0, not read)."""
    lib = _lib()
    a = rx.gru_bwd_inputs(na, H, _gen(H, na, na_next, t))
    assert rx.gru_bwd_product_bits(a, na_next, t) <= rx.GRU_PRODUCT_BITS
    row_t, row_tm1 = 2, 1
    assert row_t <= gx.GUARD and row_tm1 <= gx.GUARD
    rows = {k: Guarded(a[k]) for k in ("dHout", "r", "z", "n", "ghn")}
    hraw = Guarded(a["hprev"] if t > 0 else np.full((na, H), np.nan))
    cin, dhp = a["carry"].copy(), a["dhpart"].copy()
    cin[na_next:], dhp[na_next:] = np.nan, np.nan
    cin, dhp = Guarded(cin), Guarded(dhp)
    want = rx.gru_bwd_ref(a, na_next, t)
    for bf in (0, 1):
        typ = TBF if bf else T32
        carry, dgi, dgh, dgiop, dghop = out(na, H), out(na, 3 * H), out(na, 3 * H), out(na, 3 * H, typ), out(na, 3 * H, typ)
        back = lambda o: o.ptr() - row_t * 3 * H * o.buf.element_size()      # noqa: E731  (row row_t of the array = the block's first row)
        _ok(lib, lib.prego_debug_gru_bwd_step(bf, t, na, na_next, row_t, row_tm1, H, _vp(rows["dHout"].ptr(-row_t)), _vp(cin.ptr()), _vp(dhp.ptr()),
                                              _vp(rows["r"].ptr(-row_t)), _vp(rows["z"].ptr(-row_t)), _vp(rows["n"].ptr(-row_t)), _vp(rows["ghn"].ptr(-row_t)),
                                              _vp(hraw.ptr(-row_tm1)), _vp(carry.ptr()), _vp(back(dgi)), _vp(back(dgh)), _vp(back(dgiop)), _vp(back(dghop)), _s()))
        exact(carry, want[0], "carry_z_out")
        exact(dgi, want[1], "dGI")
        exact(dgh, want[2], "dGH")
        exact(dgiop, rx.convert(rx.t32(want[1]), typ), f"dGI operand copy bf16={bf}")
        exact(dghop, rx.convert(rx.t32(want[2]), typ), f"dGH operand copy bf16={bf}")


# ================================================================================================ pad_convert, f32_to_bf16
@pytest.mark.parametrize("typ", [T32, TBF, TF16])
@pytest.mark.parametrize("shape", [(5, 37, 8, 64), (3, 8, 3, 8), (700, 1000, 1500, 1501)])
def test_pad_convert_exact(typ, shape):
    """rows_src x cols_src of a wider source into a zero-padded rows_dst x cols_dst; the largest case is above the grid cap (stride loop).
    The fp16 store saturates: values beyond +-65504 are among the inputs"""
    lib = _lib()
    rs, cs, rd, cd = shape
    vals = torch.from_numpy(rx.finite_values(rs * cs, _gen(rs, cs, typ), typ)).view(rs, cs)
    src, o = Guarded(vals, cs + 3), out(rd, cd, typ)
    _ok(lib, lib.prego_debug_pad_convert(typ, _vp(src.ptr()), rs, cs, cs + 3, _vp(o.ptr()), rd, cd, _s()))
    want = torch.zeros((rd, cd))
    want[:rs, :cs] = vals
    exact(o, rx.convert(want, typ), "padded copy")


@pytest.mark.parametrize("n", [1, 1000, 8192 * 256 + 5])
def test_f32_to_bf16_exact(n):
    lib = _lib()
    x = rx.finite_values(n, _gen(n), TBF)
    src, o = Guarded(x), out(1, n, TBF)
    _ok(lib, lib.prego_debug_f32_to_bf16(_vp(src.ptr()), _vp(o.ptr()), n, _s()))
    exact(o, rx.convert(torch.from_numpy(x), TBF)[None], "bf16 copy")


# ================================================================================================ gelu_bwd, mask_convert
_N_ELEM = [4, 1020, 256 * 4 * 8192 + 4]          # the last: 8192 workgroups (the grid cap) plus one more vector, so the stride loop runs


@pytest.mark.parametrize("n", _N_ELEM)
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_gelu_bwd_within_derived_bound(n, p):
    """|u| from 1e-4 to 12, both signs.  The bound (rows_exact.gelu_bwd_bound) allows for the fast exponential: (3 u^2 / 2 + 3) U relative
    on phi.  The bf16 copy gets half a bf16 ulp on top and equals the bf16 of the stored fp32 value.  Largest err / bound on an MI355X
    (gfx950, ROCm 7.2, 2026-10-21): du 0.47 (n = 8388612, p = 0.1; 0.08 .. 0.37 in the other cases), bf16 copy 0.9999."""
    lib = _lib()
    g = _gen(n, int(p * 10))
    u = (np.exp(g.uniform(np.log(1e-4), np.log(12.0), n)) * g.choice([-1.0, 1.0], n)).astype(np.float32).astype(np.float64)
    u[:4] = [1e-4, -12.0, 12.0, -1e-4][:min(4, n)]
    df = (g.integers(-64, 65, n) / 16.0)
    du, dub = out(1, n), out(1, n, TBF)
    _ok(lib, lib.prego_debug_gelu_bwd(_vp(Guarded(df).ptr()), _vp(Guarded(u).ptr()), n, _vp(du.ptr()), _vp(dub.ptr()), p, SEED, _s()))
    ref, bound = rx.gelu_bwd_ref(df, u, p, SEED)[None], rx.gelu_bwd_bound(df, u, p, SEED)[None]
    kept = rx.keep_mask(SEED, 0, n, p)[None]
    assert (np64(du.block())[~kept] == 0).all()
    within(du, ref, np.where(kept, bound, 0.0), "du")
    within(dub, ref, np.where(kept, bound, 0.0), "du bf16", TBF)
    rx.assert_exact(dub.block().cpu(), du.block().cpu().to(torch.bfloat16), "the bf16 copy is the bf16 of the stored du")


@pytest.mark.parametrize("n", _N_ELEM)
@pytest.mark.parametrize("p,p2,f32_out", [(0.0, 0.0, True), (0.1, 0.0, False), (0.1, 0.1, True)])
def test_mask_convert_exact(n, p, p2, f32_out):
    """one correctly rounded product per mask: the fp32 numpy evaluation is the reference bit for bit; the nullable fp32 output"""
    lib = _lib()
    x = rx.finite_values(n, _gen(n), TBF)
    x = np.where(np.abs(x) > 1e38, np.float32(1.5), x)          # the scale must not overflow a finite value
    o32, o16 = out(1, n), out(1, n, TBF)
    _ok(lib, lib.prego_debug_mask_convert(_vp(Guarded(x).ptr()), n, _vp(o32.ptr() if f32_out else None), _vp(o16.ptr()), p, SEED, p2, SEED + 1, _s()))
    want = x.copy()
    for pp, sd in ((p, SEED), (p2, SEED + 1)):
        if pp > 0:
            want = np.where(rx.keep_mask(sd, 0, n, pp), want * rx.drop_scale(pp), np.float32(0))
    want = torch.from_numpy(want.astype(np.float32))[None]
    if f32_out:
        exact(o32, want, "fp32 output")
    else:
        assert o32.untouched()
    exact(o16, rx.convert(want, TBF), "bf16 output")


@pytest.mark.parametrize("n", [0, 6, 1022])
def test_gelu_bwd_and_mask_convert_refuse_sizes_that_are_no_multiple_of_4(n):
    lib = _lib()
    z, o32, o16 = torch.zeros(1024, device="cuda"), out(1, 1024), out(1, 1024, TBF)
    assert lib.prego_debug_gelu_bwd(_vp(z), _vp(z), n, _vp(o32.ptr()), _vp(o16.ptr()), 0.0, 0, _s()) == PREGO_EINVAL
    assert lib.prego_debug_mask_convert(_vp(z), n, _vp(o32.ptr()), _vp(o16.ptr()), 0.0, 0, 0.0, 0, _s()) == PREGO_EINVAL
    torch.cuda.synchronize()
    assert o32.untouched() and o16.untouched()


# ================================================================================================ Transformer head
_HEAD_C = [1, 3, 22, 127, 128, 129, 300, 600]          # above 128: the backward's dlogits copy is sized by C (it was a fixed 128 floats)
_HEAD_CASES = [(C, (512, 1536)[i % 2], (1, 5)[(i // 2) % 2], (2, 9)[(i + 1) % 2]) for i, C in enumerate(_HEAD_C)] + [(22, 1536, 1, 9), (128, 512, 5, 2)]


def _head(C, E, B, N):
    a = rx.head_inputs(B, N, E, C, _gen(C, E, B, N))
    if C >= 3:                                            # a tie for the maximum between classes 1 and C - 1: equal rows, equal (large) biases
        a["hw"][C - 1] = a["hw"][1]
        a["hb"][1] = a["hb"][C - 1] = 4096.0
    xs = a["x"].copy()
    xs[:, 1:, :] = np.nan                                 # only token 0 of a window is read
    return a, Guarded(xs.reshape(B * N, E))


@pytest.mark.parametrize("C,E,B,N", _HEAD_CASES)
def test_vit_head_within_derived_bound_and_first_argmax(C, E, B, N):
    """logits against rows_exact.head_ref's bound; classes 1 and C - 1 tie for the maximum bit for bit and argmax names the first.
    Largest err / bound on an MI355X (gfx950, ROCm 7.2, 2026-10-21): 1.8e-2."""
    lib = _lib()
    a, x = _head(C, E, B, N)
    o, am = out(1, B * C), torch.full((B + 4,), -7, dtype=torch.int32, device="cuda")
    _ok(lib, lib.prego_debug_vit_head(_vp(x.ptr()), B, N, E, _vp(dev(a["lnw"])), _vp(dev(a["lnb"])), _vp(dev(a["hw"])), _vp(dev(a["hb"])), C, _vp(o.ptr()),
                                      _vp(am), _s()))
    ref, bound = rx.head_ref(a)
    assert o.canary_elsewhere()
    got = o.block().view(B, C)
    rx.assert_within(np64(got), ref, bound, "logits")
    assert am[B:].tolist() == [-7] * 4
    assert am[:B].tolist() == ([1] * B if C >= 3 else [int(np.argmax(ref[b])) for b in range(B)]), "argmax takes the first maximum"
    if C >= 3:
        assert bool((got[:, 1].view(torch.int32) == got[:, C - 1].view(torch.int32)).all())


@pytest.mark.parametrize("C,E,B,N", _HEAD_CASES)
def test_vit_head_bwd_exact_sums_and_bounded_gradients(C, E, B, N):
    """dy = dlogits hw (scratch[2]), g_lnb and g_hb are sums of small integers: bit-exact.  dx[b, 0, :], g_lnw, g_hw against
    rows_exact.head_bwd_ref's bounds.  Rows 1 .. N-1 of dx keep what the caller put there.  C in {129, 300, 600} ran wrong before the
    dlogits copy was sized by C; 600 > E also has bias gradients beyond the E lanes of a row.  Largest err / bound on an MI355X (gfx950,
    ROCm 7.2, 2026-10-21): dx 7.0e-2, g_lnw 6.9e-2, g_hw 7.7e-2."""
    lib = _lib()
    a, x = _head(C, E, B, N)
    dx = out(B * N, E)
    dx.block()[:] = 7.25
    scratch, g_lnw, g_lnb, g_hw, g_hb = out(3 * B, E), out(1, E), out(1, E), out(C, E), out(1, C)
    _ok(lib, lib.prego_debug_vit_head_bwd(_vp(x.ptr()), _vp(Guarded(a["dl"]).ptr()), B, N, E, C, _vp(dev(a["lnw"])), _vp(dev(a["lnb"])), _vp(dev(a["hw"])),
                                          _vp(dx.ptr()), _vp(scratch.ptr()), _vp(g_lnw.ptr()), _vp(g_lnb.ptr()), _vp(g_hw.ptr()), _vp(g_hb.ptr()), _s()))
    ref, bound = rx.head_bwd_ref(a)
    assert rx.sum_is_exact(a["dl"][:, :, None] * a["hw"][None], 1.0, 1) and rx.sum_is_exact(ref["dy"], 1.0, 0)
    assert scratch.canary_elsewhere()
    rx.assert_exact(scratch.block()[2 * B:].cpu(), rx.t32(ref["dy"]), "dy = dlogits hw")
    exact(g_lnb, ref["g_lnb"][None], "g_lnb")
    exact(g_hb, ref["g_hb"][None], "g_hb")
    within(g_lnw, ref["g_lnw"][None], bound["g_lnw"][None], "g_lnw")
    within(g_hw, ref["g_hw"], bound["g_hw"], "g_hw")
    assert dx.canary_elsewhere()
    got = dx.block().view(B, N, E)
    assert bool((got[:, 1:] == 7.25).all()), "a dx row of tokens 1 .. N-1 was written"
    rx.assert_within(np64(got[:, 0]), ref["dx"], bound["dx"], "dx of token 0")


def test_vit_head_refuses_what_does_not_fit_its_lds():
    lib = _lib()
    z, o = torch.zeros(512, device="cuda"), out(1, 8)
    assert lib.prego_debug_vit_head(_vp(z), 1, 1, 512, _vp(z), _vp(z), _vp(z), _vp(z), 16384, _vp(o.ptr()), None, _s()) == PREGO_EINVAL
    assert lib.prego_debug_vit_head_bwd(*([_vp(z)] * 2), 1, 1, 512, 16384, *([_vp(z)] * 3), *([_vp(o.ptr())] * 6), _s()) == PREGO_EINVAL
    torch.cuda.synchronize()
    assert o.untouched()


# ================================================================================================ tokens
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 8])
@pytest.mark.parametrize("E", [512, 1536])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_vit_tokens_and_backward_exact_with_one_mask(B, T, E, p):
    """forward: one rounded addition (+ one rounded product under dropout) per element: bit-exact.  backward on small integers: denc rows
    bit-exact (the forward's mask at the same element index), g_pe / g_cls exact sums at p = 0, within (B + 1) U sum_b |v| at p = 0.1 (the
    scaled values are no integers then; largest err / bound there on an MI355X, ROCm 7.2, 2026-10-21: 0.12)."""
    lib = _lib()
    g = _gen(B, T, E)
    enc, cls, pe = (g.standard_normal(s).astype(np.float32) for s in ((B * T, E), (E,), (T + 1, E)))
    x = out(B * (T + 1), E)
    _ok(lib, lib.prego_debug_vit_tokens(_vp(Guarded(enc).ptr()), _vp(dev(cls)), _vp(Guarded(pe).ptr()), B, T, E, _vp(x.ptr()), p, SEED, _s()))
    exact(x, torch.from_numpy(rx.tokens_ref(enc, cls, pe, B, T, E, p, SEED)).view(-1, E), "token rows")
    dx64 = 4.0 * g.integers(-8, 9, (B * (T + 1), E))
    denc, g_pe, g_cls = out(B * T, E), out(T + 1, E), out(1, E)
    _ok(lib, lib.prego_debug_vit_tokens_bwd(_vp(Guarded(dx64).ptr()), B, T, E, _vp(denc.ptr()), _vp(g_pe.ptr()), _vp(g_cls.ptr()), p, SEED, _s()))
    w_enc, w_pe, w_cls = rx.tokens_bwd_ref(dx64, B, T, E, p, SEED)
    kept = rx.keep_mask(SEED, 0, dx64.size, p).reshape(B, T + 1, E)
    v32 = np.where(kept, dx64.reshape(B, T + 1, E).astype(np.float32) * rx.drop_scale(p), np.float32(0))
    exact(denc, torch.from_numpy(v32[:, :T].reshape(B * T, E)), "denc")
    if p == 0:
        exact(g_pe, w_pe, "g_pe")
        exact(g_cls, w_cls[None], "g_cls")
    else:
        b_pe = (B + 1) * rx.U * np.abs(v32.astype(np.float64)).sum(0) + 2 * rx.U * np.abs(w_pe)
        within(g_pe, w_pe, b_pe, "g_pe")
        within(g_cls, w_cls[None], b_pe[T][None], "g_cls")
        rx.assert_exact(g_cls.block().cpu(), g_pe.block()[T:].cpu(), "g_cls is g_pe's last row")


# ================================================================================================ loss
def _loss_problem(lens, C, g):
    n = len(lens)
    l = [g.standard_normal((T, C)).astype(np.float32) * 3 for T in lens]
    t = [(g.random((T, C)) < 0.2).astype(np.float32) for T in lens]
    for i in range(n):
        t[i][-1, g.integers(0, C)] = 1.0
    if n > 1:
        t[1][-1] = 0.0                                       # an all-zero target row: contributes nothing, gradient exactly zero
    if n > 2 and C > 2:
        t[2][-1, :3] = 1.0                                   # multi-label
        l[2][-1, 0], l[2][-1, 1] = 80.0, -80.0
    return l, t


def _check_loss(loss, dls, l, t, lens, C, gs, reduction):
    ref, dl, d_loss, d_dl = rx.oad_loss_ref(np.stack([x[-1] for x in l]).astype(np.float64), np.stack([x[-1] for x in t]).astype(np.float64), gs, reduction)
    rx.assert_within(np.array([float(loss)]), np.array([ref]), np.array([d_loss]), "loss")
    for i, T in enumerate(lens):
        assert dls[i].canary_elsewhere(), "dlogits written past T x C"
        got = np64(dls[i].block())
        assert (got[:T - 1] == 0).all() and not np.signbit(got[:T - 1]).any(), "the T - 1 leading rows are exactly zero"
        rx.assert_within(got[T - 1], dl[i], d_dl[i], f"dlogits of clip {i}")
    if len(lens) > 1:
        assert (np64(dls[1].block())[-1] == 0).all()


@pytest.mark.parametrize("C", [1, 63, 64, 65, 128])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_oad_loss_uniform_through_the_engine(C, n):
    """prego_amd.engine.oad_loss, both reductions, grad_scale 128; value and dlogits against fp64 with rows_exact.oad_loss_ref's bounds.
    Largest err / bound on an MI355X (gfx950, ROCm 7.2, 2026-10-21): loss 2.8e-2, dlogits 0.18 (ragged lengths: 4.0e-2 and 0.12; the
    serial path: 1.3e-3 and 0.13)."""
    from prego_amd import engine
    T = 1 + (C + n) % 3
    l, t = _loss_problem([T] * n, C, _gen(C, n))
    for reduction in ("mean", "sum"):
        loss, dl = engine.oad_loss(torch.from_numpy(np.stack(l)).cuda(), torch.from_numpy(np.stack(t)).cuda(), True, 128.0, reduction)
        torch.cuda.synchronize()
        ref, rdl, d_loss, d_dl = rx.oad_loss_ref(np.stack([x[-1] for x in l]).astype(np.float64), np.stack([x[-1] for x in t]).astype(np.float64), 128.0,
                                                 reduction)
        rx.assert_within(np.array([float(loss)]), np.array([ref]), np.array([d_loss]), f"loss {reduction}")
        got = np64(dl)
        assert (got[:, :T - 1] == 0).all()
        rx.assert_within(got[:, T - 1], rdl, d_dl, f"dlogits {reduction}")


def _loss_tables(l, t, lens, C):
    lg, tg = [Guarded(x) for x in l], [Guarded(x) for x in t]
    dls = [out(T, C) for T in lens]
    return lg, tg, dls


@pytest.mark.parametrize("C", [3, 86, 128])
def test_oad_loss_ragged_lengths(C):
    """ragged T including T = 1, through prego_oad_loss_reduce; nothing past T x C of a clip's dlogits is written"""
    lib = _lib()
    lens = [4, 1, 7, 2, 1]
    l, t = _loss_problem(lens, C, _gen(C))
    lg, tg, dls = _loss_tables(l, t, lens, C)
    from prego_amd._lib import ptr_array
    for red in (0, 1):
        loss = torch.zeros((), device="cuda")
        _ok(lib, lib.prego_oad_loss_reduce(len(lens), (ct.c_int32 * len(lens))(*lens),
                                           ptr_array([x.ptr() for x in lg]), ptr_array([x.ptr() for x in tg]), C, red, _vp(loss),
                                           ptr_array([x.ptr() for x in dls]), 128.0, _s()))
        _check_loss(loss, dls, l, t, lens, C, 128.0, "sum" if red else "mean")


def test_oad_loss_serial_path_4097_clips_and_the_product_entry_limit():
    """more clips than the kernel's LDS table holds (4096): one wave walks all clips.  The product entry (and so engine.oad_loss) refuses
    4097 clips before any launch - it stages at most 4096 - so the path is reached through prego_debug_oad_loss on device tables."""
    lib = _lib()
    from prego_amd import engine
    from prego_amd._lib import PregoError
    n, Cn = 4097, 3
    g = _gen(4097)
    l = g.standard_normal((n, 1, Cn)).astype(np.float32) * 3
    t = (g.random((n, 1, Cn)) < 0.5).astype(np.float32)
    L, Tt = torch.from_numpy(l).cuda(), torch.from_numpy(t).cuda()
    with pytest.raises(PregoError):
        engine.oad_loss(L, Tt, True, 1.0, "mean")
    dl = out(n, Cn)
    step = Cn * 4
    mk = lambda base: torch.arange(n, dtype=torch.int64, device="cuda") * step + base      # noqa: E731
    loss = out(1, 1)
    lens = torch.ones(n, dtype=torch.int32, device="cuda")
    for red in (0, 1):
        _ok(lib, lib.prego_debug_oad_loss(_vp(mk(L.data_ptr())), _vp(mk(Tt.data_ptr())), _vp(lens), n, Cn, red, _vp(loss.ptr()), _vp(mk(dl.ptr())), 128.0, _s()))
        ref, rdl, d_loss, d_dl = rx.oad_loss_ref(l[:, 0].astype(np.float64), t[:, 0].astype(np.float64), 128.0, "sum" if red else "mean")
        assert loss.canary_elsewhere() and dl.canary_elsewhere()
        rx.assert_within(np64(loss.block()), np.array([[ref]]), np.array([[d_loss]]), "loss, serial path")
        rx.assert_within(np64(dl.block()), rdl, d_dl, "dlogits, serial path")


def test_oad_loss_refuses_129_classes():
    from prego_amd import engine
    from prego_amd._lib import PregoError
    with pytest.raises(PregoError):
        engine.oad_loss(torch.zeros(2, 1, 129, device="cuda"), torch.zeros(2, 1, 129, device="cuda"))
    lib = _lib()
    z = torch.zeros(8, dtype=torch.int64, device="cuda")
    assert lib.prego_debug_oad_loss(_vp(z), _vp(z), _vp(z), 1, 129, 0, _vp(z), None, 1.0, _s()) == PREGO_EINVAL


# ================================================================================================ AdamW
_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.05)


def _adamw_call(lib, P, G, M, V, step):
    from prego_amd._lib import ptr_array
    n = len(P)
    numel = (ct.c_int64 * n)(*[int(p.numel()) for p in P])
    return lib.prego_adamw_step(n, ptr_array([p.data_ptr() for p in P]), ptr_array([g.data_ptr() for g in G]), ptr_array([m.data_ptr() for m in M]),
                                ptr_array([v.data_ptr() for v in V]), numel, step, _HP["lr"], _HP["b1"], _HP["b2"], _HP["eps"], _HP["wd"], _s())


def test_adamw_two_steps_within_derived_bound():
    """25 tensors in one call (two launches of at most 24): sizes 1, 3, 4, 4095, 4096, 4097, 8193 (partial last vectors, more than one
    workgroup), one tensor that is a view starting one float into its storage (not 16-byte aligned: the scalar path), the rest small.  Each
    step is checked against fp64 from the fp32 state the step started from (rows_exact.adamw_ref), step 2 from the device's own step-1
    state, so a wrong bias correction at step 2 shows.  Nothing behind a tensor's last element is written.
    Largest err / bound on an MI355X (gfx950, ROCm 7.2, 2026-10-21): p 0.14, m 0.30, v 0.32."""
    lib = _lib()
    g = _gen(25)
    sizes = [1, 3, 4, 4095, 4096, 4097, 8193, 4100] + [5 + i for i in range(17)]
    assert len(sizes) == 25

    def alloc(n, k, fill):
        o = gx.make_output(1, n, n + 12, torch.float32, "cuda")
        off = 1 if k == 7 else 0                      # tensor 7: a view one float into its storage
        view = o.buf[o.off + off:o.off + off + n]
        view[:] = fill
        return o, view

    store, P, G, M, V = [], [], [], [], []
    for k, n in enumerate(sizes):
        for lst, fill in ((P, dev(g.standard_normal(n))), (G, dev(g.standard_normal(n))), (M, torch.zeros(n, device="cuda")), (V, torch.zeros(n, device="cuda"))):
            o, v = alloc(n, k, fill)
            store.append((o, k, n))
            lst.append(v)
    assert P[7].data_ptr() % 16 == 4 and P[4].data_ptr() % 16 == 0
    for step in (1, 2):
        before = [[np64(x[k]) for k in range(25)] for x in (P, G, M, V)]
        if step == 2:
            for k in range(25):
                G[k][:] = dev(g.standard_normal(sizes[k]))
            before[1] = [np64(x) for x in G]
        _ok(lib, _adamw_call(lib, P, G, M, V, step))
        for k in range(25):
            p2, m2, v2, d_p, d_m, d_v = rx.adamw_ref(before[0][k], before[1][k], before[2][k], before[3][k], step, **_HP)
            rx.assert_within(np64(P[k]), p2, d_p, f"step {step} tensor {k} p")
            rx.assert_within(np64(M[k]), m2, d_m, f"step {step} tensor {k} m")
            rx.assert_within(np64(V[k]), v2, d_v, f"step {step} tensor {k} v")
    canary = gx._signed(gx.CANARY32, 32)
    for o, k, n in store:
        off = 1 if k == 7 else 0
        bits = o.buf.view(torch.int32)
        assert bool((bits[:o.off + off] == canary).all()) and bool((bits[o.off + off + n:] == canary).all()), f"tensor {k}: written outside its {n} elements"


def test_adamw_refuses_a_pointer_that_is_not_float_aligned():
    lib = _lib()
    P, G, M, V = (torch.ones(16, device="cuda") for _ in range(4))
    from prego_amd._lib import ptr_array
    numel = (ct.c_int64 * 1)(8)
    rc = lib.prego_adamw_step(1, ptr_array([P.data_ptr() + 2]), ptr_array([G.data_ptr()]), ptr_array([M.data_ptr()]), ptr_array([V.data_ptr()]), numel, 1,
                              _HP["lr"], _HP["b1"], _HP["b2"], _HP["eps"], _HP["wd"], _s())
    torch.cuda.synchronize()
    assert rc == PREGO_EINVAL and bool((P == 1).all()) and bool((M == 1).all()) and bool((V == 1).all())
