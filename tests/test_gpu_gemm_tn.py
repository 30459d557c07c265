"""GPU tests of the training GEMMs on k-major operands (csrc/gemm_tn.hip) through prego_debug_gemm_tn, which calls launch_gemm_bf16_tn as
the training steps do: every weight, bias and input gradient of the bf16 training steps, and the keeping forward's projections.

The sharp test is exact: integer operands for which fp32 accumulation is exact in any order (tests/helpers/gemm_exact.py; the claim is
checked on the CPU in tests/test_gemm_reference_cpu.py), so EVERY element of C, C16 and colsum_out must equal the fp64 result bit for
bit, whichever of the seven instantiations runs.  Outputs lie in canary-filled allocations (an unwritten or over-written element
shows), operands carry NaN wherever the launcher's contract (csrc/kernels.h) says nothing reaches a stored output.

The second test uses real-valued operands against fp64 with the worst-case bound of gemm_exact.error_bound: a backstop for realistic
exponents.  Largest err / bound seen on an MI355X: see test_tn_real_valued_within_derived_bound."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.helpers import gemm_exact as gx  # noqa: E402

PREGO_EINVAL = -1


def _lib():
    from prego_amd import _lib
    return _lib.load_debug()


def _vp(x):
    return C.c_void_p(x if isinstance(x, int) else (x.data_ptr() if x is not None else None))


def _call(lib, case, p, out32, out16, colsum, ta=None, tb=None, K=None, k_valid=None, lda=None):
    d_lda, ldb = case.ld()
    rc = lib.prego_debug_gemm_tn(case.ta if ta is None else ta, case.tb if tb is None else tb, _vp(p.A.ptr()), d_lda if lda is None else lda,
                                 _vp(p.B.ptr()), ldb, _vp(p.bias), _vp(out32.ptr()), _vp(out16.ptr() if out16 is not None else None),
                                 out32.ldc, case.M, case.N, case.K if K is None else K, case.k_valid if k_valid is None else k_valid,
                                 _vp(colsum.ptr() if colsum is not None else None), _vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _outputs(case):
    ldc = gx.round_up(case.N, 8) + 8
    out32 = gx.make_output(case.M, case.N, ldc, torch.float32, "cuda")
    out16 = gx.make_output(case.M, case.N, ldc, torch.bfloat16, "cuda") if case.c16 else None
    colsum = gx.make_output(1, case.M, gx.round_up(case.M, 8) + 8, torch.float32, "cuda") if case.colsum else None
    return out32, out16, colsum


@pytest.mark.parametrize("case", gx.TN_CASES, ids=lambda c: c.id())
def test_tn_exact_integer(case):
    lib = _lib()
    p = gx.make_tn(case, "int", torch.bfloat16, "cuda", seed=case.M + case.N + case.K)
    ref, _, ref_cs = p.reference()
    out32, out16, colsum = _outputs(case)
    rc = _call(lib, case, p, out32, out16, colsum)
    if case.refused():           # more than 256 tiles of a row-major B: not this launcher's shape (launch_gemm_bf16_nt falls through; tests/test_gpu_gemm.py)
        assert rc == PREGO_EINVAL and out32.untouched()
        return
    assert rc == 0, lib.prego_last_error()
    if case.c16:
        assert out32.untouched(), "C16 given: the fp32 C must not be written"
        got, want, out = out16.block(), gx.expected_bf16(ref), out16
    else:
        got, want, out = out32.block(), ref.to(torch.float32), out32
    assert out.canary_elsewhere(), "an element outside the M x N block was written"
    assert bool(torch.isfinite(got).all()), f"unwritten or non-finite outputs: {gx.first_mismatches(got, want)}"
    assert gx.bits_equal(got, want), gx.first_mismatches(got, want)
    if case.colsum:
        assert colsum.canary_elsewhere(), "colsum_out written outside [0, M)"
        got_cs, want_cs = colsum.block(), ref_cs.to(torch.float32)[None]
        assert gx.bits_equal(got_cs, want_cs), gx.first_mismatches(got_cs, want_cs)


@pytest.mark.parametrize("case", gx.TN_REAL, ids=lambda c: c.id())
def test_tn_real_valued_within_derived_bound(case):
    """|got - ref| <= K 2^-23 (sum_k |a_k b_k| + |bias|) per element (+ one bf16 ulp for C16); colsum_out against K 2^-23 sum_k |a_k|.
    Largest err / bound observed on an MI355X (gfx950, ROCm 7.2), over all cases of each operand form:
    wgrad 1.1e-2 (K = 64, k_valid = 16; 4.9e-3 and below at the larger K), colsum_out 2.1e-4; dgrad 1.5e-4 with fp32 C and 0.49 with C16
    (there the bf16 ulp is nearly all of the bound, and rounding to nearest uses up to half of it); row-major split-K 2.9e-3."""
    lib = _lib()
    p = gx.make_tn(case, "real", torch.bfloat16, "cuda", seed=case.M + case.N + case.K + 1)
    ref, mag, ref_cs = p.reference()
    out32, out16, colsum = _outputs(case)
    assert _call(lib, case, p, out32, out16, colsum) == 0, lib.prego_last_error()
    out = out16 if case.c16 else out32
    assert out.canary_elsewhere()
    got = out.block().to(torch.float64)
    bound = gx.error_bound_bf16(case.K, ref, mag) if case.c16 else gx.error_bound(case.K, mag)
    ratio = ((got - ref).abs() / bound).max()
    print(f"{case.id()}: max err / bound = {float(ratio):.3e}")
    assert bool(torch.isfinite(got).all()) and float(ratio) <= 1.0
    if case.colsum:
        assert colsum.canary_elsewhere()
        got_cs = colsum.block()[0].to(torch.float64)
        r_cs = ((got_cs - ref_cs).abs() / gx.error_bound(case.K, p.a.abs().sum(dim=1))).max()
        print(f"{case.id()}: colsum max err / bound = {float(r_cs):.3e}")
        assert bool(torch.isfinite(got_cs).all()) and float(r_cs) <= 1.0


# what launch_gemm_bf16_tn refuses before any launch (gemm_tn.hip: the two `return -1` lines above the first kernel launch); every buffer
# is valid and fully allocated for the LARGEST shape named anyway
_REFUSALS = [
    ("K % 64 != 0", gx.TnCase(1, 1, 128, 128, 128, 128), dict(K=96, k_valid=96)),
    ("ta && !tb", gx.TnCase(1, 1, 128, 128, 128, 128), dict(tb=0)),
    ("colsum_out with !ta", gx.TnCase(0, 1, 128, 128, 128, 128, colsum=True), {}),
    ("lda % 8 != 0", gx.TnCase(1, 1, 100, 128, 128, 128, 112), dict(lda=108)),
    ("!tb: K = 64", gx.TnCase(0, 0, 128, 128, 128, 128), dict(K=64, k_valid=64)),
    ("!tb: 257 tiles", gx.TnCase(0, 0, 128, 257 * 128, 128, 128), {}),
    ("!tb: k_valid != K", gx.TnCase(0, 0, 128, 128, 128, 128), dict(k_valid=127)),
]


@pytest.mark.parametrize("why,case,override", _REFUSALS, ids=[r[0] for r in _REFUSALS])
def test_tn_refusals_launch_nothing(why, case, override):
    lib = _lib()
    p = gx.make_tn(case, "int", torch.bfloat16, "cuda", seed=1)
    out32, out16, colsum = _outputs(case)
    assert _call(lib, case, p, out32, out16, colsum, **override) == PREGO_EINVAL, why
    assert b"unsupported shape" in lib.prego_last_error()
    assert out32.untouched() and (colsum is None or colsum.untouched()), f"{why}: refused, yet the output was written"
