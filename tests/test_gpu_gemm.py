"""GPU tests of the projection GEMM kernels through the C ABI's measurement hook (prego_debug_gemm_bf16): the production
ping-pong kernel against the plain 128x128 kernel (bit-exact: same MFMA instruction, same
ascending-k accumulation order) and against an fp32 torch matmul of the same bf16 operands (tolerance), on ragged M, the
minimum K, and a grid larger than the chip.  Below that: every bf16 variant, the production dispatcher launch_gemm_bf16_nt at its
thresholds (bf16 and fp16, through prego_debug_gemm_nt) and the training flag's branch, exactly against fp64."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.helpers import gemm_exact as gx  # noqa: E402


def _gemm(lib, variant, A, B, bias, M, N, K):
    out = torch.full((M, N), float("nan"), device="cuda")
    rc = lib.prego_debug_gemm_bf16(variant, C.c_void_p(A.data_ptr()), C.c_void_p(B.data_ptr()), C.c_void_p(bias.data_ptr()),
                                   C.c_void_p(out.data_ptr()), M, N, K, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.prego_last_error()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (4113, 512, 1024), (70001, 256, 192), (65536, 2048, 256)])
def test_pingpong_gemm_matches_plain_kernel_and_fp32(M, N, K):
    from prego_amd import _lib
    lib = _lib.load_debug()          # kernel-level hook prego_debug_gemm_bf16: only in libprego_amd_debug.so
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    A = (torch.rand((M, K), device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
    B = (torch.rand((N, K), device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
    bias = torch.randn((N,), device="cuda", generator=g)
    plain = _gemm(lib, 0, A, B, bias, M, N, K)            # 128x128 two-stage kernel
    for variant in (12,):                                 # ping-pong (production)
        got = _gemm(lib, variant, A, B, bias, M, N, K)
        assert not torch.isnan(got).any(), f"variant {variant}: unwritten output elements"
        assert torch.equal(got, plain), f"variant {variant}: differs from the plain kernel, max {float((got - plain).abs().max()):.3e}"
    rows = torch.randint(0, M, (256,), device="cuda", generator=g)
    ref = A[rows].float() @ B.float().T + bias
    assert float((plain[rows] - ref).abs().max()) < 2e-3 * (K ** 0.5)      # fp32 accumulation of K products in [-1, 1]


# ---- exact comparisons against fp64 (tests/helpers/gemm_exact.py): integer operands for which fp32 accumulation is exact in any order, so
# every element must equal the fp64 result bit for bit; outputs in canary-filled allocations, operands inside NaN-filled ones.  The
# method's own arithmetic is checked on the CPU in tests/test_gemm_reference_cpu.py.
def _vp(x):
    return C.c_void_p(x)


def _check_exact(out, ref, what):
    got, want = out.block(), ref.to(torch.float32)
    assert out.canary_elsewhere(), f"{what}: an element outside the M x N block was written"
    assert bool(torch.isfinite(got).all()), f"{what}: unwritten or non-finite outputs: {gx.first_mismatches(got, want)}"
    assert gx.bits_equal(got, want), f"{what}: {gx.first_mismatches(got, want)}"


@pytest.mark.parametrize("M,N,K,variants", [(M, N, K, (0, 1, 9, 12)) for (M, N, K) in gx.NT_VARIANT_SHAPES] + [(2048, 1024, 4096, (30,))])
def test_variants_exact_integer(M, N, K, variants):
    """variants 9 and 12 return without launching on a shape they do not take: the canary shows it"""
    from prego_amd import _lib
    lib = _lib.load_debug()
    p = gx.make_nt(M, N, K, "int", torch.bfloat16, "cuda", seed=M + N + K)
    ref, _ = p.reference()
    for variant in variants:
        out = gx.make_output(M, N, N, torch.float32, "cuda")          # the hook fixes lda = ldb = K, ldc = N
        rc = lib.prego_debug_gemm_bf16(variant, _vp(p.A.ptr()), _vp(p.B.ptr()), _vp(p.bias.data_ptr()), _vp(out.ptr()), M, N, K,
                                       _vp(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.prego_last_error()
        torch.cuda.synchronize()
        _check_exact(out, ref, f"variant {variant}")


def _dispatch(lib, f16, train_splitk, p, M, N, K):
    out = gx.make_output(M, N, N + 8, torch.float32, "cuda")
    rc = lib.prego_debug_gemm_nt(f16, train_splitk, _vp(p.A.ptr()), p.A.ld, _vp(p.B.ptr()), p.B.ld, _vp(p.bias.data_ptr()), _vp(out.ptr()), out.ldc,
                                 M, N, K, _vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.prego_last_error()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("f16", [0, 1], ids=["bf16", "f16"])
@pytest.mark.parametrize("M,N,K", gx.NT_DISPATCH)
def test_dispatcher_exact_integer_at_its_thresholds(M, N, K, f16):
    """launch_gemm_bf16_nt as production calls it, around M >= 2048 / M >= 4096, N % 256 and the ping-pong kernel's K >= 128"""
    from prego_amd import _lib
    lib = _lib.load_debug()
    p = gx.make_nt(M, N, K, "int", torch.float16 if f16 else torch.bfloat16, "cuda", seed=M + N + K + f16, lda=K + 8, ldb=K + 16)
    _check_exact(_dispatch(lib, f16, 0, p, M, N, K), p.reference()[0], f"f16 {f16}")


@pytest.mark.parametrize("M,N,K", gx.NT_TRAIN_SPLITK + [(2048, 3072, 1024)])
def test_dispatcher_train_splitk_exact_integer(M, N, K):
    """the keeping forward's flag: the split-K workgroup at K >= 1024 and at most 256 tiles; below that K, and above 256 tiles (the
    GRU input projection's 384 among them), the dispatcher must fall through to another kernel and still be exact"""
    from prego_amd import _lib
    lib = _lib.load_debug()
    p = gx.make_nt(M, N, K, "int", torch.bfloat16, "cuda", seed=M + N + K, lda=K + 8, ldb=K + 16)
    _check_exact(_dispatch(lib, 0, 1, p, M, N, K), p.reference()[0], "train_splitk")


def test_f16_real_valued_within_derived_bound():
    """fp16 operands uniform in [-1, 1] against fp64: |got - ref| <= K 2^-23 (sum_k |a_k b_k| + |bias|) per element, a worst-case bound
    (gemm_exact.error_bound).  Largest err / bound observed on an MI355X (gfx950, ROCm 7.2): 8.1e-4 (ping-pong kernel, K = 1024) and
    3.4e-3 (128 x 128 kernel, K = 192)."""
    from prego_amd import _lib
    lib = _lib.load_debug()
    for (M, N, K) in [(4113, 512, 1024), (300, 384, 192)]:        # the ping-pong kernel and the 128 x 128 kernel
        p = gx.make_nt(M, N, K, "real", torch.float16, "cuda", seed=M + N + K, lda=K + 8, ldb=K + 16)
        ref, mag = p.reference()
        out = _dispatch(lib, 1, 0, p, M, N, K)
        assert out.canary_elsewhere()
        got = out.block().to(torch.float64)
        ratio = ((got - ref).abs() / gx.error_bound(K, mag)).max()
        print(f"f16 {M}x{N}x{K}: max err / bound = {float(ratio):.3e}")
        assert bool(torch.isfinite(got).all()) and float(ratio) <= 1.0
