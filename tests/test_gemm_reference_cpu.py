"""The arithmetic the kernel-level GEMM tests rest on (tests/helpers/gemm_exact.py), checked without a GPU on every case of their
lists that is small enough for the CPU:
  (a) an fp32 CPU matmul of the integer operands equals the fp64 reference bit for bit, and the operands survive bf16 and fp16;
  (b) an fp32 CPU matmul of the real-valued operands stays inside the derived error bound;
  (c) guards and poison are where the helper says: a numpy emulation of the kernel's contract on the raw storage reproduces the
      reference, one that ignores k_valid or a column limit runs into the NaN;
  (d) the exact test cannot pass vacuously: >= 90 % of the integer operands have a non-zero low byte in bf16, and >= 90 % of the expected
      bf16 outputs differ from their fp32 source."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests.helpers import gemm_exact as gx  # noqa: E402

CPU_MAX_MNK = 2 ** 29          # a case above this is left to the GPU tests


def _small(cases):
    return [c for c in cases if c.M * c.N * c.K <= CPU_MAX_MNK]


TN_SMALL = _small(gx.TN_CASES)
NT_SMALL = sorted({s for s in gx.NT_VARIANT_SHAPES + gx.NT_DISPATCH + gx.NT_TRAIN_SPLITK if s[0] * s[1] * s[2] <= CPU_MAX_MNK})


def test_case_lists_cover_what_they_claim():
    assert len(TN_SMALL) >= 25 and len(NT_SMALL) >= 15
    tiles = {c.tiles() for c in gx.TN_WGRAD}
    assert {1, 3, 9, 15, 255, 256, 257, 272} <= tiles                       # xcd_remap at counts that are not multiples of 8; the launcher's boundary
    for c in gx.TN_CASES + gx.TN_REAL:
        lda, ldb = c.ld()
        assert lda % 8 == 0 and ldb % 8 == 0 and c.K % 64 == 0 and 0 < c.k_valid <= c.K
        assert lda >= (c.M if c.ta else c.K) and ldb >= (c.N if c.tb else c.K)
        # what launch_gemm_bf16_tn refuses is not among the cases that must compute - but for the one projection of the keeping forward
        # that has more than 256 tiles: there the refusal is asserted, and the dispatcher's fall-through computes
        assert c.refused() == ((c.ta, c.tb, c.M, c.N, c.K) == (0, 0, 2048, 3072, 1024))
        assert not c.colsum or c.ta


def test_r_of_k():
    assert [gx.r_of_k(K) for K in (64, 1024, 1088, 4096, 4352, 16384)] == [127, 127, 63, 63, 31, 31]
    for K in (64, 192, 1024, 1088, 3072, 4096):
        r = gx.r_of_k(K)
        assert r * r * K + r < 2 ** 24
        assert r == 127 or (2 * r + 1) ** 2 * K + 2 * r + 1 >= 2 ** 24        # the next larger range would not do


def test_canaries_are_nans_no_arithmetic_produces():
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        out = gx.make_output(5, 7, 16, dt)
        assert torch.isnan(out.buf).all() and out.untouched() and out.canary_elsewhere()
        plain = torch.full((1,), float("nan"), dtype=dt)
        assert not gx.bits_equal(out.buf[:1], plain)                             # told from a NaN that was computed and stored
        assert out.buf.numel() == (2 * gx.GUARD + 5) * 16 and out.off == gx.GUARD * 16
        out.block().fill_(1.0)
        assert out.canary_elsewhere() and not out.untouched() and torch.isfinite(out.block()).all()
        for (i, j) in ((gx.GUARD - 1, 0), (gx.GUARD, 7), (gx.GUARD + 5, 6), (2 * gx.GUARD + 4, 15)):      # one element past the block on every side
            o2 = gx.make_output(5, 7, 16, dt)
            o2.buf.view(-1, 16)[i, j] = 0.0
            assert not o2.canary_elsewhere()


@pytest.mark.parametrize("case", TN_SMALL, ids=lambda c: c.id())
def test_tn_integer_operands_make_fp32_exact(case):
    p = gx.make_tn(case, "int", seed=case.M + case.N + case.K)
    ref, mag, colsum = p.reference()
    r = gx.r_of_k(case.K)
    for x in (p.a, p.b):                                                          # (a) exact in both 16-bit types
        assert float(x.abs().max()) <= r
        assert torch.equal(x.to(torch.bfloat16).to(torch.float64), x) and torch.equal(x.to(torch.float16).to(torch.float64), x)
    bias32 = p.bias if p.bias is not None else torch.zeros(case.N)
    got32 = p.a.to(torch.float32) @ p.b.to(torch.float32) + bias32
    assert gx.bits_equal(got32, ref.to(torch.float32)) and torch.equal(got32.to(torch.float64), ref)
    assert float(mag.max()) < 2 ** 24 and torch.equal(colsum.to(torch.float32).to(torch.float64), colsum)
    # (c) the storage: honouring the contract reproduces the reference, ignoring any part of it meets the poison
    af, bf = p.A.flat64(), p.B.flat64()
    bias = None if p.bias is None else p.bias.double().numpy()
    assert np.array_equal(gx.emulate_tn(case, af, bf, bias), ref.numpy())
    lda, ldb = case.ld()
    if case.k_valid < case.K:
        assert np.isnan(gx.emulate_tn(case, af, bf, bias, honour_k_valid=False)).all()
    wide = gx.emulate_tn(case, af, bf, bias, honour_columns=False)
    assert np.array_equal(wide[:case.M, :case.N], ref.numpy())
    if case.ta and lda > case.M:
        assert np.isnan(wide[case.M:]).all()
    if case.tb and ldb > case.N:
        assert np.isnan(wide[:, case.N:]).all()
    for op, rows, width in ((p.A, p.A.rows, case.M if case.ta else case.K), (p.B, p.B.rows, case.N if case.tb else case.K)):
        v = op.buf.view(-1, op.ld)
        assert v.shape[0] == rows + 2 * gx.GUARD and op.off == gx.GUARD * op.ld
        assert torch.isnan(v[:gx.GUARD]).all() and torch.isnan(v[gx.GUARD + rows:]).all() and torch.isnan(v[:, width:]).all()
    for op, kmajor in ((p.A, case.ta), (p.B, case.tb)):
        v = op.buf.view(-1, op.ld)[gx.GUARD:gx.GUARD + op.rows]
        if kmajor:
            assert torch.isnan(v[case.k_valid:]).all() and torch.isfinite(v[:case.k_valid, :(case.M if op is p.A else case.N)]).all()
        else:
            assert torch.isfinite(v[:, :case.K]).all() and bool((v[:, case.k_valid:case.K] == 0).all())
    # (d) not vacuous
    if p.a.numel() >= 4096:
        assert gx.low_byte_nonzero_fraction(p.a) >= 0.90 and gx.low_byte_nonzero_fraction(p.b) >= 0.90
    if case.c16:
        e16 = gx.expected_bf16(ref)
        assert torch.equal(ref.to(torch.bfloat16), e16)                           # torch's fp64 -> bf16 is the same single RNE rounding
        assert float((e16.to(torch.float64) != ref).double().mean()) >= 0.90


@pytest.mark.parametrize("case", _small(gx.TN_REAL), ids=lambda c: c.id())
def test_tn_real_operands_fp32_inside_bound(case):
    p = gx.make_tn(case, "real", seed=case.M + case.N + case.K + 1)
    ref, mag, _ = p.reference()
    assert float(p.a.abs().max()) <= 1 and torch.equal(p.a.to(torch.bfloat16).to(torch.float64), p.a)
    bias32 = p.bias if p.bias is not None else torch.zeros(case.N)
    got = (p.a.to(torch.float32) @ p.b.to(torch.float32) + bias32).to(torch.float64)
    bound = gx.error_bound(case.K, mag)
    assert bool(((got - ref).abs() <= bound).all())
    assert float(((got - ref).abs() / bound).max()) > 0                          # and the comparison is not between two copies of one number
    got16 = got.to(torch.float32).to(torch.bfloat16).to(torch.float64)
    assert bool(((got16 - ref).abs() <= gx.error_bound_bf16(case.K, ref, mag)).all())
    assert not bool(((got16 - ref).abs() <= bound).all())                        # the bf16 rounding needs its ulp: the fp32 bound alone is too tight for it


@pytest.mark.parametrize("M,N,K", NT_SMALL)
@pytest.mark.parametrize("dtype16", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_nt_integer_operands_make_fp32_exact(M, N, K, dtype16):
    p = gx.make_nt(M, N, K, "int", dtype16, seed=M + N + K, lda=K + 8, ldb=K + 16)
    ref, mag = p.reference()
    for x in (p.a, p.b):
        assert torch.equal(x.to(dtype16).to(torch.float64), x)
    got32 = p.a.to(torch.float32) @ p.b.to(torch.float32).T + p.bias
    assert gx.bits_equal(got32, ref.to(torch.float32)) and torch.equal(got32.to(torch.float64), ref) and float(mag.max()) < 2 ** 24
    for op, R in ((p.A, M), (p.B, N)):
        v = op.buf.view(-1, op.ld)
        assert torch.isnan(v[:gx.GUARD]).all() and torch.isnan(v[gx.GUARD + R:]).all() and torch.isnan(v[:, K:]).all()
        assert torch.equal(v[gx.GUARD:gx.GUARD + R, :K].to(torch.float64), p.a if op is p.A else p.b)
        flat = op.flat64()                                                       # what the kernel's pointer and leading dimension address
        assert np.array_equal(flat[:R * op.ld].reshape(R, op.ld)[:, :K], (p.a if op is p.A else p.b).numpy())
    assert gx.low_byte_nonzero_fraction(p.a) >= 0.90 and gx.low_byte_nonzero_fraction(p.b) >= 0.90


def test_nt_real_fp16_operands_fp32_inside_bound():
    M, N, K = 300, 256, 1088
    p = gx.make_nt(M, N, K, "real", torch.float16, seed=7)
    ref, mag = p.reference()
    assert float(p.a.abs().max()) <= 1 and torch.equal(p.a.to(torch.float16).to(torch.float64), p.a)
    got = (p.a.to(torch.float32) @ p.b.to(torch.float32).T + p.bias).to(torch.float64)
    assert bool(((got - ref).abs() <= gx.error_bound(K, mag)).all())


def test_bf16_ulp():
    x = torch.tensor([1.0, 1.5, 1.9999, 2.0, 255.0, 256.0, 3e-3], dtype=torch.float64)
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 1.0, 2.0, 2.0 ** -16], dtype=torch.float64)
    assert torch.equal(gx.bf16_ulp(x), want)
    y = torch.tensor([1.0, 256.0], dtype=torch.bfloat16)                         # the neighbour above is exactly one ulp away
    nxt = (y.view(torch.int16) + 1).view(torch.bfloat16)
    assert torch.equal((nxt.double() - y.double()), gx.bf16_ulp(y.double()))
