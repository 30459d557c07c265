"""Operands, references and bounds of the kernel-level GEMM tests (tests/test_gpu_gemm_tn.py, tests/test_gpu_gemm.py), and the case
lists they share with the CPU test of this module's own arithmetic (tests/test_gemm_reference_cpu.py).

The method.  A, B and bias are INTEGERS drawn uniformly from [-r, r], r = r(K) the largest of 127, 63, 31, 15 with r*r*K + r < 2^24.
They are exact in bf16 (8 significant bits) and in fp16, every product is an integer, and every partial sum in any order is an integer
below 2^24 in magnitude - exact in fp32 WHATEVER the summation order (split-K, the inside of an MFMA, two K groups joined through LDS).
A kernel with fp32 accumulation must therefore return the fp64 result bit for bit, in every element.

Around that, every buffer a kernel sees lies inside a larger allocation of this module:
  * outputs are filled with a NaN of a payload no arithmetic produces (CANARY32 / CANARY16): after the call exactly the M x N block
    is finite, and every other element - guard rows before and behind, the columns N .. ldc-1 - still holds the canary's bits;
  * operands carry NaN wherever the kernel's contract says nothing reaches a stored output: guard rows, the pad columns of the leading
    dimension, the k rows >= k_valid of a k-major operand.  The columns k_valid .. K-1 of a ROW-MAJOR A are zeros, not NaN: they are
    multiplied by rows the kernel zero-fills, and keeping them finite is the caller's part of the contract (csrc/kernels.h).
Nothing here reads outside its own allocations."""
from dataclasses import dataclass

import numpy as np
import torch

GUARD = 3                      # guard rows before and behind every operand / output
CANARY32 = 0x7FC0BEEF          # quiet NaNs with a payload: a NaN a kernel computed (0x7FC00000) is told from an unwritten element
CANARY16 = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01}


def r_of_k(K):
    """largest operand magnitude for which every partial sum of K products plus a bias stays an integer below 2^24"""
    for r in (127, 63, 31, 15):
        if r * r * K + r < 2 ** 24:
            return r
    raise ValueError(f"K = {K}: no integer range keeps fp32 accumulation exact")


def round_up(x, m):
    return (x + m - 1) // m * m


@dataclass(frozen=True)
class TnCase:
    """one call of launch_gemm_bf16_tn: C[M,N] = op(A) . op(B); ta: A stored [K][lda] else [M][lda]; tb: B stored [K][ldb] else [N][ldb]"""
    ta: int
    tb: int
    M: int
    N: int
    K: int
    k_valid: int
    lda: int = 0               # 0: the logical width rounded up to a multiple of 8
    ldb: int = 0
    colsum: bool = False
    c16: bool = False
    bias: bool = False

    def ld(self):
        lda = self.lda or round_up(self.M if self.ta else self.K, 8)
        ldb = self.ldb or round_up(self.N if self.tb else self.K, 8)
        return lda, ldb

    def tiles(self):
        return ((self.M + 127) // 128) * ((self.N + 127) // 128)

    def refused(self):
        """launch_gemm_bf16_tn takes a row-major B only from a row-major A, with all of K present, K >= 128 and at most 256 tiles"""
        return not self.tb and bool(self.ta or self.tiles() > 256 or self.K < 128 or self.k_valid != self.K)

    def id(self):
        lda, ldb = self.ld()
        return (f"{'T' if self.ta else 'N'}{'T' if self.tb else 'N'}-{self.M}x{self.N}x{self.K}kv{self.k_valid}-lda{lda}-ldb{ldb}"
                f"{'-colsum' if self.colsum else ''}{'-c16' if self.c16 else ''}{'-bias' if self.bias else ''}")


# (M, N, K, k_valid, lda, ldb, bias): wgrad, ta = tb = 1, each with and without colsum_out
_WGRAD = [
    (86, 1024, 64, 16, 128, 0, False),        # head wgrad of the 2 x 8 fixture: K = 64 forces the plain kernel, one ragged m-tile
    (86, 1024, 128, 65, 128, 0, False),       # split-K, the second K group's only tile holds one valid row
    (86, 1024, 192, 130, 128, 0, False),      # odd tile count: group 1 one tile, group 0 two; k_valid ends two rows into the last tile
    (86, 1024, 2048, 2048, 128, 0, False),    # the 16 x 128 training step's head wgrad
    (3072, 1024, 2048, 2040, 0, 0, False),    # 192 tiles, split-K, ntn = 8: only the n0 == 0 workgroups may write the bias gradient
    (2048, 2048, 192, 192, 2056, 0, False),   # 256 tiles: the last split-K launch
    (2049, 2048, 192, 192, 2056, 0, False),   # 272 tiles: the first plain one
    (3072, 4096, 128, 120, 0, 0, False),      # 768 tiles, plain kernel with a real K loop
    (200, 300, 320, 300, 208, 304, True),     # ragged in both, padded leading dimensions, NaN in the pad columns
    (1, 8, 64, 1, 8, 0, False),               # smallest: 1 tile
    (129, 129, 128, 128, 136, 136, False),    # one element past a tile in both directions
    (128, 384, 128, 128, 0, 0, False),        # 3 tiles   } xcd_remap at counts that are not multiples of 8: the canary shows a
    (300, 300, 192, 192, 0, 0, False),        # 9 tiles   } tile visited twice or never
    (381, 640, 128, 128, 0, 0, False),        # 15 tiles  }
    (1913, 2170, 128, 100, 0, 0, False),      # 255 tiles }
    (100, 32896, 128, 128, 0, 0, False),      # 257 tiles: plain
]
TN_WGRAD = [TnCase(1, 1, M, N, K, kv, lda, ldb, colsum=cs, bias=b) for (M, N, K, kv, lda, ldb, b) in _WGRAD for cs in (False, True)]

# dgrad, ta = 0, tb = 1, each with fp32 C and with C16
_DGRAD = [
    (16, 1024, 128, 96, 0, 0, False),         # head dgrad: B rows >= 96 zero-filled by the resource, A columns 96 .. 127 zeros
    (2048, 1024, 3072, 3072, 0, 0, False),    # 128 tiles, split-K  } the GRU / layer1 dgrads
    (2048, 4096, 3072, 3072, 0, 0, False),    # 512 tiles, plain    }
    (32800, 1024, 1024, 1024, 0, 0, False),   # ViTEnc's 32 windows x 1025 tokens: 2056 tiles, a ragged last m-tile of 32 rows
    (130, 200, 192, 192, 0, 208, True),       # ragged both
]
TN_DGRAD = [TnCase(0, 1, M, N, K, kv, lda, ldb, c16=c16, bias=b) for (M, N, K, kv, lda, ldb, b) in _DGRAD for c16 in (False, True)]

# row-major split-K, ta = tb = 0 (the keeping forward's projections), with bias.  (2048, 3072, 1024) - the GRU input projection - has 384
# tiles: the launcher refuses it and launch_gemm_bf16_nt falls through to the 256 x 128 kernel; the test asserts exactly that
TN_NT = [TnCase(0, 0, M, N, K, K, bias=True) for (M, N, K) in
         [(2048, 1024, 4096), (2048, 3072, 1024), (100, 136, 128), (2048, 2048, 192)]]
TN_CASES = TN_WGRAD + TN_DGRAD + TN_NT

# one real-valued case per operand form and kernel (split-K / plain)
TN_REAL = [TnCase(1, 1, 200, 300, 320, 300, 208, 304, colsum=True, bias=True), TnCase(1, 1, 86, 1024, 64, 16, 128, colsum=True),
           TnCase(1, 1, 3072, 1024, 2048, 2040, colsum=True), TnCase(1, 1, 2049, 2048, 192, 192, 2056),
           TnCase(0, 1, 2048, 1024, 3072, 3072), TnCase(0, 1, 2048, 4096, 3072, 3072, c16=True), TnCase(0, 1, 130, 200, 192, 192, 0, 208, c16=True, bias=True),
           TnCase(0, 0, 2048, 1024, 4096, 4096, bias=True), TnCase(0, 0, 100, 136, 128, 128, bias=True)]

# the NT family (tests/test_gpu_gemm.py)
NT_VARIANT_SHAPES = [(300, 256, 128), (4113, 512, 1024), (70001, 256, 192), (65536, 2048, 256)]      # prego_debug_gemm_bf16's shapes
NT_DISPATCH = [(M, N, K) for M in (2047, 2048, 4095, 4096, 4097) for N in (256, 384) for K in (64, 128, 1088)]      # launch_gemm_bf16_nt's thresholds
NT_TRAIN_SPLITK = [(2048, 1024, 1024), (2048, 1024, 960), (2048, 4096 + 128, 1024)]


# ---- which kernel an NT product ran on BEFORE the chooser existed (tests/test_gemm_dispatch_cpu.py): a transcription, function by
# function, of the launcher chain as it stood in the commit before gemm_nt_choose - gemm.hip (launch_gemm_bf16_nt, launch_gemm_bf16_nt_epi),
# gemm_pp.hip (launch_gemm_bf16_pingpong_epi / _mode / launch_gemm_bf16_pingpong), gemm_tn.hip (launch_gemm_bf16_tn) and the `proj` lambda
# of miniroad_forward.cpp.  It is the record of that chain: it is not to be brought into line with the chooser.
K128, K256X128, K256SQ, KPINGPONG, KSPLITK, KNONE = 0, 1, 2, 3, 4, -1                      # GemmNtKernel (csrc/kernels.h)
EPI_STORE, EPI_RESIDUAL, EPI_GELU_BF16, EPI_STORE_BF16, EPI_QKV, EPI_TOKENS = range(6)     # csrc/kernels.h
ENTRY_PLAIN, ENTRY_EPI, ENTRY_PROJ16 = 0, 1, 2                                             # GemmNtEntry (csrc/kernels.h)
KNOB_NO_BIG, KNOB_NO_SPLITK, KNOB_NO_PINGPONG = 1, 2, 4


def _old_tn_launches_nt(M, N, K, lda, ldb):
    """launch_gemm_bf16_tn(false, false, ..., k_valid = K, colsum_out = NULL) == 0"""
    if K % 64 or K <= 0 or M <= 0 or N <= 0 or lda % 8 or ldb % 8:
        return False
    ldmax = max(lda, ldb)
    if lda <= 0 or ldb <= 0 or K * ldmax * 2 > 0x7fffffff or M * lda * 2 > 0x7fffffff or (128 + 1) * ldmax * 2 + K * 2 > 0x7fffffff:
        return False
    ntm, ntn = (M + 127) // 128, (N + 127) // 128
    return not (ntm * ntn > 256 or K < 2 * 64)                   # the !tb branch; k_valid == K here


def _old_pingpong_epi_launches(N, K, has_bias, mode, dh, emb):
    """launch_gemm_bf16_pingpong_epi(...) == 0"""
    if N % 256 or K % 64 or K < 2 * 64 or (not has_bias and N > 8192):
        return False
    return not (mode == EPI_QKV and (dh % 8 or emb % 8))


def _old_pingpong_mode_launches(N, K, has_bias, out16):
    """launch_gemm_bf16_pingpong_mode(...) == 0 (and launch_gemm_bf16_pingpong with out16 = False)"""
    if not has_bias:
        return False
    return _old_pingpong_epi_launches(N, K, True, EPI_STORE_BF16 if out16 else EPI_STORE, 0, 0)


def _old_nt_epi(M, N, K, has_bias, mode, dh, emb, knobs):
    """launch_gemm_bf16_nt_epi"""
    if M <= 0:
        return KNONE
    if M >= 4096 and not knobs & KNOB_NO_PINGPONG:
        if _old_pingpong_epi_launches(N, K, has_bias, mode, dh, emb):
            return KPINGPONG
    return K128                                                   # the f16 switch and the bf16 switch: the same kernel template


def _old_nt(M, N, K, lda, ldb, has_bias, f16, train_splitk, knobs):
    """launch_gemm_bf16_nt"""
    if f16:
        return _old_nt_epi(M, N, K, has_bias, EPI_STORE, 0, 0, knobs)
    if (train_splitk and not knobs & KNOB_NO_SPLITK and ((M + 127) // 128) * ((N + 127) // 128) <= 256 and K >= 1024 and K % 64 == 0
            and _old_tn_launches_nt(M, N, K, lda, ldb)):
        return KSPLITK
    if M >= 4096 and N % 256 == 0 and not knobs & KNOB_NO_BIG:
        if knobs & KNOB_NO_PINGPONG or not _old_pingpong_mode_launches(N, K, has_bias, False):
            return K256SQ                                         # launch_gemm_bf16_experimental(9, ...): N % 256 == 0 holds here
        return KPINGPONG
    if M >= 2048 and not knobs & KNOB_NO_BIG:
        return K256X128
    return _old_nt_epi(M, N, K, has_bias, EPI_STORE, 0, 0, knobs)


def _old_proj(M, N, K, lda, ldb, has_bias, f16, out16, keep, knobs):
    """the 16-bit-operand branches of miniroad_forward.cpp's proj (h->bf16 set, no x2)"""
    if not out16 and not f16:
        return _old_nt(M, N, K, lda, ldb, has_bias, False, keep, knobs)
    if M >= 4096 and _old_pingpong_mode_launches(N, K, has_bias, out16):
        return KPINGPONG
    return _old_nt_epi(M, N, K, has_bias, EPI_STORE_BF16 if out16 else EPI_STORE, 0, 0, knobs)


def old_nt_choice(entry, M, N, K, lda, ldb, has_bias, f16, train_splitk, mode, dh, emb, knobs):
    """the kernel the old chain ran for what prego_debug_gemm_nt_choice is asked, by the entry's old function"""
    if entry == ENTRY_PLAIN:
        assert mode == EPI_STORE
        return _old_nt(M, N, K, lda, ldb, has_bias, f16, train_splitk, knobs)
    if entry == ENTRY_PROJ16:
        assert mode in (EPI_STORE, EPI_STORE_BF16) and (f16 or mode == EPI_STORE_BF16)
        return _old_proj(M, N, K, lda, ldb, has_bias, f16, mode == EPI_STORE_BF16, train_splitk, knobs)
    return _old_nt_epi(M, N, K, has_bias, mode, dh, emb, knobs)


@dataclass
class Operand:
    """a 16-bit matrix inside its NaN-filled allocation: the kernel gets ptr() and ld; rows x width is what it may use"""
    buf: torch.Tensor          # flat
    off: int                   # element offset of the matrix's first element
    rows: int                  # rows the matrix has behind off (k-major: K, of which the first k_valid are values)
    ld: int

    def ptr(self):
        return self.buf.data_ptr() + self.off * self.buf.element_size()

    def flat64(self):
        """what lies at and behind the kernel's pointer, to the end of the allocation, as fp64 numpy (the CPU emulation's view)"""
        return self.buf[self.off:].to(torch.float64).cpu().numpy()


def _values(shape, kind, r, dtype16, gen, device):
    if kind == "int":
        return torch.randint(-r, r + 1, shape, generator=gen, device=device, dtype=torch.int32).to(torch.float64)
    v = torch.rand(shape, generator=gen, device=device, dtype=torch.float32) * 2 - 1           # uniform in [-1, 1], rounded to the operand type
    return v.to(dtype16).to(torch.float64)


def _nan_buf(n, dtype, device):
    return torch.full((n,), float("nan"), dtype=dtype, device=device)


def kmajor_operand(vals, K, ld, dtype16):
    """vals [k_valid, W] stored as rows 0 .. k_valid-1 of a [K][ld] matrix; rows >= k_valid, columns >= W and the guard rows are NaN"""
    kv, W = vals.shape
    assert kv <= K and W <= ld
    buf = _nan_buf((GUARD + K + GUARD) * ld, dtype16, vals.device)
    buf.view(-1, ld)[GUARD:GUARD + kv, :W] = vals.to(dtype16)
    return Operand(buf, GUARD * ld, K, ld)


def rowmajor_operand(vals, K, ld, dtype16):
    """vals [R, k_valid] stored as [R][ld]: columns k_valid .. K-1 ZEROS (the caller's contract), columns >= K and the guard rows NaN"""
    R, kv = vals.shape
    assert kv <= K <= ld
    buf = _nan_buf((GUARD + R + GUARD) * ld, dtype16, vals.device)
    v = buf.view(-1, ld)
    v[GUARD:GUARD + R, :kv] = vals.to(dtype16)
    v[GUARD:GUARD + R, kv:K] = 0
    return Operand(buf, GUARD * ld, R, ld)


@dataclass
class TnProblem:
    case: TnCase
    A: Operand
    B: Operand
    bias: torch.Tensor         # fp32 [N] or None
    a: torch.Tensor            # fp64 [M, k_valid]: the logical operands
    b: torch.Tensor            # fp64 [k_valid, N]

    def reference(self):
        """fp64 (C, sum_k |a b| + |bias|, column sums of A over k)"""
        ref = self.a @ self.b
        mag = self.a.abs() @ self.b.abs()
        if self.bias is not None:
            ref = ref + self.bias.to(torch.float64)
            mag = mag + self.bias.to(torch.float64).abs()
        return ref, mag, self.a.sum(dim=1)


def make_tn(case, kind="int", dtype16=torch.bfloat16, device="cpu", seed=0):
    lda, ldb = case.ld()
    gen = torch.Generator(device=device).manual_seed(seed)
    r = r_of_k(case.K)
    a = _values((case.M, case.k_valid), kind, r, dtype16, gen, device)
    b = _values((case.k_valid, case.N), kind, r, dtype16, gen, device)
    bias = _values((case.N,), kind, r, torch.float32, gen, device).to(torch.float32) if case.bias else None
    A = kmajor_operand(a.T, case.K, lda, dtype16) if case.ta else rowmajor_operand(a, case.K, lda, dtype16)
    B = kmajor_operand(b, case.K, ldb, dtype16) if case.tb else rowmajor_operand(b.T, case.K, ldb, dtype16)
    return TnProblem(case, A, B, bias, a, b)


@dataclass
class Output:
    """an M x N block with leading dimension ldc inside a canary-filled allocation with guard rows before and behind"""
    buf: torch.Tensor
    off: int
    M: int
    N: int
    ldc: int

    def ptr(self):
        return self.buf.data_ptr() + self.off * self.buf.element_size()

    def _bits(self):
        return self.buf.view(torch.int32 if self.buf.dtype == torch.float32 else torch.int16).view(-1, self.ldc)

    def block(self):
        return self.buf.view(-1, self.ldc)[GUARD:GUARD + self.M, :self.N]

    def canary_elsewhere(self):
        """every element outside the block still holds the canary's bits"""
        bits = self._bits()
        c = _signed(CANARY32, 32) if self.buf.dtype == torch.float32 else _signed(CANARY16[self.buf.dtype], 16)
        return bool((bits[:GUARD] == c).all()) and bool((bits[GUARD + self.M:] == c).all()) and \
            bool((bits[GUARD:GUARD + self.M, self.N:] == c).all())

    def untouched(self):
        c = _signed(CANARY32, 32) if self.buf.dtype == torch.float32 else _signed(CANARY16[self.buf.dtype], 16)
        return bool((self._bits() == c).all())


def _signed(v, bits):
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


def make_output(M, N, ldc, dtype=torch.float32, device="cpu"):
    assert ldc >= N
    buf = torch.empty(((GUARD + M + GUARD) * ldc,), dtype=dtype, device=device)
    if dtype == torch.float32:
        buf.view(torch.int32).fill_(_signed(CANARY32, 32))
    else:
        buf.view(torch.int16).fill_(_signed(CANARY16[dtype], 16))
    return Output(buf, GUARD * ldc, M, N, ldc)


def bits_equal(got, want):
    """bit-for-bit equality of two tensors of one floating type"""
    it = {4: torch.int32, 2: torch.int16}[got.element_size()]
    return got.dtype == want.dtype and got.shape == want.shape and bool((got.contiguous().view(it) == want.contiguous().view(it)).all())


def first_mismatches(got, want, n=5):
    """'(m, n): got x want y' of the first differing elements, for the assertion message"""
    bad = (got != want) | torch.isnan(got)
    idx = bad.nonzero()[:n].tolist()
    return f"{int(bad.sum())} elements differ; " + ", ".join(f"({i}, {j}): got {float(got[i, j])!r} want {float(want[i, j])!r}" for i, j in idx)


def expected_bf16(ref64):
    """the fp64 result as a kernel with a round-to-nearest-even bf16 store must write it (the integers here are exact in fp32, so the
    way through fp32 rounds once)"""
    return ref64.to(torch.float32).to(torch.bfloat16)


def error_bound(K, mag64):
    """|got - ref| <= K * 2^-23 * (sum_k |a_k b_k| + |bias|): fp32 accumulation of the K exact products and the bias in ANY order (first-order
    bound (n - 1) u sum |x_i| of an n = K + 1 term sum, with the unit roundoff taken as 2^-23 instead of RNE's 2^-24 so that an
    accumulate that does not round to nearest inside the MFMA is covered).  A worst-case bound, not a measurement."""
    return K * 2.0 ** -23 * mag64


def bf16_ulp(x64):
    """spacing of bf16 (8 significant bits) at |x|"""
    _, e = torch.frexp(x64.abs())              # |x| = m 2^e, m in [0.5, 1): the leading bit weighs 2^(e-1), the last of eight 2^(e-8)
    return torch.ldexp(torch.ones_like(x64), e - 8)


def error_bound_bf16(K, ref64, mag64):
    """the fp32 bound plus one bf16 ulp (taken at |ref| + bound, so that a result rounded across a binade is covered)"""
    b = error_bound(K, mag64)
    return b + bf16_ulp(ref64.abs() + b)


# ---- the NT family: C[M,N] = A[M,K] . B[N,K]^T + bias, both operands row-major over k
@dataclass
class NtProblem:
    A: Operand
    B: Operand
    bias: torch.Tensor
    a: torch.Tensor            # fp64 [M, K]
    b: torch.Tensor            # fp64 [N, K]

    def reference(self):
        bias = self.bias.to(torch.float64)
        return self.a @ self.b.T + bias, self.a.abs() @ self.b.abs().T + bias.abs()


def make_nt(M, N, K, kind="int", dtype16=torch.bfloat16, device="cpu", seed=0, lda=0, ldb=0):
    """lda / ldb = 0: K (what prego_debug_gemm_bf16 fixes); larger: the pad columns are NaN"""
    gen = torch.Generator(device=device).manual_seed(seed)
    r = r_of_k(K)
    a = _values((M, K), kind, r, dtype16, gen, device)
    b = _values((N, K), kind, r, dtype16, gen, device)
    bias = _values((N,), kind, r, torch.float32, gen, device).to(torch.float32)
    return NtProblem(rowmajor_operand(a, K, lda or K, dtype16), rowmajor_operand(b, K, ldb or K, dtype16), bias, a, b)


# ---- numpy emulation of launch_gemm_bf16_tn's contract on the raw storage (the CPU test's check that guards and poison are where this
# module says): everything is read from the flat arrays behind the kernel's pointers with the strides the kernel is given
def emulate_tn(case, a_flat, b_flat, bias, honour_k_valid=True, honour_columns=True):
    """fp64 C from the storage.  honour_k_valid = False contracts over all K rows / columns; honour_columns = False takes every column of a
    k-major operand up to its leading dimension for an output row / column (C then has lda rows / ldb columns)."""
    lda, ldb = case.ld()
    M, N, K = case.M, case.N, case.K
    kv = case.k_valid if honour_k_valid else K
    if case.ta:
        A = a_flat[:K * lda].reshape(K, lda)[:kv, :(M if honour_columns else lda)].T
    else:
        A = a_flat[:M * lda].reshape(M, lda)[:, :kv]
    if case.tb:
        B = b_flat[:K * ldb].reshape(K, ldb)[:kv, :(N if honour_columns else ldb)]
    else:
        B = b_flat[:N * ldb].reshape(N, ldb)[:, :kv].T
    with np.errstate(invalid="ignore"):
        C = A @ B
    if bias is not None:
        C[:, :N] += bias
    return C


def low_byte_nonzero_fraction(vals64):
    """fraction of the values whose bf16 pattern has a non-zero low byte (a load that drops the low mantissa bits changes them)"""
    bits = vals64.to(torch.bfloat16).contiguous().view(torch.int16)
    return float(((bits & 0xFF) != 0).double().mean())
