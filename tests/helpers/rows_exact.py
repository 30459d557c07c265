"""References, exact input families and derived bounds of the kernel-level tests of the row-wise training kernels
(tests/test_gpu_rows.py), and the checks the CPU test of this module's own arithmetic shares with them (tests/test_rows_reference_cpu.py).

The method is that of tests/helpers/gemm_exact.py, whose make_output / bits_equal / first_mismatches / expected_bf16 are used here.

EXACT families.  Inputs are chosen so that every intermediate of the operation is a dyadic rational that fp32 represents, and every sum
has terms that are multiples of one power of two q with sum |term| / q < 2^24: the result is then the same bits under any summation
order and with or without fused multiply-add, and the tests ask for bit equality on every element.  `exact32` and `sum_is_exact` check
those two conditions on the actual instance (not only on paper), and tests/test_rows_reference_cpu.py evaluates the families in fp32 in
two orders, with and without an emulated FMA.
  * gru_bwd_step: r, z in k/8 inside (0, 1), n in k/8 inside (-1, 1), ghn and hprev in k/8 (|.| <= 2), dHout, carry_z_in, dhpart in k/4
    (|.| <= 1, so dh = K/4 with |K| <= 12: 4 bits).  The longest product dh (1-z) (1-n^2) ghn r (1-r) has factors of 4, 3, 6 (1 - n^2 =
    (64 - k^2) / 64 <= 63/64), 4, 3, 3 bits: 23 bits, so every association of it and every shorter product (dz z (1-z): 4 + 5 + 3 + 3)
    is exact.  GRU_PRODUCT_BITS = 24 is what fp32 holds; gru_bwd_product_bits measures the instance and the tests assert it.
  * ln_relu_bwd: mu integer, rstd in {1/2, 1/4}, Y - mu and dE small integers (dE multiples of 4, so that the dropout scale of p = 0.2,
    fl32(1 / (1 - 0.2f)) = 1.25 exactly, keeps them integers), gamma = +-2^k, beta small integers.  At E a power of two the two row means
    are exact quotients.

DERIVED bounds for what cannot be exact.  U = 2^-23 is used as the unit roundoff: twice round-to-nearest's 2^-24, which covers
second-order terms and library functions of up to 2 ulp where one is named below.  Notation: d(x) is the bound on |computed x - exact x|.
  * a sum of n fp32 terms reduced by ONE WAVE (or one 256-thread workgroup) - each lane adds its share in some order, then a 6-level
    butterfly (and 3 more additions across four waves) - passes every term through at most `depth` additions:
        d(sum) <= depth U sum |term|.
  * LayerNorm statistics of a row v of E values (ln_forward_bounds), depth D:
        d(mu)   <= D U sum|v| / E + U |mu|
        d(c_i)  <= d(mu) + U |c_i|,                     c_i = v_i - mu
        d(var)  <= [sum (2 |c_i| d(c_i) + U c_i^2) + D U sum c_i^2] / E + U var
        d(rstd) <= rstd (d(var) / (2 (var + eps)) + 3 U)              (the addition of eps, a correctly rounded sqrt and division)
        d(xhat_i) <= d(c_i) rstd + |c_i| d(rstd) + U |xhat_i|
        d(out_i) <= |g_i| d(xhat_i) + 2 U (|xhat_i g_i| + |b_i|)      then x scale with one more rounding when dropout is on;
    ReLU is 1-Lipschitz and keeps the bound.  A 16-bit output adds half an ulp of its type at |ref| + bound.
  * LayerNorm backward of a row (ln_bwd_dy_bound) with exact dxh and xhat (the exact family at E not a power of two): m1 = s1 / E and
    m2 = s2 / E round once each, then dxh - m1 - xhat m2 takes two subtractions and a product:
        d(dY) <= rstd U (2 |dxh| + 3 |m1| + 3 |xhat m2|) (+ U (|dY| + |prior|) when accumulating).
  * GELU derivative (gelu_bwd_bound): g (Phi(u) + u phi(u)).  phi uses the FAST exponential __expf(y) = exp2(y log2 e) on y = -u^2/2: the
    rounding of y (two products) and of y log2 e is amplified by |y| - exp(y (1 + e)) = exp(y) (1 + y e) - so its relative error is
    (3 |y| + 3) U rather than one ulp; at |u| = 12 that is 219 U = 2.6e-5.  erff is taken at HIP's documented 4 ulp = 2 U, its argument
    u / sqrt 2 rounds twice and erf' = 2 / sqrt(pi) exp(-x^2):
        d(Phi) <= 0.5 (2 U |erf| + 1.13 exp(-u^2/2) 2 U |u| + U |1 + erf|)
        d(u phi) <= |u| phi ((3 |y| + 3) U + 2 U)
        d(du) <= |g| (d(Phi) + d(u phi) + 2 U |Phi + u phi|) + 2^-126.
  * head, loss and AdamW: at their functions below."""
from __future__ import annotations

import numpy as np
import torch

from oracle.oracle_np import hash_dropout_mask
from tests.helpers.gemm_exact import CANARY32, bits_equal, expected_bf16, first_mismatches, make_output  # noqa: F401

U = 2.0 ** -23
F16_MAX = 65504.0
GRU_PRODUCT_BITS = 24
T32, TBF, TF16 = 0, 1, 2
TORCH_TYPE = {T32: torch.float32, TBF: torch.bfloat16, TF16: torch.float16}


# ---- the two assertions every test of these kernels uses (GPU tests on kernel output, the CPU test on mutants) ----------------------------
def as2d(t):
    return t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])


def assert_exact(got, want, what=""):
    """bit equality over the WHOLE tensor (torch tensors of one floating type)"""
    got, want = as2d(got), as2d(want)
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)} vs {want.dtype} {tuple(want.shape)}"
    assert bits_equal(got, want), f"{what}: {first_mismatches(got.float(), want.float())}"


def assert_within(got64, ref64, bound64, what=""):
    """|got - ref| <= bound on every element (numpy fp64); returns the largest err / bound"""
    got64, ref64, bound64 = np.asarray(got64, np.float64), np.asarray(ref64, np.float64), np.asarray(bound64, np.float64)
    assert got64.shape == ref64.shape == bound64.shape, f"{what}: shapes {got64.shape} {ref64.shape} {bound64.shape}"
    assert np.isfinite(got64).all(), f"{what}: {int((~np.isfinite(got64)).sum())} non-finite outputs"
    err = np.abs(got64 - ref64)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound64, 1e-300))
    i = int(np.argmax(ratio))
    worst = float(ratio.flat[i])
    print(f"{what}: max err / bound = {worst:.3e}")
    assert worst <= 1.0, f"{what}: element {np.unravel_index(i, ratio.shape)}: got {got64.flat[i]!r} want {ref64.flat[i]!r} bound {bound64.flat[i]:.3e} (ratio {worst:.3f})"
    return worst


def exact32(x64):
    """the fp64 array holds fp32-representable values only"""
    x64 = np.asarray(x64, np.float64)
    return bool((x64.astype(np.float32).astype(np.float64) == x64).all())


def sum_is_exact(terms64, q, axis=None):
    """every term is a multiple of q and sum |term| / q < 2^24: any partial sum in any order is fp32-exact"""
    t = np.asarray(terms64, np.float64) / q
    return bool((t == np.round(t)).all()) and bool((np.abs(t).sum(axis=axis) < 2 ** 24).all())


def significant_bits(x64):
    """the longest significand among the values (0 for zeros)"""
    m, _ = np.frexp(np.abs(np.asarray(x64, np.float64)))
    k = np.zeros(m.shape, np.int64)
    for b in range(1, 54):
        k = np.where((m * 2.0 ** b == np.round(m * 2.0 ** b)) & (k == 0) & (m != 0), b, k)
    return int(k.max()) if k.size else 0


# ---- conversions ---------------------------------------------------------------------------------------------------------------------------
def t32(x64):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x64, np.float64).astype(np.float32)))


def convert(x32, typ, mutant=None):
    """fp32 torch tensor -> the kernels' store of type `typ`: bf16 round to nearest even, fp16 saturated at +-65504 then round to nearest
    even, fp32 as it is.  mutant 'truncate': the low 16 bits dropped instead of rounded (bf16)"""
    x32 = x32.to(torch.float32)
    if typ == T32:
        return x32.clone()
    if typ == TBF:
        if mutant == "truncate":
            return ((x32.contiguous().view(torch.int32) >> 16).to(torch.int16)).view(torch.bfloat16)
        return x32.to(torch.bfloat16)
    return x32.clamp(-F16_MAX, F16_MAX).to(torch.float16)


def bf16_rne_bits(x32_np):
    """round to nearest even in integer arithmetic (finite inputs): an implementation independent of torch's, for the CPU test"""
    b = np.asarray(x32_np, np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def edge_values(typ):
    """fp32 inputs at which a 16-bit conversion goes wrong first: ties (to even, both parities), values just above and below a tie, the
    largest finite values, subnormals of the target and of fp32, signed zeros; for fp16 values beyond +-65504 (saturated)"""
    f = np.float32
    if typ == TF16:
        tie, eps = 2.0 ** -11, 2.0 ** -20
        v = [1 + tie, 1 + 3 * tie, 1 + tie + eps, 1 + tie - eps, 1 + 3 * tie + eps, 1 + 3 * tie - eps, 65504.0, 65519.0, 65520.0, 65536.0, 70000.0, 1e5,
             3.0e38, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -10), 3 * 2.0 ** -25, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 1e-10, 1e-40, 0.0]
    else:
        tie, eps = 2.0 ** -8, 2.0 ** -20
        v = [1 + tie, 1 + 3 * tie, 1 + tie + eps, 1 + tie - eps, 1 + 3 * tie + eps, 1 + 3 * tie - eps, 3.3895313892515355e38, 3.4028234663852886e38,
             3.39e38, 2.0 ** -126, 2.0 ** -127, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -134 * (1 + 2.0 ** -10), 1e-40, 2.0 ** -149, 0.0,
             65504.0, 70000.0]
    v = np.array(v, np.float64)
    return np.concatenate([v, -v]).astype(f)


def finite_values(n, gen, typ=T32):
    """arbitrary finite fp32 values over many binades, the edge values of `typ` first"""
    x = (gen.standard_normal(n) * np.exp2(gen.integers(-20, 20, n))).astype(np.float32)
    e = edge_values(typ if typ != T32 else TBF)
    k = min(len(e), n)
    x[:k] = e[:k]
    return x


# ---- dropout -------------------------------------------------------------------------------------------------------------------------------
def drop_scale(p):
    """the kernels' scale: 1.f / (1.f - p) in fp32 (1 for p = 0)"""
    return np.float32(1) / (np.float32(1) - np.float32(p)) if p > 0 else np.float32(1)


def keep_mask(seed, start, n, p):
    """bool [n]: elements start .. start + n - 1 survive; the threshold is (unsigned)((double)(float)p 2^32) as on the device"""
    if p <= 0:
        return np.ones(n, bool)
    return hash_dropout_mask(seed, start + n, float(np.float32(p)))[start:] > 0


# ---- LayerNorm forward -----------------------------------------------------------------------------------------------------------------------
def ln_stats(v64, eps):
    mu = v64.mean(axis=-1, keepdims=True)
    var = ((v64 - mu) ** 2).mean(axis=-1, keepdims=True)
    return mu, var, 1.0 / np.sqrt(var + eps)


def ln_relu_ref(Y64, gamma64, beta64, eps, relu, p, seed, row0_abs, mutant=None):
    """fp64 (out, mu, rstd) of LayerNorm [+ ReLU] [+ dropout on element (row0_abs + r) E + c]"""
    R, E = Y64.shape
    mu, var, rstd = ln_stats(Y64, float(np.float32(eps)))
    o = (Y64 - mu) * rstd * gamma64 + beta64
    if relu:
        o = np.maximum(o, 0.0)
    if p > 0:
        start = {"drop_shift": row0_abs * E + 1, "no_row0": 0}.get(mutant, row0_abs * E)
        o = np.where(keep_mask(seed, start, R * E, p).reshape(R, E), o * float(drop_scale(p)), 0.0)
    return o, mu[:, 0], rstd[:, 0]


def ln_forward_bounds(v64, gamma64, beta64, eps, depth, scale=1.0):
    """(d(out), d(mu), d(rstd), d(xhat)) per the module docstring; v64 [R, E]"""
    E = v64.shape[-1]
    mu, var, rstd = ln_stats(v64, eps)
    c = v64 - mu
    d_mu = depth * U * np.abs(v64).sum(-1, keepdims=True) / E + U * np.abs(mu)
    d_c = d_mu + U * np.abs(c)
    d_var = ((2 * np.abs(c) * d_c + U * c * c).sum(-1, keepdims=True) + depth * U * (c * c).sum(-1, keepdims=True)) / E + U * var
    d_rstd = rstd * (d_var / (2 * (var + eps)) + 3 * U)
    xh = c * rstd
    d_xh = d_c * rstd + np.abs(c) * d_rstd + U * np.abs(xh)
    d_out = np.abs(gamma64) * d_xh + 2 * U * (np.abs(xh * gamma64) + np.abs(beta64))
    if scale != 1.0:
        d_out = d_out * scale + U * np.abs((xh * gamma64 + beta64) * scale)
    return d_out, d_mu[:, 0], d_rstd[:, 0], d_xh


def ulp16(x64, typ):
    """spacing of bf16 (8 significant bits) / fp16 (11, subnormals below 2^-14) at |x|"""
    _, e = np.frexp(np.abs(x64))
    e = np.where(np.asarray(x64) == 0, -1000, e)
    if typ == TBF:
        return np.ldexp(1.0, np.maximum(e, -125) - 8)
    return np.ldexp(1.0, np.maximum(e, -13) - 11)


def store_bound(ref64, bound64, typ):
    """the fp32 bound, plus half an ulp of a 16-bit store taken at |ref| + bound (a result rounded across a binade is covered)"""
    if typ == T32:
        return bound64
    return bound64 + 0.5 * ulp16(np.abs(ref64) + bound64, typ)


def ln_inputs(R, E, gen, in_typ=T32):
    """dyadic rows (k / 8 around a per-row integer offset): at E a power of two the row mean is an exact quotient, so stats[2 r] is checked
    bit for bit there; gamma, beta real-valued"""
    Y = gen.integers(-64, 65, (R, E)) / 8.0 + gen.integers(-3, 4, (R, 1))
    if in_typ != T32:
        Y = t32(Y).to(TORCH_TYPE[in_typ]).to(torch.float64).numpy()
    gamma = gen.standard_normal(E).astype(np.float32).astype(np.float64)
    beta = (0.5 * gen.standard_normal(E)).astype(np.float32).astype(np.float64)
    return Y, gamma, beta


# ---- LayerNorm backward ----------------------------------------------------------------------------------------------------------------------
def ln_bwd_inputs(R, E, gen):
    """the exact family (module docstring): dict of fp64 arrays; stats [R, 2] = (mu, rstd)"""
    mu = gen.integers(-3, 4, (R, 1)).astype(np.float64)
    rstd = np.exp2(-gen.integers(1, 3, (R, 1)).astype(np.float64))
    Y = mu + gen.integers(-6, 7, (R, E))
    gamma = np.exp2(gen.integers(-1, 2, E)) * gen.choice([-1.0, 1.0], E)
    beta = gen.integers(-2, 3, E).astype(np.float64)
    dE = 4.0 * gen.integers(-3, 4, (R, E))
    prior = gen.integers(-8, 9, (R, E)).astype(np.float64)
    return dict(Y=Y, dE=dE, gamma=gamma, beta=beta, stats=np.concatenate([mu, rstd], 1), prior=prior)


def ln_bwd_ref(a, relu, p, seed, row0_abs, accumulate, mutant=None, fp=np.float64, order=1, fma=False):
    """(dY, dgamma, dbeta, pre) from the formulas of train.hip's header comment.  fp / order / fma: the evaluation the CPU test varies to
    hold the exactness claim (fp32, reversed summation, fused multiply-add emulated in fp64)."""
    f = fp
    Y, dE, g, b = (a[k].astype(f) for k in ("Y", "dE", "gamma", "beta"))
    R, E = Y.shape
    mu, rstd = a["stats"][:, :1].astype(f), a["stats"][:, 1:].astype(f)

    def mad(x, y, z):                       # x y + z, fused (one rounding) or not
        if fma:
            return (x.astype(np.float64) * y.astype(np.float64) + z.astype(np.float64)).astype(f)
        return (x * y).astype(f) + z

    def rsum(x, axis):
        x = x if order == 1 else np.flip(x, axis)
        return np.add.accumulate(x, axis=axis, dtype=f).take(-1, axis=axis) if f != np.float64 else x.sum(axis)

    xh = ((Y - mu) * rstd).astype(f)
    pre = mad(xh, g, b)
    d = dE.copy()
    if relu:
        d = np.where(pre >= 0 if mutant == "relu_ge" else pre > 0, d, f(0))
    if p > 0:
        start = {"drop_shift": row0_abs * E + 1, "no_row0": 0}.get(mutant, row0_abs * E)
        d = np.where(keep_mask(seed, start, R * E, p).reshape(R, E), (d * f(drop_scale(p))).astype(f), f(0))
    dxh = (d * g).astype(f)
    div = f(R if mutant == "mean_nrows" else E)
    m1 = (rsum(dxh, 1) / div).astype(f)[:, None]
    m2 = (rsum((dxh * xh).astype(f), 1) / div).astype(f)[:, None]
    dY = (rstd * mad(-xh, m2, (dxh - m1).astype(f))).astype(f)
    if accumulate:
        dY = (dY + a["prior"].astype(f)).astype(f)
    rows = R - R % 4 if mutant == "skip_last_block" else R
    dgam, dbet = rsum((d * xh).astype(f)[:rows], 0), rsum(d[:rows], 0)
    if mutant == "drop_dgamma_col":
        dgam = dgam.copy()
        dgam[int(np.argmax(np.abs(dgam)))] = 0
    return dY, dgam, dbet, pre


def ln_bwd_is_exact(a, relu, p, seed, row0_abs, accumulate):
    """the conditions of the module docstring on this instance (E a power of two)"""
    Y, dE, g, b = a["Y"], a["dE"], a["gamma"], a["beta"]
    R, E = Y.shape
    mu, rstd = a["stats"][:, :1], a["stats"][:, 1:]
    xh = (Y - mu) * rstd
    dY, dgam, dbet, pre = ln_bwd_ref(a, relu, p, seed, row0_abs, accumulate)
    d = dE * (pre > 0 if relu else 1)
    if p > 0:
        d = np.where(keep_mask(seed, row0_abs * E, R * E, p).reshape(R, E), d * 1.25, 0.0)
    dxh = d * g
    m2 = (dxh * xh).sum(1, keepdims=True) / E
    return (float(drop_scale(p)) in (1.0, 1.25) and sum_is_exact(dxh, 0.5, 1) and sum_is_exact(dxh * xh, 0.125, 1) and sum_is_exact(d * xh, 0.25, 0)
            and sum_is_exact(d, 1.0, 0) and all(exact32(x) for x in (xh, pre, xh * m2, dxh - dxh.sum(1, keepdims=True) / E - xh * m2, dY, dgam, dbet)))


def ln_bwd_dy_bound(a, relu, p, seed, row0_abs, accumulate):
    Y, g = a["Y"], a["gamma"]
    E = Y.shape[1]
    mu, rstd = a["stats"][:, :1], a["stats"][:, 1:]
    xh = (Y - mu) * rstd
    dY, _, _, pre = ln_bwd_ref(a, relu, p, seed, row0_abs, accumulate)
    d = a["dE"] * (pre > 0 if relu else 1)
    if p > 0:
        d = np.where(keep_mask(seed, row0_abs * E, Y.size, p).reshape(Y.shape), d * float(drop_scale(p)), 0.0)
    dxh = d * g
    m1, m2 = dxh.sum(1, keepdims=True) / E, (dxh * xh).sum(1, keepdims=True) / E
    bound = rstd * U * (2 * np.abs(dxh) + 3 * np.abs(m1) + 3 * np.abs(xh * m2))
    if accumulate:
        bound = bound + U * (np.abs(dY) + np.abs(a["prior"]))
    return bound


# ---- sums ------------------------------------------------------------------------------------------------------------------------------------
def int_matrix(M, N, gen, r=127):
    """small integers: exact in bf16 (8 bits) and every partial column sum below 2^24"""
    assert r <= 127 and M * r < 2 ** 24
    return gen.integers(-r, r + 1, (M, N)).astype(np.float64)


def colsum_ref(src64, mutant=None):
    return src64[:src64.shape[0] - src64.shape[0] % 64].sum(0) if mutant == "skip_last_block" else src64.sum(0)


# ---- layout helpers --------------------------------------------------------------------------------------------------------------------------
def transpose_ref(src32, M, N, Mpad, out_typ, mutant=None):
    """dst [N][Mpad] from the src [>= M][ld] torch fp32 VALUES (bf16 inputs are passed upcast): pad columns zero"""
    dst = torch.zeros((N, Mpad), dtype=torch.float32)
    dst[:, :M] = src32[:M, :N].T
    out = convert(dst, out_typ, "truncate" if mutant == "truncate" else None)
    if mutant == "pad_unwritten" and Mpad > M:
        out[:, M:] = float("nan")
    return out


def plan_rows(lens):
    """rowoff [t_max + 1], sorted_clip (clips by length, descending, stable), and (t, clip) of every packed row"""
    order = sorted(range(len(lens)), key=lambda i: -lens[i])
    t_max = max(lens)
    nact = [sum(1 for n in lens if n > t) for t in range(t_max)]
    rowoff = np.concatenate([[0], np.cumsum(nact)]).astype(np.int32)
    rows = [(t, order[i]) for t in range(t_max) for i in range(nact[t])]
    return rowoff, np.array(order, np.int32), rows


def gather_dlogits_ref(dl_list32, lens, C, Cpad, out_typ):
    rowoff, order, rows = plan_rows(lens)
    out = torch.zeros((len(rows), Cpad), dtype=torch.float32)
    for r, (t, clip) in enumerate(rows):
        out[r, :C] = dl_list32[clip][t]
    return convert(out, out_typ)


def build_hprev_ref(Hraw32, lens, out_typ):
    rowoff, order, rows = plan_rows(lens)
    out = torch.zeros((len(rows), Hraw32.shape[1]), dtype=torch.float32)
    for r, (t, clip) in enumerate(rows):
        if t > 0:
            out[r] = Hraw32[rowoff[t - 1] + (r - rowoff[t])]
    return convert(out, out_typ)


# ---- GRU backward step -------------------------------------------------------------------------------------------------------------------------
def gru_bwd_inputs(na, H, gen):
    """the exact family of the module docstring, for rows b < na: dict of fp64 [na, H]"""
    e = lambda lo, hi: gen.integers(lo, hi + 1, (na, H)) / 8.0      # noqa: E731
    q = lambda lo, hi: gen.integers(lo, hi + 1, (na, H)) / 4.0      # noqa: E731
    return dict(r=e(1, 7), z=e(1, 7), n=e(-7, 7), ghn=e(-16, 16), hprev=e(-16, 16), dHout=q(-4, 4), carry=q(-4, 4), dhpart=q(-4, 4))


def gru_bwd_ref(a, na_next, t, mutant=None, fp=np.float64, fma=False):
    """(carry_z_out [na,H], dGI [na,3H], dGH [na,3H]) by train.hip's header formulas; hprev = 0 at t = 0"""
    f = fp
    r, z, n, ghn, dHout = (a[k].astype(f) for k in ("r", "z", "n", "ghn", "dHout"))
    na = r.shape[0]
    hprev = a["hprev"].astype(f) if t > 0 else np.zeros_like(r)
    cont = (np.arange(na) < na_next)[:, None]
    dh = (dHout + np.where(cont, (a["carry"].astype(f) + a["dhpart"].astype(f)).astype(f), f(0))).astype(f)
    one = f(1)
    dn = (dh * (one - z)).astype(f)
    dz = (dh * (hprev - n)).astype(f)
    if fma:                                  # 1 - n n as one fused operation
        omn2 = (one - n.astype(np.float64) * n.astype(np.float64)).astype(f)
    else:
        omn2 = (one - (n * n).astype(f)).astype(f)
    dpn = (dn * omn2).astype(f)
    dpr = (((dpn * ghn).astype(f) * r).astype(f) * (one - r)).astype(f)
    dpz = ((dz * z).astype(f) * (one - z)).astype(f)
    carry = dn if mutant == "carry_1mz" else (dh * z).astype(f)
    dgi = np.concatenate([dpr, dpz, dpn], 1)
    dgh = np.concatenate([dpr, dpz, dpn if mutant == "no_r_dgh" else (dpn * r).astype(f)], 1)
    return carry, dgi, dgh


def gru_bwd_product_bits(a, na_next, t):
    """significant bits of the longest product of the step on this instance (must be <= GRU_PRODUCT_BITS)"""
    _, dgi, dgh = gru_bwd_ref(a, na_next, t)
    return max(significant_bits(dgi), significant_bits(dgh))


# ---- GELU backward -------------------------------------------------------------------------------------------------------------------------------
def _erf64(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x))).numpy()


def gelu_bwd_ref(df64, u64, p, seed):
    g = df64 if p <= 0 else np.where(keep_mask(seed, 0, df64.size, p), df64 * float(drop_scale(p)), 0.0)
    cdf = 0.5 * (1.0 + _erf64(u64 / np.sqrt(2.0)))
    pdf = np.exp(-0.5 * u64 * u64) / np.sqrt(2 * np.pi)
    return g * (cdf + u64 * pdf)


def gelu_bwd_bound(df64, u64, p, seed):
    g = np.abs(df64) * (float(drop_scale(p)) if p > 0 else 1.0)
    y = 0.5 * u64 * u64
    erf = _erf64(u64 / np.sqrt(2.0))
    pdf = np.exp(-y) / np.sqrt(2 * np.pi)
    d_cdf = 0.5 * (2 * U * np.abs(erf) + 1.13 * np.exp(-y) * 2 * U * np.abs(u64) + U * np.abs(1 + erf))
    d_upd = np.abs(u64) * pdf * ((3 * y + 3) * U + 2 * U)
    return g * (d_cdf + d_upd + 3 * U * np.abs(0.5 * (1 + erf) + u64 * pdf)) + 2.0 ** -126


# ---- Transformer head ------------------------------------------------------------------------------------------------------------------------------
def head_inputs(B, N, E, C, gen):
    """x real-valued [B, N, E] (token 0 is what counts); lnw = +-2^k, lnb and hb dyadic, hw and dlogits small integers: dy = dlogits hw and
    every sum over the windows of dlogits and dy is then exact (the exact part of vit_head_bwd2)"""
    x = gen.standard_normal((B, N, E)).astype(np.float32).astype(np.float64) * 2 + 0.5
    lnw = np.exp2(gen.integers(-1, 2, E)) * gen.choice([-1.0, 1.0], E)
    lnb = gen.integers(-4, 5, E) / 4.0
    hw = gen.integers(-3, 4, (C, E)).astype(np.float64)
    hb = gen.integers(-8, 9, C) / 4.0
    dl = gen.integers(-3, 4, (B, C)).astype(np.float64)
    return dict(x=x, lnw=lnw, lnb=lnb, hw=hw, hb=hb, dl=dl)


def head_ref(a):
    """fp64 logits [B, C] and their bound: LayerNorm by a 256-thread workgroup (depth E / 256 + 9), then a dot product per class whose
    terms pass through at most E / 256 + 10 additions and the bias':  d(logit) <= sum |w| d(y) + (E / 256 + 11) U (sum |y w| + |hb|)"""
    x0 = a["x"][:, 0, :]
    E = x0.shape[1]
    mu, var, rstd = ln_stats(x0, 1e-5)
    y = (x0 - mu) * rstd * a["lnw"] + a["lnb"]
    d_y, _, _, _ = ln_forward_bounds(x0, a["lnw"], a["lnb"], 1e-5, E // 256 + 9)
    logits = y @ a["hw"].T + a["hb"]
    bound = d_y @ np.abs(a["hw"]).T + (E // 256 + 11) * U * (np.abs(y) @ np.abs(a["hw"]).T + np.abs(a["hb"]))
    return logits, bound


def head_bwd_ref(a):
    """fp64 gradients of the head and their bounds.  Exact (bound 0): dy = dlogits hw, g_lnb = sum_b dy, g_hb = sum_b dlogits.  Bounded, with
    D = E / 256 + 10 and the forward's d(xhat), d(rstd):
      d(m2) <= [sum |dxh| d(xhat) + D U sum |dxh xhat|] / E + U |m2|,   m1 exact up to its division: U |m1|
      d(dx) <= rstd [U |m1| + |xhat| d(m2) + |m2| d(xhat) + 2 U |xhat m2| + 2 U (|dxh| + |m1| + |xhat m2|)] + d(rstd) |dxh - m1 - xhat m2| + U |dx|
      d(g_lnw) <= sum_b |dy| d(xhat) + (B + 1) U sum_b |dy xhat|
      d(g_hw)  <= sum_b |dl| d(y) + (B + 1) U sum_b |dl y|,   d(y) <= |lnw| d(xhat) + 2 U (|xhat lnw| + |lnb|)"""
    x0, lnw, lnb, hw, dl = a["x"][:, 0, :], a["lnw"], a["lnb"], a["hw"], a["dl"]
    B, E = x0.shape
    mu, var, rstd = ln_stats(x0, 1e-5)
    _, _, d_rstd, d_xh = ln_forward_bounds(x0, lnw, lnb, 1e-5, E // 256 + 9)
    d_rstd = d_rstd[:, None]
    xh = (x0 - mu) * rstd
    y = xh * lnw + lnb
    dy = dl @ hw
    dxh = dy * lnw
    m1, m2 = dxh.mean(1, keepdims=True), (dxh * xh).mean(1, keepdims=True)
    inner = dxh - m1 - xh * m2
    dx = rstd * inner
    D = E // 256 + 10
    d_m2 = ((np.abs(dxh) * d_xh).sum(1, keepdims=True) + D * U * np.abs(dxh * xh).sum(1, keepdims=True)) / E + U * np.abs(m2)
    d_dx = rstd * (U * np.abs(m1) + np.abs(xh) * d_m2 + np.abs(m2) * d_xh + 2 * U * np.abs(xh * m2) + 2 * U * (np.abs(dxh) + np.abs(m1) + np.abs(xh * m2))) \
        + d_rstd * np.abs(inner) + U * np.abs(dx)
    d_y = np.abs(lnw) * d_xh + 2 * U * (np.abs(xh * lnw) + np.abs(lnb))
    ref = dict(dx=dx, dy=dy, g_lnw=(dy * xh).sum(0), g_lnb=dy.sum(0), g_hw=dl.T @ y, g_hb=dl.sum(0))
    bound = dict(dx=d_dx, g_lnw=(np.abs(dy) * d_xh).sum(0) + (B + 1) * U * np.abs(dy * xh).sum(0),
                 g_hw=np.abs(dl).T @ d_y + (B + 1) * U * (np.abs(dl).T @ np.abs(y)))
    return ref, bound


# ---- tokens ----------------------------------------------------------------------------------------------------------------------------------------
def tokens_ref(enc32, cls32, pe32, B, T, E, p, seed):
    """x [B, T + 1, E] in fp32: ONE correctly rounded addition and, under dropout, ONE correctly rounded product per element - no order, no
    fusable pair of operations - so the fp32 numpy evaluation is the reference bit for bit"""
    x = np.empty((B, T + 1, E), np.float32)
    x[:, :T] = enc32.reshape(B, T, E) + pe32[:T]
    x[:, T] = cls32 + pe32[T]
    if p > 0:
        x = np.where(keep_mask(seed, 0, x.size, p).reshape(x.shape), x * drop_scale(p), np.float32(0))
    return x


def tokens_bwd_ref(dx64, B, T, E, p, seed):
    """small-integer dx (multiples of 4 under p = 0.2): (denc [B T, E], g_pe [T + 1, E], g_cls [E]) exact"""
    v = dx64.reshape(B, T + 1, E)
    if p > 0:
        v = np.where(keep_mask(seed, 0, v.size, p).reshape(v.shape), v * float(drop_scale(p)), 0.0)
    return v[:, :T].reshape(B * T, E), v.sum(0), v.sum(0)[T]


# ---- loss --------------------------------------------------------------------------------------------------------------------------------------------
def oad_loss_ref(last_logits64, last_targets64, grad_scale, reduction):
    """loss = mean_b (or sum_b) sum_k -(y / max(||y||, 1e-12))_k log_softmax(l)_k over the LAST rows [n, C]; returns (loss, dlast [n, C],
    d(loss), d(dlast)).  Bounds, with A_k = |l_k - lse|, the exponential's argument rounding amplified by its size, expf / logf at 1 ulp:
      d(lse) <= U (|lse| + |log se|) + (max_k |l_k - max l| + 10) U
      d(per) <= sum_k y_k (d(lse) + 16 U A_k) + 8 U sum_k |y_k (l_k - lse)|
      d(loss) <= (sum_b d(per_b) + n U sum_b |per_b|) / denom + U |loss|                       (the clips are added one by one)
      d(p_k) <= p_k ((A_k + 2) U + d(lse)) + 2^-126,   y and sum y carry 14 U relative
      d(dl_k) <= [d(p_k) sum y + 14 U (p_k sum y + y_k) + 2 U (p_k sum y + y_k)] gs / denom + 2 U |dl_k|"""
    l, tg = last_logits64, last_targets64
    n = l.shape[0]
    denom = float(n) if reduction == "mean" else 1.0
    y = tg / np.maximum(np.sqrt((tg * tg).sum(1, keepdims=True)), 1e-12)
    mx = l.max(1, keepdims=True)
    se = np.exp(l - mx).sum(1, keepdims=True)
    lse = mx + np.log(se)
    per = (-y * (l - lse)).sum(1)
    loss = per.sum() / denom
    ysum = y.sum(1, keepdims=True)
    prob = np.exp(l - lse)
    dl = (prob * ysum - y) * grad_scale / denom
    A = np.abs(l - lse)
    d_lse = U * (np.abs(lse) + np.abs(np.log(se))) + (np.abs(l - mx).max(1, keepdims=True) + 10) * U
    d_per = (np.abs(y) * (d_lse + 16 * U * A)).sum(1) + 8 * U * np.abs(y * (l - lse)).sum(1)
    d_loss = (d_per.sum() + n * U * np.abs(per).sum()) / denom + U * abs(loss)
    d_p = prob * ((A + 2) * U + d_lse) + 2.0 ** -126
    d_dl = (d_p * ysum + 16 * U * (prob * ysum + np.abs(y))) * grad_scale / denom + 2 * U * np.abs(dl)
    return loss, dl, d_loss, d_dl


# ---- AdamW ---------------------------------------------------------------------------------------------------------------------------------------------
def adamw_ref(p, g, m, v, step, lr, b1, b2, eps, wd, mutant=None):
    """one step of torch.optim.AdamW's single-tensor form in fp64 on fp32-valued inputs and fp32-valued hyper-parameters (the ABI takes
    floats: 1 - b2 of the fp32 0.999 differs from 1 - 0.999 by 6e-5 relative, which is the caller's input, not the kernel's error).
    Returns (p', m', v', d(p'), d(m'), d(v')):
      d(m') <= 3 U (|b1 m| + |(1 - b1) g|),  d(v') <= 4 U (|b2 v| + |(1 - b2) g^2|)
      den = sqrt(v') / sqrt(1 - b2^t) + eps:  d(den) <= [d(v') / (2 sqrt v') + 3 U sqrt v'] / sqrt(1 - b2^t) + U den   (v' = 0: d(den) = U eps)
      upd = lr / (1 - b1^t) m' / den:  d(upd) <= |upd| (d(m') / |m'| + d(den) / den + 5 U)
      d(p') <= 3 U |p| + d(upd) + U |p'|"""
    lr, b1, b2, eps, wd = (float(np.float32(x)) for x in (lr, b1, b2, eps, wd))
    bstep = 1 if mutant == "bc_step1" else step
    bc1, bc2s = 1.0 - b1 ** bstep, np.sqrt(1.0 - b2 ** bstep)
    m2 = b1 * m + (1 - b1) * g
    v2 = b2 * v + (1 - b2) * g * g
    den = np.sqrt(v2) / bc2s + eps
    upd = lr / bc1 * m2 / den
    p2 = (p - upd) * (1 - lr * wd) if mutant == "wd_after" else p * (1 - lr * wd) - upd
    d_m = 3 * U * (np.abs(b1 * m) + np.abs((1 - b1) * g))
    d_v = 4 * U * (np.abs(b2 * v) + (1 - b2) * g * g)
    sq = np.sqrt(v2)
    d_den = (np.where(sq > 0, d_v / (2 * np.maximum(sq, 1e-300)), 0.0) + 3 * U * sq) / bc2s + U * den
    d_upd = np.abs(upd) * (d_den / den + 5 * U) + lr / bc1 * d_m / den
    d_p = 3 * U * np.abs(p) + d_upd + U * np.abs(p2)
    return p2, m2, v2, d_p, d_m, d_v
