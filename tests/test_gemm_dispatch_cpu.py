"""Which kernel an NT product runs on, without a device: gemm_nt_choose (csrc/gemm.hip) through prego_debug_gemm_nt_choice against the
transcription of the launcher chain that the chooser replaced (tests/helpers/gemm_exact.py: old_nt_choice, written from the sources of
the commit before it).  The full product of shapes, bias, operand type, train_splitk and epilogue x output width, under every
combination of the three knobs (an argument of the debug entry: the environment is read once per process)."""
import itertools

import pytest

pytest.importorskip("torch")

from tests.helpers import gemm_exact as gx                    # noqa: E402

MS = (0, 1, 128, 2047, 2048, 4095, 4096, 4097, 32768, 70001)
NS = (128, 256, 384, 8192, 8448)
KS = (64, 128, 192, 960, 1024, 1088)
MODES = (gx.EPI_STORE, gx.EPI_RESIDUAL, gx.EPI_GELU_BF16, gx.EPI_STORE_BF16, gx.EPI_QKV, gx.EPI_TOKENS)
NAMES = {gx.K128: "128x128", gx.K256X128: "256x128", gx.K256SQ: "256x256", gx.KPINGPONG: "ping-pong", gx.KSPLITK: "split-K", gx.KNONE: "none"}


def _entries(mode, out16, f16):
    """the call paths that carry (mode, output width) in production: a plain fp32 projection enters through launch_gemm_bf16_nt, a
    projection with a 16-bit C (or fp16 operands) through the MiniROAD forward's proj, and every mode through launch_gemm_bf16_nt_epi"""
    if mode == gx.EPI_STORE:
        if out16:
            return [(gx.ENTRY_PROJ16, gx.EPI_STORE_BF16)]
        return [(gx.ENTRY_PLAIN, mode), (gx.ENTRY_EPI, mode)] + ([(gx.ENTRY_PROJ16, mode)] if f16 else [])
    if mode == gx.EPI_STORE_BF16:
        return [(gx.ENTRY_PROJ16, mode), (gx.ENTRY_EPI, mode)] if out16 else []          # a 16-bit store has no fp32 form
    return [(gx.ENTRY_EPI, mode)]                                                        # the width is the mode's own: out16 changes nothing


def _choice(lib, entry, M, N, K, lda, ldb, bias, f16, splitk, mode, dh, emb, knobs):
    return lib.prego_debug_gemm_nt_choice(entry, M, N, K, lda, ldb, bias, f16, splitk, mode, dh, emb, knobs)


@pytest.fixture(scope="module")
def lib():
    from prego_amd import _lib
    return _lib.load_debug()


@pytest.mark.parametrize("knobs", range(8), ids=lambda k: "knobs-" + "".join(n for b, n in ((1, "B"), (2, "S"), (4, "P")) if k & b) if k else "knobs-none")
def test_chooser_matches_the_old_chain_over_the_full_product(lib, knobs):
    n, seen, bad = 0, set(), []
    for M, N, K, bias, f16, splitk, mode, out16 in itertools.product(MS, NS, KS, (1, 0), (0, 1), (0, 1), MODES, (0, 1)):
        for entry, emode in _entries(mode, out16, f16):
            if entry == gx.ENTRY_PLAIN or entry == gx.ENTRY_PROJ16:
                sk = splitk                                   # proj passes the keeping forward's flag on both of its branches
            else:
                sk = 0
            args = (entry, M, N, K, K, K, bias, f16, sk, emode, 64, 1024, knobs)
            got, want = _choice(lib, *args), gx.old_nt_choice(*args)
            n += 1
            seen.add(want)
            if got != want and len(bad) < 10:
                bad.append(f"entry {entry} M {M} N {N} K {K} bias {bias} f16 {f16} train_splitk {sk} mode {emode}: {NAMES.get(got, got)}, the old chain {NAMES[want]}")
    assert not bad, bad
    assert n > 20000
    if knobs == 0:
        assert seen == set(NAMES), f"the product does not reach every answer: {sorted(seen)}"


@pytest.mark.parametrize("knobs", (0, 4))
def test_qkv_head_width_and_leading_dimensions(lib, knobs):
    """EPI_QKV with dh % 8 or emb % 8 is refused by ping-pong and falls to the 128 x 128 kernel; the split-K launcher's conditions on
    the leading dimensions (multiples of 8, byte offsets within 31 bits) are part of the choice"""
    for M, N, K, bias, f16, (dh, emb) in itertools.product((4095, 4096, 70001), (256, 384), (64, 128), (0, 1), (0, 1), ((64, 1024), (20, 1000), (64, 1004), (4, 256))):
        args = (gx.ENTRY_EPI, M, N, K, K, K, bias, f16, 0, gx.EPI_QKV, dh, emb, knobs)
        assert _choice(lib, *args) == gx.old_nt_choice(*args), args
    if knobs == 0:
        assert _choice(lib, gx.ENTRY_EPI, 4096, 256, 128, 128, 128, 0, 0, 0, gx.EPI_QKV, 20, 1000, 0) == gx.K128
        assert _choice(lib, gx.ENTRY_EPI, 4096, 256, 128, 128, 128, 0, 0, 0, gx.EPI_QKV, 64, 1024, 0) == gx.KPINGPONG
    for M, N, K, lda, ldb in [(2048, 1024, 1024, 1024, 1024), (2048, 1024, 1024, 1028, 1024), (2048, 1024, 1024, 1024, 1036), (2048, 1024, 1024, 1032, 1040),
                              (2048, 1024, 1024, 1 << 20, 1024), (2048, 1024, 1024, 1024, 1 << 21), (128, 128, 1024, 1 << 23, 1 << 23), (2048, 1024, 1024, 0, 1024)]:
        args = (gx.ENTRY_PLAIN, M, N, K, lda, ldb, 1, 0, 1, gx.EPI_STORE, 0, 0, knobs)
        assert _choice(lib, *args) == gx.old_nt_choice(*args), args
