"""Which recurrence kernel a launch runs, and where the exchange layout puts an element, without a device: gru_choose
(csrc/gru_recurrence.hip) through prego_debug_gru_choice against the transcription of the launcher chain it replaced
(tests/helpers/gru_choice.py, written from the sources of the commit before it), and the layout functions of csrc/gru_tile.h through
prego_debug_gru_hx_offset."""
import ctypes as C
import itertools

import pytest

pytest.importorskip("torch")

from tests.helpers import gru_choice as gc                    # noqa: E402

HIDS = (512, 768, 1024, 2048)
ROWS_MAX_OK = ((1 << 31) - 65536 - 1) // 2048                 # the largest rows with rows * 1024 * 2 < 2^31 - 65536
ROWS = (0, 1, ROWS_MAX_OK, ROWS_MAX_OK + 1, 1 << 20)


@pytest.fixture(scope="module")
def lib():
    from prego_amd import _lib
    return _lib.load_debug()


def _ask(lib, *args):
    grid, lds = C.c_int(-7), C.c_int(-7)
    return lib.prego_debug_gru_choice(*args, C.byref(grid), C.byref(lds)), grid.value, lds.value


def _queries():
    for op, hid, nct, gi, train, no_mt, stamps, rows, spec in itertools.product((gc.BF16, gc.F16, gc.F32), HIDS, range(6), (0, 1), (0, 1), (0, 1), (0, 1),
                                                                                  ROWS, (-1, 0, 1)):
        yield (gc.ENTRY_MAIN, op, hid, nct, 8, gi, train, no_mt, stamps, rows, spec, 0, 0)
    for hid, nct, G, ready in itertools.product(HIDS, range(6), (0, 1, 4, 5), (0, 1)):         # fp16x2 operands: their own entry
        yield (gc.ENTRY_X2, gc.OPX2, hid, nct, G, 0, 0, 0, 0, 4096, -1, 0, ready)
    for op, hid, Gd, gi, ready, G in itertools.product((gc.BF16, gc.F16), HIDS, range(9), (0, 1), (0, 1), (8, 4)):
        yield (gc.ENTRY_PASS, op, hid, 1, G, gi, 0, 0, 0, 4096, -1, Gd, ready)


def test_chooser_matches_the_old_chain_over_the_full_product(lib):
    n, families, reasons, bad, dropped = 0, set(), set(), [], 0
    for q in _queries():
        want = gc.old_gru_choice(*q)
        got, grid, lds = _ask(lib, *q)
        n += 1
        if isinstance(want, gc.Refused):
            reasons.add(want.reason)
            ok = got == -1
        elif gc.refused_now(want):
            dropped += 1
            ok = got == -1 and q[1] == gc.F32 and q[2] == 1024 and q[5] == 1
        else:
            families.add(want.family)
            ok = (got, grid, lds) == (gc.pack(want), want.grid, want.lds)
        if not ok and len(bad) < 10:
            bad.append(f"{q}: {got:#x} grid {grid} lds {lds}, the old chain {want}")
    assert not bad, bad
    assert n > 18000 and dropped == 5 * 2 * 2 * 5 * 3            # nct 0 .. 4 x no_mt x stamps x rows x spec of that one combination, nothing else
    assert families == {gc.CLASSIC, gc.MULTI_TILE, gc.X2, gc.PASS}
    assert reasons == gc.REASONS, f"the product does not reach every refusal: {sorted(gc.REASONS - reasons)}"


def test_tile_count_and_spec_of_the_multi_tile_choice(lib):
    """three live tiles run the four-tile instantiation with the tag check inside the multiply; PREGO_GRU_MT_SPEC overrides both ways"""
    for nct, spec, want_n, want_spec in ((2, -1, 2, 0), (3, -1, 4, 1), (4, -1, 4, 1), (2, 1, 2, 1), (4, 0, 4, 0)):
        got, grid, lds = _ask(lib, gc.ENTRY_MAIN, gc.BF16, 1024, nct, 8, 1, 0, 0, 0, 4096, spec, 0, 0)
        assert (got & 3, got >> 6 & 7, got >> 11 & 1, grid) == (gc.MULTI_TILE, want_n, want_spec, 256)
        assert lds == 2 * 4 * 3 * 2 * 64 * 16 + 2 * 4 * 8 * 1024 + 2 * want_n * 3 * 1024


def test_sizes_are_what_they_were(lib):
    f = lib.prego_debug_gru_hx_offset
    for bf16, hid, G in itertools.product((0, 1), HIDS, (1, 4, 8)):
        wb = 2 if bf16 else 4
        assert f(10, wb, 0, hid, G, 0) == gc.old_hx_bytes(bf16, hid, G)
        assert f(11, 2, 0, hid, G, 0) == gc.old_x2_hx_bytes(hid, G)
        assert f(12, wb, 0, hid, 0, 0) == gc.old_group_size(bf16, hid)
        assert bool(f(13, wb, 0, hid, 0, 0)) == gc.old_hidden_supported(bool(bf16), hid)
        assert f(14, 0, 0, 0, G, 0) == gc.old_max_slots(G, False) and f(14, 0, 0, 0, G, 1) == gc.old_max_slots(G, True)


@pytest.mark.parametrize("name,wb,tiles", [("16-bit", 2, 8), ("fp32", 4, 8), ("x2 plane", 2, 4)])
@pytest.mark.parametrize("hid", (512, 1024, 2048))
def test_exchange_layout_is_a_bijection_in_fragment_order(lib, name, wb, tiles, hid):
    f = lib.prego_debug_gru_hx_offset
    kf, epl = (32, 8) if wb == 2 else (16, 4)
    plane = f(3, wb, tiles, hid, 0, 0)
    assert plane == (hid // kf) * tiles * 1024
    seen = bytearray(plane // wb)
    for ct, k, col in itertools.product(range(tiles), range(hid), range(16)):
        off = f(0, wb, tiles, col, k, ct)
        assert 0 <= off < plane and off % wb == 0 and not seen[off // wb], (col, k, ct, off)
        seen[off // wb] = 1
    assert all(seen)                                          # onto: 16 columns x hid units x tiles elements fill the plane
    # the inverse: lane l of a consumer loads 16 bytes at fragment base + 16 l; byte e * wb of them must be B[k][n] of the MFMA with
    # k = frag * KF + (l >> 4) * EPL + e, n = l & 15
    for frag, lane, e in itertools.product(range(hid // kf), range(64), range(epl)):
        k, col = f(1, wb, tiles, frag, lane, e * wb), f(2, wb, tiles, 0, lane, 0)
        assert (k, col) == (frag * kf + (lane >> 4) * epl + e, lane & 15)
        for ct in (0, tiles - 1):
            assert f(0, wb, tiles, col, k, ct) == (frag * tiles + ct) * 1024 + lane * 16 + e * wb
