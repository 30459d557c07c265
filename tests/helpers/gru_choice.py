"""What the GRU recurrence launchers ran before gru_choose (csrc/gru_recurrence.hip) replaced them: a transcription, branch by branch,
of launch_gru_recurrence, launch_gru_recurrence_other<HID>, launch_gru_recurrence_pass and launch_gru_recurrence_x2 with their LAUNCH /
LAUNCH_O / LAUNCH_T / LAUNCH_MT macro trees, written from the sources of the commit before the chooser (gru_recurrence.hip and
gru_recurrence_x2.hip there), and of the size functions beside them.  tests/test_gru_choice_cpu.py holds the chooser to it.

An answer is (family, operand, UT, NCT, TRAIN, GI16, SPEC, hid, grid, lds) or Refused(reason); `pack` gives the int that
prego_debug_gru_choice returns for it."""
from collections import namedtuple

ENTRY_MAIN, ENTRY_X2, ENTRY_PASS = 0, 1, 2
CLASSIC, MULTI_TILE, X2, PASS = 0, 1, 2, 3
BF16, F16, F32, OPX2 = 0, 1, 2, 3
Choice = namedtuple("Choice", "family op ut nct train gi16 spec hid grid lds")
Refused = namedtuple("Refused", "reason")
REASONS = {"hidden size", "more than four tiles", "fp16 operands keep nothing", "other: keeps with 16-bit GI or fp16", "other: 16-bit operands, fp32 GI",
           "other: fp32 operands, 16-bit GI", "x2: shape", "x2: tiles", "pass: shape"}


def refused_now(c):
    """the one answer of the old chain that gru_choose does not give: fp32 operands with 16-bit GI at hidden size 1024 ran the classic GI16
    kernel.  inter16() needs 16-bit operands, so no caller could ask; the kernel is no longer instantiated and the chooser refuses"""
    return isinstance(c, Choice) and c.family == CLASSIC and c.op == F32 and c.gi16


def pack(c):
    if isinstance(c, Refused):
        return -1
    return c.family | c.op << 2 | c.ut << 4 | c.nct << 6 | int(c.train) << 9 | int(c.gi16) << 10 | int(c.spec) << 11 | c.hid << 12


def old_hx_bytes(bf16, hid, G):
    return 2 * G * (hid // 32 if bf16 else hid // 16) * 8 * 1024            # GRU_MAX_TILES 8


def old_x2_hx_bytes(hid, G):
    return 2 * G * 4 * (hid // 32) * 4 * 1024                               # X2_TILES 4


def old_group_size(bf16, hid):
    return hid // (32 if bf16 and hid <= 1024 else 16)


def old_hidden_supported(bf16, hid):
    return hid == 1024 or hid == 512 or (bf16 and hid == 2048)


def old_max_slots(G, x2):
    return G * 16 * (2 if x2 else 4)                                        # max_slots_of: G * 16 * (x2 ? 2 : gru_max_tiles()), which returned 4


def _classic_lds(ut):
    return 2 * 4 * 3 * ut * 64 * 16


def _tiles(nct):
    """if (nct == 1) ...1; else if (nct == 2) ...2; else if (nct <= 4) ...4; else return -1 - so 0 and 3 ran the four-tile kernel"""
    return 1 if nct == 1 else 2 if nct == 2 else 4 if nct <= 4 else None


def _old_other(hid, bf16, f16, nct, gi_bf16, train, grid):
    utb = 2 if hid <= 1024 else 1
    if train:                                                               # LAUNCH_T
        if gi_bf16 or f16:
            return Refused("other: keeps with 16-bit GI or fp16")
        if not bf16 and hid > 512:
            return Refused("hidden size")
        op, ut = (BF16, utb) if bf16 else (F32, 1)
        n = _tiles(nct)
        return Choice(CLASSIC, op, ut, n, True, False, False, hid, grid, _classic_lds(ut)) if n else Refused("more than four tiles")
    if bf16:                                                                # LAUNCH_O
        if not gi_bf16:
            return Refused("other: 16-bit operands, fp32 GI")
        n = _tiles(nct)
        return Choice(CLASSIC, F16 if f16 else BF16, utb, n, False, True, False, hid, grid, _classic_lds(utb)) if n else Refused("more than four tiles")
    if hid > 512:
        return Refused("hidden size")
    if gi_bf16:
        return Refused("other: fp32 operands, 16-bit GI")
    n = _tiles(nct)
    return Choice(CLASSIC, F32, 1, n, False, False, False, hid, grid, _classic_lds(1)) if n else Refused("more than four tiles")


def _old_main(bf16, f16, hid, nct, G, gi_bf16, train, no_mt, stamps, rows, mt_spec):
    if hid != 1024:
        if not old_hidden_supported(bf16, hid):
            return Refused("hidden size")
        return _old_other(hid, bf16, f16, nct, gi_bf16, train, G * old_group_size(bf16, hid))
    grid = G * (32 if bf16 else 64)
    stamps_ok = not stamps                                                  # a build without GRU_MT_STAMPS
    rows_ok = rows > 0 and rows * hid * 2 < (1 << 31) - 65536
    if bf16 and gi_bf16 and 2 <= nct <= 4 and not train and not no_mt and stamps_ok and rows_ok:
        spec = (mt_spec != 0) if mt_spec >= 0 else nct >= 3
        n = 2 if nct == 2 else 4
        lds = 2 * 4 * 3 * 2 * 64 * 16 + 2 * 4 * 8 * 1024 + 2 * n * 3 * 1024
        return Choice(MULTI_TILE, F16 if f16 else BF16, 2, n, False, True, spec, 1024, grid, lds)
    if bf16 and f16:
        if train:
            return Refused("fp16 operands keep nothing")
        op, ut = F16, 2
    elif bf16:
        op, ut = BF16, 2
    else:
        op, ut = F32, 1
    n = _tiles(nct)
    if not n:
        return Refused("more than four tiles")
    # LAUNCH: train ? <.., true> : gi_bf16 ? <.., false, true> : <.., false>
    return Choice(CLASSIC, op, ut, n, bool(train), bool(gi_bf16) and not train, False, 1024, grid, _classic_lds(ut))


def old_gru_choice(entry, operand, hid, nct, G, gi_bf16, train, no_mt, stamps, rows, mt_spec, Gd, ready):
    """the arguments of prego_debug_gru_choice"""
    if entry == ENTRY_X2:
        if hid != 1024 or G < 1 or G > 4 or not ready:
            return Refused("x2: shape")
        if nct not in (1, 2):
            return Refused("x2: tiles")
        return Choice(X2, OPX2, 1, nct, False, False, False, 1024, G * 64, 2 * 4 * 3 * 64 * 16)
    if entry == ENTRY_PASS:
        if hid != 1024 or G != 8 or Gd < 1 or Gd >= 8 or not gi_bf16 or not ready:
            return Refused("pass: shape")
        return Choice(PASS, F16 if operand == F16 else BF16, 2, 1, False, True, False, 1024, 256, 2 * 4 * 3 * 2 * 64 * 16)
    return _old_main(operand != F32, operand == F16, hid, nct, G, gi_bf16, train, no_mt, stamps, rows, mt_spec)
