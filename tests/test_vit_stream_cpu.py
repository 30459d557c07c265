"""CPU side of the Transformer stream pool (prego_amd/stream_pool.py: TransformerStreamPool, csrc/vit_stream.hip): the entry points are
declared and bound, `ring_source` - the host statement of the token rule the ring kernel follows - equals a brute-force model of a
stream's ring for every (frames, token), the slot bookkeeping is `SlotTable`'s, and a CPU model has no pool."""
import os
import re

import pytest

from prego_amd._lib import PregoError
from prego_amd.stream_pool import RING_BIAS, RING_CLS, SlotTable, TransformerStreamPool, ring_source

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(hdr, name, where):
    m = re.search(r"\b(?:int|size_t|void)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in {where}"
    return [a.strip() for a in m.group(1).split(",")]


def test_entry_points_are_declared_and_bound():
    from prego_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "prego_amd.h")).read()
    want = {"prego_vit_stream_pool_bytes": 3, "prego_vit_stream_pool_create": 8, "prego_vit_stream_pool_destroy": 1,
            "prego_vit_step_pool_workspace_bytes": 2, "prego_vit_step_pool": 12, "prego_vit_stream_pool_flush": 4,
            "prego_vit_stream_pool_reset": 4, "prego_vit_stream_pool_record": 4, "prego_vit_stream_pool_window": 5}
    for name, n_args in want.items():
        assert len(_args(hdr, name, "include/prego_amd.h")) == n_args, name
        assert name in _lib.SYMBOLS
    a = _args(hdr, "prego_vit_step_pool", "include/prego_amd.h")
    assert a[1].endswith("p") and a[3].endswith("slots") and a[7].endswith("argmax") and a[9].endswith("workspace") and a[11].endswith("stream")
    assert "#define PREGO_ABI_VERSION 7" in hdr                              # an addition: the ABI version stays
    dhdr = open(os.path.join(ROOT, "include", "prego_amd_debug.h")).read()
    assert len(_args(dhdr, "prego_debug_vit_ring_tokens", "include/prego_amd_debug.h")) == 5
    assert "prego_debug_vit_ring_tokens" in _lib.DEBUG_SYMBOLS and "prego_debug_vit_ring_tokens" not in _lib.SYMBOLS
    assert "prego_debug_vit_ring_tokens" not in hdr
    # every new name has its argtypes in the binding (a missing prototype would pass a 64-bit size or pointer as an int)
    src = open(os.path.join(ROOT, "prego_amd", "_lib.py")).read()
    for name in list(want) + ["prego_debug_vit_ring_tokens"]:
        assert f"lib.{name}.argtypes" in src, name
    for name in ("prego_vit_stream_pool_bytes", "prego_vit_step_pool_workspace_bytes"):
        assert f"lib.{name}.restype = sz" in src, name


@pytest.mark.parametrize("T", [1, 2, 5, 32])
def test_ring_source_equals_a_brute_force_ring(T):
    """the model: frame f is written to row f mod T; the window after `frames` frames holds frames frames - T .. frames - 1 at tokens
    0 .. T - 1, frames below 0 being the zero rows in front of the stream"""
    for frames in range(0, 3 * T + 1):
        ring = [None] * T
        for f in range(frames):
            ring[f % T] = f
        head, fill = frames % T, min(frames, T)
        assert ring_source(head, fill, T, T) == RING_CLS
        for j in range(T):
            f = frames - T + j
            got = ring_source(head, fill, T, j)
            if f < 0:
                assert got == RING_BIAS, (frames, j)
            else:
                assert 0 <= got < T and ring[got] == f, (frames, j, got)
                assert got == (head + j) % T                                # the form the kernel computes (head, j < T: one subtraction)
    for bad in [(0, 0, T, T + 1), (T, 0, T, 0), (0, T + 1, T, 0), (0, 0, T, -1)]:
        with pytest.raises(ValueError):
            ring_source(*bad)


def test_the_pool_keeps_its_slots_in_a_slot_table():
    t = SlotTable(3)
    assert [t.open() for _ in range(3)] == [0, 1, 2]
    t.release(1)
    assert t.open() == 1                                                    # reopen: the lowest free slot
    t.release(0)
    with pytest.raises(PregoError, match="slot 0 is not open"):
        t.check([2, 0], "push")
    with pytest.raises(PregoError, match="slot 2 is named twice"):
        t.check([2, 1, 2], "push")
    assert t.check([2, 1], "push") == [2, 1]
    for name in ("open", "push", "events", "close", "window", "free", "capacity"):
        assert hasattr(TransformerStreamPool, name), name
    for name in ("push_frames", "push_ragged", "vote", "state"):            # bursts and the GRU state are not this pool's
        assert not hasattr(TransformerStreamPool, name), name


def test_a_cpu_model_has_no_pool():
    from prego_amd.config import assembly101_cfg
    from prego_amd.registry import build_model
    import prego_amd.transformer  # noqa: F401
    cfg = assembly101_cfg(model="Transformer", window_size=32, patch_dim=1, num_heads=8, attn_dropout_rate=0.0, dropout=0.0)
    m = build_model(cfg, "cpu")
    with pytest.raises(PregoError, match="no CPU path"):
        m.stream_pool(capacity=4)
    m32 = build_model(dict(cfg, compute_dtype="fp32"), "cpu")
    with pytest.raises(PregoError, match="fp32"):
        m32.stream_pool(capacity=4)
