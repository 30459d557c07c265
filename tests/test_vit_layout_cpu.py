"""The Transformer workspace layouts without a device (csrc/vit_handle.h: vit_ws, vit_ws32, vit_step_ws, vit_train_ws, attn_ws,
attn_train_ws, attn_op_ws, all on one Arena) through prego_debug_vit_layout: alignment, order, no overlap, the total, and the totals of
the parent commit (tests/golden/vit_workspace_parent.json, recorded from its library by scripts/record_vit_workspace.py): equal for every
inference layout, smaller by exactly the dead blocks for the two training layouts."""
import json
import os

import pytest

pytest.importorskip("torch")

from tests.helpers import vit_layouts as V                    # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = json.load(open(os.path.join(ROOT, "tests", "golden", "vit_workspace_parent.json")))["bytes"]
ALL = V.INFERENCE + V.TRAINING


@pytest.fixture(scope="module")
def lib():
    from prego_amd import _lib
    return _lib.load_debug()


@pytest.mark.parametrize("name,kind,dims,a,b", ALL, ids=[c[0] for c in ALL])
def test_blocks_are_aligned_ordered_disjoint_and_the_total_is_their_end(lib, name, kind, dims, a, b):
    blocks, total = V.layout(lib, kind, dims, a, b)
    end = 0
    for off, size in blocks:
        assert off % 256 == 0 and size > 0
        assert off >= end, f"{name}: a block at {off} starts inside the one before it (ends at {end})"
        end = off + size
    assert total == V.up(end) and total - end < 256
    assert blocks[0][0] == 0


@pytest.mark.parametrize("name,kind,dims,a,b", V.INFERENCE, ids=[c[0] for c in V.INFERENCE])
def test_inference_totals_are_the_parents(lib, name, kind, dims, a, b):
    assert V.layout(lib, kind, dims, a, b)[1] == PARENT[name]


def _dead_vit_train(dims, B):
    """what the parent's vit_train_ws reserved and its backward never touched: T2, WT, and the part of T1 behind the bf16 copy of denc"""
    d_rgb, d_flow, E, mlp, heads, layers, T, ncls = dims
    Mp = V.up(B * (T + 1), 64)
    wide = max(3 * E, mlp, d_rgb + d_flow)
    t1 = V.up(wide * Mp * 2)
    return (t1 - V.up(B * T * E * 2)) + t1 + V.up(3 * E * E * 2)


def _dead_attn_train(dims, B, L):
    """the parent's attn_train_ws: T1, T2, WT, part"""
    D, M = dims[2], B * L
    Mp = V.up(M, 64)
    return 2 * V.up(3 * D * Mp * 2) + V.up(3 * D * D * 2) + V.up((M // 64 + 2) * 3 * D * 4)


@pytest.mark.parametrize("name,kind,dims,a,b", V.TRAINING, ids=[c[0] for c in V.TRAINING])
def test_training_totals_are_the_parents_minus_the_dead_blocks(lib, name, kind, dims, a, b):
    dead = _dead_attn_train(dims, a, b) if kind == V.ATTN_TRAIN else _dead_vit_train(dims, a)
    assert dead > 0
    assert V.layout(lib, kind, dims, a, b)[1] == PARENT[name] - dead


def test_a_short_buffer_and_an_unknown_kind_are_refused(lib):
    import ctypes as C
    out = (C.c_uint64 * 4)()
    dims = (C.c_int32 * 8)(*V.SMALL)
    assert lib.prego_debug_vit_layout(V.FORWARD16, dims, 3, 0, out, 4) == -1
    assert lib.prego_debug_vit_layout(99, dims, 3, 0, out, 4) == -1
    assert lib.prego_debug_vit_layout(V.FORWARD16, None, 3, 0, out, 4) == -1
