"""The shapes and layout kinds of the Transformer workspace tests (tests/test_vit_layout_cpu.py, tests/test_gpu_vit_workspace.py) and of
scripts/record_vit_workspace.py, which records tests/golden/vit_workspace_parent.json.  dims = d_rgb, d_flow, embedding_dim, hidden_dim
(mlp), num_heads, num_layers, window_size, n_classes: the argument of prego_debug_vit_layout / prego_debug_vit_tensor."""
import ctypes as C

# kinds of prego_debug_vit_layout (include/prego_amd_debug.h)
FORWARD16, FORWARD32, FRAMES, STEP_POOL, TRAIN, ATTN16, ATTN32, ATTN_TRAIN, ATTN_OP = range(9)

SMALL = (64, 0, 512, 128, 8, 2, 5, 7)            # batch 3: odd sizes, two layers, rows far from any tile multiple
WIDE = (64, 64, 1024, 512, 8, 1, 128, 7)         # batch 16: the benchmark's window and batch
ATTN = (0, 0, 128, 0, 2, 0, 0, 0)                # the attention layer reads d_model (embedding_dim) and heads only; batch 2, len 5

# (name in the golden file, kind, dims, a, b); the public function each one belongs to is in scripts/record_vit_workspace.py
INFERENCE = [
    ("small/forward_bf16", FORWARD16, SMALL, 3, 0), ("small/forward_f16", FORWARD16, SMALL, 3, 0), ("small/forward_f32", FORWARD32, SMALL, 3, 0),
    ("small/frames", FRAMES, SMALL, 9, 4), ("small/step_pool", STEP_POOL, SMALL, 3, 0),
    ("wide/forward_bf16", FORWARD16, WIDE, 16, 0), ("wide/forward_f16", FORWARD16, WIDE, 16, 0), ("wide/forward_f32", FORWARD32, WIDE, 16, 0),
    ("wide/frames", FRAMES, WIDE, 40, 16), ("wide/step_pool", STEP_POOL, WIDE, 16, 0),
    ("attn/handle_bf16", ATTN16, ATTN, 2, 5), ("attn/handle_f16", ATTN16, ATTN, 2, 5), ("attn/handle_f32", ATTN32, ATTN, 2, 5),
    ("attn/stateless", ATTN_OP, ATTN, 2, 5),
]
TRAINING = [("small/train", TRAIN, SMALL, 3, 0), ("wide/train", TRAIN, WIDE, 16, 0), ("attn/train", ATTN_TRAIN, ATTN, 2, 5)]


def layout(lib, kind, dims, a, b=0, cap=257):
    """[(offset, bytes asked for)] of the blocks in order, and the total"""
    out = (C.c_uint64 * cap)()
    n = lib.prego_debug_vit_layout(kind, (C.c_int32 * 8)(*dims), a, b, out, cap)
    assert n > 0, f"prego_debug_vit_layout(kind {kind}) returned {n}"
    return [(out[2 * i], out[2 * i + 1]) for i in range(n)], out[2 * n]


def up(v, a=256):
    return (v + a - 1) // a * a
