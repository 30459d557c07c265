"""The Transformer entries stay inside the workspace they ask for (the canary pattern of tests/test_gpu_step_wide.py): need + 256 bytes of
0xA5, the 256 bytes behind `need` untouched after the call; with need - 1 the call returns PREGO_EWORKSPACE and has written nothing.
prego_vit_forward (bf16, fp32), prego_vit_forward_frames, prego_vit_forward_train + prego_vit_backward with dropout on, and
prego_attention_layer_forward_train + _backward with dx; the training pairs also have finite gradients, which a live block dropped from
the layout by mistake (the layouts lost their dead blocks, csrc/vit_train.cpp, attention_layer.cpp) would not leave."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import _lib                                       # noqa: E402
from tests.helpers import vit_layouts as V                       # noqa: E402

DEV = "cuda:0"
EWORKSPACE = -3
CANARY = 256
B, FRAMES, WPB = 3, 9, 4
ATTN_B, ATTN_L = 2, 5


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _rand(n, seed, scale=0.05):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g) * scale).to(DEV)


@pytest.fixture(scope="module")
def lib():
    return _lib.load_debug()


def _vit(lib, dtype):
    """a ViTEnc handle of the SMALL shape with seeded weights; the caller destroys it"""
    dims = (C.c_int32 * 8)(*V.SMALL)
    r, c, m = C.c_int32(), C.c_int32(), C.c_int32()
    n = lib.prego_debug_vit_tensor(dims, 0, C.byref(r), C.byref(c), C.byref(m))
    ts = []
    for i in range(n):
        lib.prego_debug_vit_tensor(dims, i, C.byref(r), C.byref(c), C.byref(m))
        ts.append(_rand(r.value * c.value, 100 + i))
    h = C.c_void_p()
    assert lib.prego_vit_create(C.byref(h), *V.SMALL) == 0
    assert lib.prego_vit_set_compute_dtype(h, dtype) == 0
    assert lib.prego_vit_num_tensors(h) == n
    assert lib.prego_vit_set_weights(h, _ptrs(ts), n, None) == 0, lib.prego_last_error().decode()
    torch.cuda.synchronize()
    return h, ts


def _canary(need, call, outputs):
    """call(ws, ws_bytes) -> rc, on need + CANARY bytes of 0xA5: fine and inside `need`; refused and nothing written with need - 1"""
    assert need > 0
    ws = torch.full((need + CANARY,), 0xA5, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    for o in outputs:
        o.fill_(float("nan"))
    assert call(ws, need - 1) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool((ws == 0xA5).all()), "a refused call wrote to the workspace"
    assert all(bool(torch.isnan(o).all()) for o in outputs), "a refused call wrote an output"
    rc = call(ws, need)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((ws[need:] == 0xA5).all()), "written past workspace_bytes"
    assert bool((ws[:need] != 0xA5).any())
    assert all(bool(torch.isfinite(o).all()) for o in outputs)


@pytest.mark.parametrize("dtype", (_lib.PREGO_BF16, _lib.PREGO_F32), ids=("bf16", "fp32"))
def test_forward(lib, dtype):
    h, _ = _vit(lib, dtype)
    try:
        T, din, ncls = V.SMALL[6], V.SMALL[0], V.SMALL[7]
        x, out = _rand(B * T * din, 1, 1.0), torch.empty((B, ncls), device=DEV)
        need = lib.prego_vit_workspace_bytes(h, B)
        _canary(need, lambda ws, n: lib.prego_vit_forward(h, B, _p(x), None, _p(out), 0, _p(ws), n, None), [out])
    finally:
        lib.prego_vit_destroy(h)


def test_forward_frames(lib):
    h, _ = _vit(lib, _lib.PREGO_BF16)
    try:
        din, ncls = V.SMALL[0], V.SMALL[7]
        x, out = _rand(FRAMES * din, 2, 1.0), torch.empty((FRAMES, ncls), device=DEV)
        am = torch.full((FRAMES,), -7, dtype=torch.int32, device=DEV)
        need = lib.prego_vit_frames_workspace_bytes(h, FRAMES, WPB)
        _canary(need, lambda ws, n: lib.prego_vit_forward_frames(h, FRAMES, _p(x), None, _p(out), _p(am), WPB, 0, _p(ws), n, None), [out])
        assert torch.equal(am.long(), out.argmax(1))
    finally:
        lib.prego_vit_destroy(h)


def test_forward_train_and_backward_with_dropout(lib):
    h, ts = _vit(lib, _lib.PREGO_BF16)
    try:
        assert lib.prego_vit_set_dropout(h, 0.1, 0.15, 1234) == 0
        T, din, ncls = V.SMALL[6], V.SMALL[0], V.SMALL[7]
        x, out, dl = _rand(B * T * din, 3, 1.0), torch.empty((B, ncls), device=DEV), _rand(B * ncls, 4, 1.0)
        grads = [torch.empty_like(t) for t in ts]

        def call(ws, n):
            rc = lib.prego_vit_forward_train(h, B, _p(x), None, _p(out), 0, _p(ws), n, None)
            rc2 = lib.prego_vit_backward(h, B, _p(dl), _ptrs(grads), len(grads), 0, _p(ws), n, None)
            assert rc == rc2, (rc, rc2)
            return rc

        _canary(lib.prego_vit_train_workspace_bytes(h, B), call, [out] + grads)
        assert all(bool((g != 0).any()) for g in grads)
    finally:
        lib.prego_vit_destroy(h)


def test_attention_layer_forward_train_and_backward(lib):
    D, heads = V.ATTN[2], V.ATTN[4]
    h = C.c_void_p()
    assert lib.prego_attention_layer_create(C.byref(h), D, heads) == 0
    try:
        ws_ = [_rand(D * D if i % 2 == 0 else D, 200 + i) for i in range(8)]        # wq, bq, wk, bk, wv, bv, wo, bo
        assert lib.prego_attention_layer_set_weights(h, *[_p(t) for t in ws_], None) == 0
        M = ATTN_B * ATTN_L
        x, out, dout, dx = _rand(M * D, 5, 1.0), torch.empty((M, D), device=DEV), _rand(M * D, 6, 1.0), torch.empty((M, D), device=DEV)
        grads = [torch.empty_like(t) for t in ws_]

        def call(ws, n):
            rc = lib.prego_attention_layer_forward_train(h, ATTN_B, ATTN_L, 1, _p(x), _p(out), _p(ws), n, None)
            rc2 = lib.prego_attention_layer_backward(h, ATTN_B, ATTN_L, 1, _p(dout), _p(dx), _ptrs(grads), 8, _p(ws), n, None)
            assert rc == rc2, (rc, rc2)
            return rc

        _canary(lib.prego_attention_layer_train_workspace_bytes(h, ATTN_B, ATTN_L), call, [out, dx] + grads)
        assert all(bool((g != 0).any()) for g in grads)
    finally:
        lib.prego_attention_layer_destroy(h)
