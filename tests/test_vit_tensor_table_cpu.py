"""The ViTEnc handle's tensor table (csrc/vit_host.cpp: vit_tensors, the one enumeration behind prego_vit_set_weights, the gradient list of
prego_vit_backward and prego_vit_adamw_step) without a device, through prego_debug_vit_tensor: as many entries as _tensor_order names,
entry i with the shape of that state_dict tensor, and exactly the encoding weight and the four per-layer projection weights as matrices."""
import ctypes as C

import pytest

pytest.importorskip("torch")

from prego_amd import weights as W                            # noqa: E402
from prego_amd.config import FEATURE_SIZES, assembly101_cfg, flow_dim, rgb_dim  # noqa: E402
from prego_amd.transformer import _tensor_order               # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from prego_amd import _lib
    return _lib.load_debug()


def _entry(lib, dims, i):
    r, c, m = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    n = lib.prego_debug_vit_tensor((C.c_int32 * 8)(*dims), i, C.byref(r), C.byref(c), C.byref(m))
    return n, r.value, c.value, m.value


@pytest.mark.parametrize("layers", (1, 3))
def test_table_is_the_state_dict_in_tensor_order(lib, layers, monkeypatch):
    monkeypatch.setitem(FEATURE_SIZES, "rgb_64", 64)          # a feature size of this test's own: din 64
    cfg = assembly101_cfg(model="Transformer", window_size=5, patch_dim=1, num_heads=8, embedding_dim=512, hidden_dim=128, num_layers=layers,
                          num_classes=7, rgb_type="rgb_64", no_flow=True)
    assert rgb_dim(cfg) + flow_dim(cfg) == 64
    dims = (rgb_dim(cfg), flow_dim(cfg), 512, 128, 8, layers, 5, 7)
    sd, names = W.vit_state_dict(cfg), _tensor_order(layers)
    assert len(names) == 4 + 11 * layers + 4
    matrices = {"linear_encoding.weight"} | {n for n in names if n.endswith(("qkv.weight", "proj.weight", "net.0.weight", "net.3.weight"))}
    assert len(matrices) == 1 + 4 * layers
    for i, name in enumerate(names):
        n, rows, cols, is_matrix = _entry(lib, dims, i)
        assert n == len(names)
        t = sd[name]
        assert rows * cols == t.size, name
        if name in matrices:
            assert is_matrix == 1 and (rows, cols) == t.shape, name
        else:
            assert is_matrix == 0 and (rows, cols) == (1, t.size), name
    for i in (-1, len(names)):                                 # outside the table: the count, nothing written
        assert _entry(lib, dims, i) == (len(names), -1, -1, -1)
    assert lib.prego_debug_vit_tensor(None, 0, None, None, None) == -1
