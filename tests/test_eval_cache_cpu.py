"""CPU: the switch of Evaluate's device feature cache (cfg['eval_cache_device'], prego_amd/eval_cache.py).  There is no device memory to
keep anything in on a CPU device, so the cache must say so and every call must run from the loader exactly as without the switch; the
stand-in model is the one of tests/test_distributed_cpu.py (oracle port underneath)."""
import json
import logging
import os
import re

import numpy as np
import torch

from tests.test_distributed_cpu import _FakeModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _CountingLoader:
    def __init__(self, items):
        self.items, self.iterations = items, 0

    def __iter__(self):
        self.iterations += 1
        return iter(self.items)


def _setup(tmp_path, name, **extra):
    from prego_amd import weights as W
    from prego_amd.config import epic_tent_cfg
    from prego_amd.evaluate import Evaluate
    from oracle.oracle_torch import TorchPort
    vl = os.path.join(tmp_path, "vl.json")
    json.dump({"EPIC-TENT-O": {"class_index": [f"c{i}" for i in range(12)]}}, open(vl, "w"))
    cfg = epic_tent_cfg(eval="x.pth", video_list_path=vl, eval_output_dir=os.path.join(tmp_path, name), **extra)
    model = _FakeModel(TorchPort(W.miniroad_state_dict(cfg, 20, head_gain=8.0), 1024))
    items = []
    for i, T in enumerate([30, 11, 25, 18, 9]):
        tgt = np.zeros((T, 12), np.float32)
        tgt[np.arange(T), (np.arange(T) // 5 + i) % 12] = 1
        items.append((torch.from_numpy(W.tsn_features((T, 2048), 9, f"ec.{i}"))[None], torch.zeros(1, T, 2048), torch.from_numpy(tgt)[None],
                      (f"v{i}",), torch.tensor([0]), torch.tensor([T])))
    return Evaluate(cfg), model, _CountingLoader(items), os.path.join(tmp_path, name, "output_miniROAD.json")


def test_switch_off_is_the_default_and_reports_itself(tmp_path):
    ev, model, loader, out = _setup(str(tmp_path), "off")
    assert ev.cache_info()["enabled"] is False
    ev(model, loader, logging.getLogger("t"), "cpu")
    ev(model, loader, logging.getLogger("t"), "cpu")
    assert ev.last_source == "loader" and loader.iterations == 2
    info = ev.cache_info()
    assert info["enabled"] is False and info["state"] == "disabled" and info["videos"] == 0 and info["bytes"] == 0
    ev.drop_cache()                                          # nothing to drop: not an error


def test_switch_on_a_cpu_device_changes_nothing_and_says_why(tmp_path):
    ev0, model, loader0, out0 = _setup(str(tmp_path), "off")
    want = float(ev0(model, loader0, logging.getLogger("t"), "cpu"))
    want_json = open(out0, "rb").read()
    ev, model, loader, out = _setup(str(tmp_path), "on", eval_cache_device=True)
    for call in (1, 2, 3):
        got = float(ev(model, loader, logging.getLogger("t"), "cpu"))
        assert got == want and open(out, "rb").read() == want_json
        assert ev.last_source == "loader" and loader.iterations == call
        info = ev.cache_info()
        assert info["enabled"] is True and info["state"] == "disabled" and info["reason"] == "cpu"
        assert info["videos"] == 0 and info["frames"] == 0 and info["bytes"] == 0 and info["dtype"] is None


def test_header_declares_the_cast_entry_point():
    from prego_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "prego_amd.h")).read()
    m = re.search(r"int\s+prego_cast_features\s*\(([^)]*)\)\s*;", hdr)
    assert m, "prego_cast_features is not declared in include/prego_amd.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert args == ["const float* src", "void* dst", "int64_t n", "int dtype", "prego_stream_t stream"]
    assert "prego_cast_features" in _lib.SYMBOLS                  # test_host_cpu checks every SYMBOLS entry against the library's exports
    assert re.search(r"#define\s+PREGO_ABI_VERSION\s+7\b", hdr)  # an addition: the ABI version stays


def test_cast_entry_point_refuses_bad_arguments_before_it_touches_a_device():
    """the argument checks of prego_cast_features come before any HIP call, so they answer on a box without a GPU too: PREGO_EINVAL (-1)
    with a message; n == 0 is not an error and launches nothing"""
    import ctypes as C
    from prego_amd import _lib
    lib = _lib.load()
    buf = (C.c_char * 4096)()
    s = (C.addressof(buf) + 15) // 16 * 16
    d = s + 2048
    call = lambda src, dst, n, dtype: lib.prego_cast_features(C.c_void_p(src), C.c_void_p(dst), n, dtype, None)
    assert call(s, d, 0, _lib.PREGO_BF16) == 0
    for what, args in {"NULL src": (None, d, 64, 1), "NULL dst": (s, None, 64, 1), "negative n": (s, d, -8, 1), "n % 8": (s, d, 12, 1),
                       "misaligned src": (s + 4, d, 64, 1), "misaligned dst": (s, d + 2, 64, 2), "fp32": (s, d, 64, _lib.PREGO_F32),
                       "fp16x2": (s, d, 64, _lib.PREGO_F16X2), "unknown dtype": (s, d, 64, 9), "dst inside src": (s, s + 64, 64, 1),
                       "src inside dst": (d, d - 16, 64, 2)}.items():
        assert call(*args) == -1, what
        assert b"cast_features" in lib.prego_last_error(), what


def test_cache_bookkeeping_with_stand_in_tensors():
    """EvalFeatureCache's own rules, on CPU tensors that already hold the kept dtype (so nothing is converted): bytes counted video by
    video, the video that would pass the budget releases everything, the key (dataset object + signature), the loader-item grouping the
    evaluator's loop sees again, and that a filling call that raised leaves nothing behind"""
    import types
    from prego_amd.eval_cache import EvalFeatureCache, EvalVideo
    dev, log = types.SimpleNamespace(type="cuda"), logging.getLogger("t")

    class _DS:
        pass

    ds = _DS()

    def fill(c, sig=("sig",)):
        assert c.begin(ds, sig, dev, torch.float32, log) is False and c.filling
        for first, lens in ((0, [3, 5, 2]), (3, [4])):
            items = [EvalVideo(torch.ones(T, 8), None if (first + i) % 2 else torch.ones(T, 8), None, f"v{first + i}", first + i, (first + i) // 2)
                     for i, T in enumerate(lens)]
            c.retain(items, [b.features for b in items], [b.flow for b in items], [torch.zeros(b.features.shape[0], dtype=torch.int32) for b in items], dev)

    c = EvalFeatureCache(10 ** 9)
    fill(c)
    assert c.info()["state"] == "empty"                                # not a cache before the filling call has ended
    c.commit()
    need = (3 + 5 + 2 + 4) * 8 * 4 + (3 + 2) * 8 * 4 + 14 * 4       # rgb of every video, flow of videos 0 and 2, one int32 id per frame
    assert c.info() == dict(enabled=True, state="filled", reason=None, videos=4, frames=14, bytes=need, dtype="fp32")
    assert c.begin(ds, ("sig",), dev, torch.float32, log) is True
    assert [[e.name for e in g] for g in c.videos()] == [["v0", "v1"], ["v2", "v3"]]      # two videos per loader item, as they came
    assert [e.flow is None for g in c.videos() for e in g] == [False, True, False, True]
    fill(c, ("another signature",))                                    # a mismatch drops and refills ...
    c.abort()                                                          # ... and a filling call that raised keeps nothing
    assert c.info()["state"] == "empty" and c.info()["bytes"] == 0 and c.info()["videos"] == 0
    for limit, state in ((need - 1, "disabled"), (need, "filled")):
        c = EvalFeatureCache(limit)
        fill(c)
        c.commit()
        info = c.info()
        assert info["state"] == state and info["bytes"] == (need if state == "filled" else 0)
        assert (state == "filled") or ("budget" in info["reason"] and info["videos"] == 0)
        assert c.begin(ds, ("sig",), dev, torch.float32, log) is (state == "filled") and not c.filling      # disabled: from the loader, no refill
        c.drop()
        assert c.begin(ds, ("sig",), dev, torch.float32, log) is False and c.filling                        # drop_cache(): fills again
    plain = [1, 2]                                                      # no weak reference to a list: its identity is the key all the same
    c = EvalFeatureCache(1)
    c.begin(plain, ("sig",), dev, torch.float32, log)
    c.commit()
    assert c.begin(plain, ("sig",), dev, torch.float32, log) is True and c.begin(list(plain), ("sig",), dev, torch.float32, log) is False
