"""Records tests/golden/vit_workspace_parent.json: what the public *_workspace_bytes functions of a library return, on real handles, for
the shapes of tests/helpers/vit_layouts.py.  Run on a GPU machine against the PARENT commit's library,
    bash scripts/build_old.sh vit_host.cpp vit_stream.cpp && python scripts/record_vit_workspace.py
and commit the file: tests/test_vit_layout_cpu.py holds the tree's layouts to these totals.  Totals only.
usage: python scripts/record_vit_workspace.py [--lib LIB] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prego_amd import _lib                                   # noqa: E402
from tests.helpers import vit_layouts as V                   # noqa: E402

DTYPE = {"bf16": _lib.PREGO_BF16, "f16": _lib.PREGO_F16, "f32": _lib.PREGO_F32}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "prego_amd", "lib_ab", "libold.so"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "vit_workspace_parent.json"))
    args = ap.parse_args()
    lib = _lib._open(args.lib, debug=False)

    def ok(rc):
        if rc != 0:
            raise SystemExit(f"record_vit_workspace: {lib.prego_last_error().decode()}")

    res = {}
    for name, kind, dims, a, b in V.INFERENCE + V.TRAINING:
        dt = DTYPE[name.rsplit("_", 1)[-1]] if name.rsplit("_", 1)[-1] in DTYPE else _lib.PREGO_BF16
        h = C.c_void_p()
        if kind >= V.ATTN16:
            if kind == V.ATTN_OP:
                res[name] = lib.prego_attention_layer_workspace_bytes(a, b, dims[2])
                continue
            ok(lib.prego_attention_layer_create(C.byref(h), dims[2], dims[4]))
            ok(lib.prego_attention_layer_set_compute_dtype(h, dt))
            fn = lib.prego_attention_layer_train_workspace_bytes if kind == V.ATTN_TRAIN else lib.prego_attention_layer_handle_workspace_bytes
            res[name] = fn(h, a, b)
            lib.prego_attention_layer_destroy(h)
            continue
        ok(lib.prego_vit_create(C.byref(h), *dims))
        ok(lib.prego_vit_set_compute_dtype(h, dt))
        if kind in (V.FORWARD16, V.FORWARD32):
            res[name] = lib.prego_vit_workspace_bytes(h, a)
        elif kind == V.FRAMES:
            res[name] = lib.prego_vit_frames_workspace_bytes(h, a, b)
        elif kind == V.STEP_POOL:
            res[name] = lib.prego_vit_step_pool_workspace_bytes(h, a)
        else:
            res[name] = lib.prego_vit_train_workspace_bytes(h, a)
        lib.prego_vit_destroy(h)
    assert all(v > 0 for v in res.values()), res
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    doc = {"what": "totals of the public *_workspace_bytes functions, shapes of tests/helpers/vit_layouts.py", "library_of_commit": commit, "bytes": res}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
