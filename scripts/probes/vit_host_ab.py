"""Bit-for-bit A/B of the Transformer host files (csrc/vit_host.cpp, vit_train.cpp, attention_layer.cpp, vit_stream.cpp's block loop): the
tree's debug library against prego_amd/lib_ab/libold.so (the parent commit: bash scripts/build_old.sh vit_host.cpp vit_stream.cpp), both
opened in one process, the same seeded inputs and weights, torch.equal on every output.  The kernels are the same objects in both, so a
mismatch is a launch or an argument that the host code changed.
  prego_vit_forward           bf16 / fp16 / fp32, layers 1 and 2, causal and not, B*T = 15 (token kernel) and 4096 (tokens in the encoding
                              GEMM's epilogue: window 128, batch 32, emb 512); flags bit 1 (every row through the last block) once
  prego_vit_forward_frames    layers 1 (fused token kernel) and 2, 9 frames, 4 windows per batch: logits and argmax
  training                    forward_train -> backward with dropout (0.1, 0.15), layers 1 and 2: logits and every gradient tensor
  prego_vit_adamw_step        one step: params, both moments, and a forward afterwards (reads the refreshed operand copies)
  attention layer             handle forward in three dtypes, stateless forward, forward_train -> backward with dropout 0.1 and dx
One JSON line: comparisons, mismatches.  usage: python scripts/probes/vit_host_ab.py [--old LIB] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch                                                 # noqa: E402

from prego_amd import _lib                                   # noqa: E402

vp = C.c_void_p
DEV = "cuda:0"
DT = {"bf16": _lib.PREGO_BF16, "fp16": _lib.PREGO_F16, "fp32": _lib.PREGO_F32}


def p(t):
    return vp(t.data_ptr()) if t is not None else None


def ptrs(ts):
    return (vp * len(ts))(*[t.data_ptr() for t in ts])


def rand(n, seed, scale=0.05):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def tensor_sizes(d_rgb, d_flow, E, mlp, heads, layers, T, ncls):
    """element counts in set_weights order (transformer.py: _tensor_order)"""
    per = [E, E, 3 * E * E, E * E, E, E, E, mlp * E, mlp, E * mlp, E]
    return [E * (d_rgb + d_flow), E, E, (T + 1) * E] + per * layers + [E, E, ncls * E, ncls]


class Vit:
    def __init__(self, lib, dims, dtype):
        self.lib, self.dims, self.h = lib, dims, vp()
        self.ok(lib.prego_vit_create(C.byref(self.h), *dims))
        self.ok(lib.prego_vit_set_compute_dtype(self.h, DT[dtype]))
        self.w = [rand(n, 100 + i) for i, n in enumerate(tensor_sizes(*dims))]
        self.ok(lib.prego_vit_set_weights(self.h, ptrs(self.w), len(self.w), None))

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(self.lib.prego_last_error().decode())

    def ws(self, nbytes):
        return torch.zeros(nbytes, dtype=torch.uint8, device=DEV)

    def forward(self, B, flags):
        d_rgb, d_flow, T, ncls = self.dims[0], self.dims[1], self.dims[6], self.dims[7]
        rgb = rand(B * T * d_rgb, 1, 1.0)
        flow = rand(B * T * d_flow, 2, 1.0) if d_flow else None
        out = torch.full((B, ncls), float("nan"), device=DEV)
        ws = self.ws(self.lib.prego_vit_workspace_bytes(self.h, B))
        self.ok(self.lib.prego_vit_forward(self.h, B, p(rgb), p(flow), p(out), flags, p(ws), ws.numel(), None))
        return [out]

    def frames(self, n, wb):
        d_rgb, ncls = self.dims[0], self.dims[7]
        rgb, out = rand(n * d_rgb, 3, 1.0), torch.full((n, ncls), float("nan"), device=DEV)
        am = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        ws = self.ws(self.lib.prego_vit_frames_workspace_bytes(self.h, n, wb))
        self.ok(self.lib.prego_vit_forward_frames(self.h, n, p(rgb), None, p(out), p(am), wb, 1, p(ws), ws.numel(), None))
        return [out, am]

    def train(self, B):
        d_rgb, T, ncls = self.dims[0], self.dims[6], self.dims[7]
        self.ok(self.lib.prego_vit_set_dropout(self.h, 0.1, 0.15, 4321))
        rgb, out, dl = rand(B * T * d_rgb, 4, 1.0), torch.full((B, ncls), float("nan"), device=DEV), rand(B * ncls, 5, 1.0)
        grads = [torch.full_like(t, float("nan")) for t in self.w]
        ws = self.ws(self.lib.prego_vit_train_workspace_bytes(self.h, B))
        self.ok(self.lib.prego_vit_forward_train(self.h, B, p(rgb), None, p(out), 1, p(ws), ws.numel(), None))
        self.ok(self.lib.prego_vit_backward(self.h, B, p(dl), ptrs(grads), len(grads), 1, p(ws), ws.numel(), None))
        return [out] + grads

    def adamw(self, B):
        grads = [rand(t.numel(), 300 + i, 1.0) for i, t in enumerate(self.w)]
        m = [rand(t.numel(), 400 + i, 0.01) for i, t in enumerate(self.w)]
        v = [rand(t.numel(), 500 + i, 0.01).abs() for i, t in enumerate(self.w)]
        self.ok(self.lib.prego_vit_adamw_step(self.h, ptrs(self.w), ptrs(grads), ptrs(m), ptrs(v), len(self.w), 3, 1e-3, 0.9, 0.999, 1e-8, 0.05, None))
        return self.w + m + v + self.forward(B, 0)

    def close(self):
        self.lib.prego_vit_destroy(self.h)


def attention(lib, what, dtype="bf16"):
    D, heads, B, L = 128, 2, 2, 5
    M = B * L
    w = [rand(D * D if i % 2 == 0 else D, 200 + i) for i in range(8)]            # wq, bq, wk, bk, wv, bv, wo, bo
    x, out = rand(M * D, 6, 1.0), torch.full((M, D), float("nan"), device=DEV)

    def ok(rc):
        if rc != 0:
            raise RuntimeError(lib.prego_last_error().decode())

    if what == "stateless":
        ws = torch.zeros(lib.prego_attention_layer_workspace_bytes(B, L, D), dtype=torch.uint8, device=DEV)
        ok(lib.prego_attention_layer_forward(B, L, D, heads, 1, p(x), *[p(t) for t in w], p(out), p(ws), ws.numel(), None))
        return [out]
    h = vp()
    ok(lib.prego_attention_layer_create(C.byref(h), D, heads))
    try:
        ok(lib.prego_attention_layer_set_compute_dtype(h, DT[dtype]))
        ok(lib.prego_attention_layer_set_weights(h, *[p(t) for t in w], None))
        if what == "handle":
            ws = torch.zeros(lib.prego_attention_layer_handle_workspace_bytes(h, B, L), dtype=torch.uint8, device=DEV)
            ok(lib.prego_attention_layer_handle_forward(h, B, L, 1, p(x), p(out), p(ws), ws.numel(), None))
            return [out]
        ok(lib.prego_attention_layer_set_dropout(h, 0.1, 99))
        dout, dx = rand(M * D, 7, 1.0), torch.full((M, D), float("nan"), device=DEV)
        grads = [torch.full_like(t, float("nan")) for t in w]
        ws = torch.zeros(lib.prego_attention_layer_train_workspace_bytes(h, B, L), dtype=torch.uint8, device=DEV)
        ok(lib.prego_attention_layer_forward_train(h, B, L, 1, p(x), p(out), p(ws), ws.numel(), None))
        ok(lib.prego_attention_layer_backward(h, B, L, 1, p(dout), p(dx), ptrs(grads), 8, p(ws), ws.numel(), None))
        return [out, dx] + grads
    finally:
        torch.cuda.synchronize()
        lib.prego_attention_layer_destroy(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=os.path.join(ROOT, "prego_amd", "lib_ab", "libold.so"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vit_host_ab: no GPU")
    libs = {"new": _lib.load_debug(), "old": _lib._open(args.old, debug=False)}
    n_cmp, bad, cases = 0, [], []

    def both(what, fn):
        nonlocal n_cmp
        res = {}
        for name, lib in libs.items():
            res[name] = [t.clone() for t in fn(lib)]
            torch.cuda.synchronize()
        assert len(res["new"]) == len(res["old"])
        cases.append(what)
        for i, (a, b) in enumerate(zip(res["new"], res["old"])):
            n_cmp += 1
            if not torch.equal(a, b) or (a.is_floating_point() and not bool(torch.isfinite(a).all())):
                bad.append(f"{what} [output {i}]")

    def vit(dims, dtype, fn):
        def run(lib):
            m = Vit(lib, dims, dtype)
            try:
                out = fn(m)
                torch.cuda.synchronize()
                return out
            finally:
                m.close()
        return run

    small = lambda layers: (64, 0, 512, 128, 8, layers, 5, 7)
    big = lambda layers: (64, 64, 512, 128, 8, layers, 128, 7)
    for dtype in DT:
        for layers in (1, 2):
            for causal in (0, 1):
                both(f"forward {dtype} layers {layers} causal {causal} B*T 15", vit(small(layers), dtype, lambda m: m.forward(3, causal)))
                both(f"forward {dtype} layers {layers} causal {causal} B*T 4096", vit(big(layers), dtype, lambda m: m.forward(32, causal)))
    both("forward bf16 layers 2, every row through the last block", vit(small(2), "bf16", lambda m: m.forward(3, 2)))
    for layers in (1, 2):
        for dtype in ("bf16", "fp16"):
            both(f"forward_frames {dtype} layers {layers}", vit(small(layers), dtype, lambda m: m.frames(9, 4)))
        both(f"forward_train + backward layers {layers}, dropout 0.1 / 0.15", vit(small(layers), "bf16", lambda m: m.train(3)))
    both("adamw step, then forward", vit(small(2), "bf16", lambda m: m.adamw(3)))
    for dtype in DT:
        both(f"attention handle forward {dtype}", lambda lib: attention(lib, "handle", dtype))
    both("attention stateless forward", lambda lib: attention(lib, "stateless"))
    both("attention forward_train + backward, dropout 0.1", lambda lib: attention(lib, "train"))
    doc = {"probe": "vit_host_ab", "cases": len(cases), "comparisons": n_cmp, "mismatches": bad, "case_list": cases}
    line = json.dumps(doc)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(doc, indent=1) + "\n")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
