"""Bit-for-bit A/B of the NT GEMM family (csrc/gemm_tile.h, gemm.hip, gemm_pp.hip, gemm_tn.hip, ff_pass.hip and their host callers): the
tree's debug library against prego_amd/lib_ab/libold_debug.so, both opened in one process, raw output bytes compared.  Build the old one with
    DEBUG=1 bash scripts/build_old.sh gemm.hip gemm_pp.hip gemm_exp.hip ff_pass.hip gemm_tn.hip miniroad_forward.cpp miniroad_train.cpp \
        vit_host.cpp vit_stream.cpp host_misc.cpp
(those sources as of git HEAD).  The smallest shapes at which each piece can still go wrong:
  ping-pong loop     prego_debug_gemm_bf16 variant 12, M in {300, 513} (ragged rows in one tile / three tile rows), N in {256, 512},
                     K in {128, 192, 256, 320} (nk = 2 .. 5: prologue only, one steady iteration, even and odd tails), and (4113, 512, 4096)
  SPLIT              an fp16x2 forward whose layer1 contraction is K in {64, 96, 128} (the minimum and the odd counts of the 32-wide tile)
  worker             prego_debug_gemm_worker at (513, 512, 192), xcd_lo in {0, 4}, grid 256
  forced variants    0, 1, 9, 12, 30 at NT_VARIANT_SHAPES[0:2]
  dispatcher         prego_debug_gemm_nt over NT_DISPATCH, bf16 and fp16, and NT_TRAIN_SPLITK with the flag
  epilogues          one ViT forward and one ViT training step (dropout on: both masks, pre_f32) at B * T below and above 4096, so that the
                     128 x 128 and the ping-pong kernel each carry every mode: outputs, loss and every gradient
  feed-forward       one split-pass forward per operand type at (d_rgb, d_flow, emb) = (1088, 576, 512): logits and argmax
Every comparison must be equal.  One JSON line: comparisons, mismatches.  usage: python scripts/probes/gemm_ab.py [--old LIB] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np                                           # noqa: E402
import torch                                                 # noqa: E402

from prego_amd import _lib                                   # noqa: E402
from prego_amd import weights as W                           # noqa: E402
from prego_amd.config import assembly101_cfg                 # noqa: E402
from tests.helpers import gemm_exact as gx                   # noqa: E402

vp, i32 = C.c_void_p, C.c_int


def open_old(path):
    """the old debug library has the debug entries of its own commit only: the product ABI's types, then the four hooks used here"""
    lib = _lib._open(path, debug=False)
    lib.prego_debug_gemm_worker.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, vp]
    lib.prego_debug_gemm_bf16.argtypes = [i32, vp, vp, vp, vp, i32, i32, i32, vp]
    lib.prego_debug_gemm_nt.argtypes = [i32, i32, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, vp]
    return lib


class using:
    """the Python modules ask _lib.load() for the library on every call: point it at one of the two"""
    def __init__(self, lib):
        self.lib = lib

    def __enter__(self):
        self.saved = (_lib._lib, _lib._dbg)
        _lib._lib = _lib._dbg = self.lib

    def __exit__(self, *a):
        _lib._lib, _lib._dbg = self.saved


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=os.path.join(ROOT, "prego_amd", "lib_ab", "libold_debug.so"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gemm_ab: no GPU")
    libs = {"new": _lib.load_debug(), "old": open_old(args.old)}
    p = lambda t: vp(t.data_ptr()) if t is not None else None
    stream = lambda: vp(torch.cuda.current_stream().cuda_stream)
    n_cmp, bad, sizes, refused = 0, [], {}, set()

    def raw(t):
        return t.detach().reshape(-1).contiguous().view(torch.uint8).cpu().numpy().tobytes()

    def both(what, fn):
        """fn(lib) -> list of tensors (or an error text): run on both libraries, compare the bytes"""
        nonlocal n_cmp
        res = {}
        for name, lib in libs.items():
            try:
                out = fn(lib)
                torch.cuda.synchronize()
                res[name] = [raw(t) if torch.is_tensor(t) else repr(t).encode() for t in out]
            except (_lib.PregoError, ValueError, NotImplementedError) as e:      # a refusal is a result too: both must refuse in the same words
                res[name] = [("refused: " + str(e)).encode()]
                refused.add(what)
        n_cmp += 1
        sizes[what] = sum(len(b) for b in res["new"])
        if res["new"] != res["old"]:
            k = next((i for i, (a, b) in enumerate(zip(res["new"], res["old"])) if a != b), -1)
            bad.append(f"{what}: output {k} differs" + (f" ({res['new'][k][:120]!r} / {res['old'][k][:120]!r})" if k >= 0 and len(res["new"][k]) < 400 else ""))

    def operands(M, N, K, dt, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        A = (torch.rand((M, K), device="cuda", generator=g) * 2 - 1).to(dt)
        B = (torch.rand((N, K), device="cuda", generator=g) * 2 - 1).to(dt)
        return A, B, torch.randn((N,), device="cuda", generator=g)

    def variant(v, M, N, K):
        A, B, bias = operands(M, N, K, torch.bfloat16, M + N + K)

        def run(lib):
            out = torch.full((M, N), float("nan"), device="cuda")
            rc = lib.prego_debug_gemm_bf16(v, p(A), p(B), p(bias), p(out), M, N, K, stream())
            return [out, rc]
        both(f"variant {v} ({M}, {N}, {K})", run)

    # ---- the ping-pong loop
    for M in (300, 513):
        for N in (256, 512):
            for K in (128, 192, 256, 320):
                variant(12, M, N, K)
    variant(12, 4113, 512, 4096)
    # ---- the five forced variants
    for (M, N, K) in gx.NT_VARIANT_SHAPES[0:2]:
        for v in (0, 1, 9, 12, 30):
            variant(v, M, N, K)
    # ---- the dispatcher
    for f16 in (0, 1):
        for (M, N, K), sk in [(s, 0) for s in gx.NT_DISPATCH] + ([(s, 1) for s in gx.NT_TRAIN_SPLITK + [(2048, 3072, 1024)]] if not f16 else []):
            A, B, bias = operands(M, N, K, torch.float16 if f16 else torch.bfloat16, M + N + K + f16)

            def run(lib):
                out = torch.full((M, N), float("nan"), device="cuda")
                rc = lib.prego_debug_gemm_nt(f16, sk, p(A), K, p(B), K, p(bias), p(out), N, M, N, K, stream())
                return [out, rc]
            both(f"dispatcher f16 {f16} train_splitk {sk} ({M}, {N}, {K})", run)
    # ---- the worker hook
    for xcd_lo in (0, 4):
        M, N, K = 513, 512, 192
        A, B, bias = operands(M, N, K, torch.bfloat16, 99)

        def run(lib):
            out = torch.full((M, N), float("nan"), device="cuda")
            counter = torch.zeros(1, dtype=torch.int32, device="cuda")
            rc = lib.prego_debug_gemm_worker(p(A), p(B), p(bias), p(out), M, N, K, xcd_lo, p(counter), 256, stream())
            return [out, rc]
        both(f"worker xcd_lo {xcd_lo}", run)

    # ---- SPLIT: the fp16x2 forward, layer1's contraction = d_rgb; and the feed-forward kernel: a split pass per operand type
    from prego_amd.engine import MiniRoadEngine

    def miniroad_sd(din, emb, H, ncls, seed):
        rng = np.random.default_rng(seed)
        u = lambda shape, b: rng.uniform(-b, b, shape).astype(np.float32)
        return {"gru.weight_ih_l0": u((3 * H, emb), 1 / 32), "gru.weight_hh_l0": u((3 * H, H), 1 / 32), "gru.bias_ih_l0": u((3 * H,), 1 / 32),
                "gru.bias_hh_l0": u((3 * H,), 1 / 32), "layer1.0.weight": u((emb, din), din ** -0.5), "layer1.0.bias": u((emb,), din ** -0.5),
                "layer1.1.weight": (1.0 + u((emb,), 0.25)), "layer1.1.bias": u((emb,), 0.1),
                "f_classification.0.weight": 8.0 * u((ncls, H), 1 / 32), "f_classification.0.bias": u((ncls,), 1 / 32)}

    def feat(shape, seed):
        g = torch.Generator(device="cuda").manual_seed(seed)
        return torch.randn(shape, device="cuda", generator=g).clamp_(min=0)

    for K in (64, 96, 128):
        sd = miniroad_sd(K, 512, 1024, 12, K)
        rgb = [feat((T, K), 40 + i) for i, T in enumerate((300, 213))]

        def run(lib):
            e = MiniRoadEngine(K, 0, 512, 1024, 12, "cuda:0", "fp16x2", lib=lib)
            e.set_weights({k: torch.from_numpy(v).cuda() for k, v in sd.items()})
            o, a, _ = e.forward_ragged(rgb, None, softmax=False, want_out=True, want_argmax=True)
            e.check()
            return list(o) + list(a)
        both(f"fp16x2 forward, layer1 K = {K}", run)

    d_rgb, d_flow, emb = 1088, 576, 512
    sd = miniroad_sd(d_rgb + d_flow, emb, 1024, 12, 5)
    g = torch.Generator().manual_seed(31)
    lens = [int(x) for x in torch.randint(5100, 5601, (52,), generator=g)]
    rgb = [feat((T, d_rgb), 3100 + i) for i, T in enumerate(lens)]
    flow = [feat((T, d_flow), 3900 + i) for i, T in enumerate(lens)]
    for dtype in ("fp16", "bf16"):
        def run(lib):
            os.environ["PREGO_SPLIT_PASS"] = "3"
            try:
                e = MiniRoadEngine(d_rgb, d_flow, emb, 1024, 12, "cuda:0", dtype, lib=lib)
            finally:
                os.environ.pop("PREGO_SPLIT_PASS", None)
            e.set_weights({k: torch.from_numpy(v).cuda() for k, v in sd.items()})
            for _ in range(2):                                # the first call of a handle establishes the placement: chunked
                o, a, _ = e.forward_ragged(rgb, flow, softmax=False, want_out=True, want_argmax=True)
                e.check()
            return list(o) + list(a) + [e.pass_info()["mode"]]
        both(f"split pass {dtype} {(d_rgb, d_flow, emb)}", run)
    del rgb, flow

    # ---- the epilogues: ViT forward and training step, B * T below and above 4096
    from prego_amd.registry import build_criterion, build_model
    import prego_amd.loss, prego_amd.transformer             # noqa: E401,F401
    for dtype in ("bf16", "fp16"):
        cfg = assembly101_cfg(model="Transformer", window_size=128, patch_dim=1, num_heads=8, attn_dropout_rate=0.15, dropout=0.1, compute_dtype=dtype,
                              num_layers=1)
        sd = W.vit_state_dict(cfg, 20)
        for B in (2, 33):                                     # B * T = 256 / 4224 encoder rows, B * (T + 1) = 258 / 4257 token rows
            rgb = torch.from_numpy(W.tsn_features((B, 128, 2048), 21, "ab.rgb")).cuda()
            flow = torch.from_numpy(W.tsn_features((B, 128, 2048), 21, "ab.flow")).cuda()
            cls = (W.uniform01((B, 128), 21, "ab.tgt") * 86).astype(np.int64)
            tgt = torch.nn.functional.one_hot(torch.from_numpy(cls), 86).float().cuda()

            def run(lib, train):
                with using(lib):
                    model = build_model(cfg, "cuda:0")
                    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
                    if not train:
                        model.eval()
                        with torch.no_grad():
                            return [model(rgb, flow)["logits"]]
                    model.debug_dropout_seed = 123456789
                    crit = build_criterion(cfg, "cuda:0")
                    model.train()
                    out = model(rgb, flow)
                    loss = crit(out, tgt)
                    loss.backward()
                    torch.cuda.synchronize()
                    return [out["logits"], loss] + [pr.grad for _, pr in model.named_parameters()]
            both(f"ViT {dtype} forward B {B}", lambda lib: run(lib, False))
            both(f"ViT {dtype} training step B {B}", lambda lib: run(lib, True))

    line = json.dumps({"probe": "gemm_ab", "old": os.path.relpath(args.old, ROOT), "comparisons": n_cmp, "mismatches": len(bad),
                       "bytes_compared": sum(sizes.values()), "refused_by_both_or_one": sorted(refused), "first_mismatches": bad[:10]})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
