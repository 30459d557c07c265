"""Speed A/B of the NT GEMM kernels against the parent's library (prego_amd/lib_ab/libold_debug.so, scripts/probes/gemm_ab.py says how it is
built), both opened in one process.  Per shape and round three slots run back to back - parent, new, parent again - each `--iters` launches
between two events; the parent-against-parent ratio of the same rounds is the bar the new-against-parent ratio is read against.
  ping-pong            the bench workload's projections (49152 rows: layer1 N 2048 K 4096, W_ih N 3072 K 2048), bf16 and fp16, via the dispatcher
  128 x 128, 256 x 128, ping-pong   one Transformer-sized shape each, forced through prego_debug_gemm_bf16
  worker               one launch of prego_debug_gemm_worker per iteration
  host                 wall time per call of the dispatcher at a small shape (launch_gemm_bf16_nt's chooser runs once per launch)
One JSON document.  usage: python scripts/probes/gemm_speed_ab.py [--old LIB] [--rounds 7] [--iters 20] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch                                                 # noqa: E402

from prego_amd import _lib                                   # noqa: E402
from gemm_ab import open_old                                 # noqa: E402

vp = C.c_void_p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=os.path.join(ROOT, "prego_amd", "lib_ab", "libold_debug.so"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    new, old = _lib.load_debug(), open_old(args.old)
    slots = [("parent_a", old), ("new", new), ("parent_b", old)]
    p = lambda t: vp(t.data_ptr())
    s = lambda: vp(torch.cuda.current_stream().cuda_stream)

    def operands(M, N, K, dt):
        g = torch.Generator(device="cuda").manual_seed(M + N + K)
        A = (torch.rand((M, K), device="cuda", generator=g) * 2 - 1).to(dt)
        B = (torch.rand((N, K), device="cuda", generator=g) * 2 - 1).to(dt)
        return A, B, torch.randn((N,), device="cuda", generator=g), torch.empty((M, N), device="cuda")

    def dispatcher(M, N, K, f16):
        A, B, bias, out = operands(M, N, K, torch.float16 if f16 else torch.bfloat16)
        return lambda lib: lib.prego_debug_gemm_nt(f16, 0, p(A), K, p(B), K, p(bias), p(out), N, M, N, K, s())

    def forced(v, M, N, K):
        A, B, bias, out = operands(M, N, K, torch.bfloat16)
        return lambda lib: lib.prego_debug_gemm_bf16(v, p(A), p(B), p(bias), p(out), M, N, K, s())

    def worker(M, N, K):
        A, B, bias, out = operands(M, N, K, torch.bfloat16)
        counter = torch.zeros(1, dtype=torch.int32, device="cuda")

        def run(lib):
            counter.zero_()
            return lib.prego_debug_gemm_worker(p(A), p(B), p(bias), p(out), M, N, K, 0, p(counter), 256, s())
        return run

    cases = [("pingpong layer1 bf16 (49152, 2048, 4096)", dispatcher(49152, 2048, 4096, 0)), ("pingpong layer1 fp16 (49152, 2048, 4096)", dispatcher(49152, 2048, 4096, 1)),
             ("pingpong w_ih bf16 (49152, 3072, 2048)", dispatcher(49152, 3072, 2048, 0)), ("pingpong w_ih fp16 (49152, 3072, 2048)", dispatcher(49152, 3072, 2048, 1)),
             ("pingpong forced (4224, 2048, 2048)", forced(12, 4224, 2048, 2048)), ("128x128 forced (1032, 2048, 2048)", forced(0, 1032, 2048, 2048)),
             ("256x128 forced (2064, 2048, 2048)", forced(1, 2064, 2048, 2048)), ("worker (49152, 2048, 4096)", worker(49152, 2048, 4096))]
    doc = {"probe": "gemm_speed_ab", "old": os.path.relpath(args.old, ROOT), "rounds": args.rounds, "iters": args.iters, "unit": "us per launch", "rows": {}}
    for name, call in cases:
        for _, lib in slots:                                   # warm-up: attributes set, clocks up
            for _ in range(3):
                assert call(lib) == 0
        torch.cuda.synchronize()
        t = {k: [] for k, _ in slots}
        for _ in range(args.rounds):
            for k, lib in slots:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    call(lib)
                e1.record()
                e1.synchronize()
                t[k].append(e0.elapsed_time(e1) * 1e3 / args.iters)
        pp = [b / a for a, b in zip(t["parent_a"], t["parent_b"])]
        np_ = [n / ((a + b) / 2) for a, n, b in zip(t["parent_a"], t["new"], t["parent_b"])]
        widest = max(max(pp), 1 / min(pp))
        doc["rows"][name] = {"median_us": {k: round(statistics.median(v), 3) for k, v in t.items()},
                             "parent_b_over_parent_a": {"min": round(min(pp), 4), "max": round(max(pp), 4), "widest": round(widest, 4)},
                             "new_over_parent": {"min": round(min(np_), 4), "median": round(statistics.median(np_), 4), "max": round(max(np_), 4)},
                             "median_within_parent_spread": statistics.median(np_) <= widest}
    # host time per call: a small shape, the stream drained first, wall clock over many calls (the launches queue up; the device is not waited for)
    call = dispatcher(128, 128, 64, 0)
    host = {k: [] for k, _ in slots}
    for _ in range(args.rounds):
        for k, lib in slots:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(200):
                call(lib)
            host[k].append((time.perf_counter() - t0) / 200 * 1e6)
            torch.cuda.synchronize()
    doc["host_us_per_call_dispatcher_128x128x64"] = {k: round(statistics.median(v), 3) for k, v in host.items()}
    line = json.dumps(doc, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
