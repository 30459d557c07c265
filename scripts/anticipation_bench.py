#!/usr/bin/env python3
"""MiniROADA inference on the bench workload (workloads.assembly101_eval_lengths, anticipation_length 8): prints one JSON line with
MROADA and MROAD frames/s, the anticipation head's own time (MROADA pass - MROAD pass on the same handle), its TFLOP/s and share of the
2.5 PFLOP/s dense bf16 spec, and which pass ran.

    python scripts/anticipation_bench.py [--dtype bf16] [--steps 3] [--warmup 1] [--clips N]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prego_amd import weights as W                          # noqa: E402
from prego_amd import workloads                             # noqa: E402
from prego_amd.config import anticipation_cfg, assembly101_cfg  # noqa: E402
from prego_amd.registry import build_model                  # noqa: E402
import prego_amd.model  # noqa: F401,E402

SPEC = 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--clips", type=int, default=0, help="first N clips of the workload (0 = all)")
    ap.add_argument("--L", type=int, default=8)
    a = ap.parse_args()
    dev = "cuda:0"
    lens = workloads.assembly101_eval_lengths()
    if a.clips:
        lens = lens[:a.clips]
    frames = int(sum(lens))
    cfg = anticipation_cfg(assembly101_cfg(compute_dtype=a.dtype), a.L)
    sd = W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0)
    m = build_model(cfg, dev)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m.eval()
    eng = m.engine()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    rgb = [torch.randn((T, 2048), device=dev, generator=gen).clamp_(min=0) for T in lens]
    flow = [torch.randn((T, 2048), device=dev, generator=gen).clamp_(min=0) for T in lens]

    def timed(want_ant):
        for _ in range(a.warmup):
            eng.forward_ragged(rgb, flow, softmax=True, want_argmax=True, want_ant=want_ant)
        eng.check()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            r = eng.forward_ragged(rgb, flow, softmax=True, want_argmax=True, want_ant=want_ant)
            del r
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / a.steps
        eng.check()
        return dt, eng.pass_info()

    dt_a, info_a = timed(True)
    dt_0, info_0 = timed(False)
    H, C, L = cfg["hidden_dim"], cfg["num_classes"], a.L
    flop = frames * (2.0 * H * L * H + 2.0 * L * H * C)
    head = max(dt_a - dt_0, 1e-9)
    print(json.dumps({
        "metric": "MiniROADA inference frames/s (anticipation head fused, csrc/ant_head.hip)", "dtype": a.dtype, "frames": frames,
        "clips": len(lens), "anticipation_length": L,
        "mroada_frames_per_s": frames / dt_a, "mroad_frames_per_s": frames / dt_0,
        "mroada_ms": dt_a * 1e3, "mroad_ms": dt_0 * 1e3, "head_ms": head * 1e3, "head_tflop": flop / 1e12,
        "head_tflops": flop / head / 1e12, "head_share_of_spec": flop / head / SPEC,
        "pass_mroada": info_a, "pass_mroad": info_0}))


if __name__ == "__main__":
    main()
