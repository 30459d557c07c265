#!/usr/bin/env python3
"""Per-stage AP on the device (prego_perstage_ap_labels) beside the per-frame AP (prego_perframe_ap_labels) on the same inputs in one
process: the bench eval set's shape (workloads.assembly101_eval_lengths: 182 videos, 2.3 M frames, 86 classes), softmax-like scores
that favour the labelled class, class ids in runs of realistic length (workloads.action_labels per video: 24 .. 624 frames, a quarter
background).  Prints one JSON line: the median device time of each entry (a device-event pair per call, alternating rounds after
warm-up), their ratio, the p10 / p90 of each, the workspace sizes, and the largest difference to the host form on a slice.

    python scripts/perstage_ap_bench.py [--steps 10] [--warmup 2] [--rounds 3] [--clips 0] [--check-frames 20000] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prego_amd import _lib, workloads                       # noqa: E402
from prego_amd._lib import check                            # noqa: E402
from prego_amd.metrics import perstage_ap_raw               # noqa: E402

N_CLASSES = 86


def inputs(clips: int, seed: int = 20):
    lens = workloads.assembly101_eval_lengths()
    if clips:
        lens = lens[:clips]
    labels = np.concatenate([workloads.action_labels(T, N_CLASSES, seed, f"perstage.bench.{i}") for i, T in enumerate(lens)]).astype(np.int32)
    n = labels.shape[0]
    g = torch.Generator(device="cuda").manual_seed(seed)
    logits = torch.randn((n, N_CLASSES), generator=g, device="cuda")
    lab = torch.from_numpy(labels).cuda()
    logits[torch.arange(n, device="cuda"), lab.long()] += 2.0          # right more often than not
    return torch.softmax(logits, 1).contiguous(), lab, len(lens)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10, help="timed calls per entry and round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--clips", type=int, default=0, help="first N videos of the eval set (0 = all)")
    ap.add_argument("--check-frames", type=int, default=20000, help="frames of the slice compared with the host form (0 = no check)")
    ap.add_argument("--out", default=None, help="write the JSON line there as well")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("perstage_ap_bench: no GPU (a device time cannot be measured without one)")
    lib = _lib.load()
    scores, labels, n_videos = inputs(a.clips)
    n = int(scores.shape[0])
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    ws_stage = torch.empty(lib.prego_perstage_ap_workspace_bytes(n, N_CLASSES), dtype=torch.uint8, device="cuda")
    ws_frame = torch.empty(lib.prego_perframe_ap_workspace_bytes(n, N_CLASSES), dtype=torch.uint8, device="cuda")
    out_stage = torch.empty((2, 10, N_CLASSES), dtype=torch.float64, device="cuda")
    out_frame = torch.empty((3, N_CLASSES), dtype=torch.float64, device="cuda")

    def stage():
        check(lib.prego_perstage_ap_labels(p(scores), p(labels), n, N_CLASSES, p(out_stage[0]), p(out_stage[1]), p(ws_stage), ws_stage.numel(), s))

    def frame():
        check(lib.prego_perframe_ap_labels(p(scores), p(labels), n, N_CLASSES, p(out_frame[0]), p(out_frame[1]), p(out_frame[2]), p(ws_frame),
                                           ws_frame.numel(), s))
    for _ in range(a.warmup):
        stage()
        frame()
    torch.cuda.synchronize()
    first = out_stage.clone()
    times = {"perstage": [], "perframe": []}
    for _ in range(a.rounds):                                # alternating rounds: both entries see the same machine
        for name, fn in (("perstage", stage), ("perframe", frame)):
            evs = []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                evs.append((e0, e1))
            torch.cuda.synchronize()
            times[name] += [e0.elapsed_time(e1) for e0, e1 in evs]
    res = {"n_frames": n, "n_classes": N_CLASSES, "n_videos": n_videos, "calls_per_entry": a.rounds * a.steps,
           "same_bits_every_call": bool(torch.equal(first.view(torch.int64), out_stage.view(torch.int64))),
           "workspace_bytes": {"perstage": ws_stage.numel(), "perframe": ws_frame.numel()}}
    for name, t in times.items():
        t = np.array(t)
        res[name + "_ms"] = {"median": round(float(np.median(t)), 4), "p10": round(float(np.percentile(t, 10)), 4),
                             "p90": round(float(np.percentile(t, 90)), 4)}
    res["ratio_perstage_over_perframe"] = round(res["perstage_ms"]["median"] / res["perframe_ms"]["median"], 3)
    stage_ap = out_stage[0].cpu().numpy()
    res["mean_ap_by_stage"] = [round(float(x), 4) for x in stage_ap[:, 1:].mean(1)]
    if a.check_frames:
        m = min(n, a.check_frames)
        ws = torch.empty(lib.prego_perstage_ap_workspace_bytes(m, N_CLASSES), dtype=torch.uint8, device="cuda")
        sub = scores[:m].contiguous()
        check(lib.prego_perstage_ap_labels(p(sub), p(labels), m, N_CLASSES, p(out_stage[0]), p(out_stage[1]), p(ws), ws.numel(), s))
        torch.cuda.synchronize()
        host_ap, host_pos = perstage_ap_raw(sub.cpu().numpy(), labels[:m].cpu().numpy())
        res["check"] = {"frames": m, "max_abs_diff_to_host": float(np.abs(out_stage[0].cpu().numpy() - host_ap).max()),
                        "positives_equal": bool(np.array_equal(out_stage[1].cpu().numpy().view(np.int64), host_pos))}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
