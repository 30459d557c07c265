"""Calibrated AP on the device beside AP, and beside the host path it replaces, on the bench eval-set shape (2 306 143 frames x 86
classes, softmax of random logits so that saturated ties occur, one class id per frame in runs).  Per entry: `--steps` calls in
alternating rounds, a device-event pair per call (median, p10-p90).  The host path = the device -> host copy of the score and target
matrices (host clock around a copy that ends in a synchronise) + calibrated_average_precision_columns (host clock), once.  A slice is
checked against the host functions.  One JSON line.  usage: python scripts/probes/cap_time.py [--frames N] [--steps 10] [--rounds 3]
[--no-host] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np                                           # noqa: E402
import torch                                                 # noqa: E402

from prego_amd import _lib                                   # noqa: E402
from prego_amd._lib import check                             # noqa: E402
from prego_amd.metrics import calibrated_average_precision_columns, perstage_ap_raw       # noqa: E402

N_CLASSES = 86


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2_306_143)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--check-frames", type=int, default=20_000)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cap_time: no GPU (a device time cannot be measured without one)")
    lib = _lib.load()
    n = args.frames
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    scores = torch.softmax(torch.randn(n, N_CLASSES, device="cuda", generator=g) * 30, -1)     # many exact 0.0 and 1.0
    runs = torch.randint(24, 625, (n // 24 + 1,), device="cuda", generator=g)
    ids = torch.randint(0, N_CLASSES, (runs.numel(),), device="cuda", generator=g)
    labels = torch.repeat_interleave(ids, runs)[:n].to(torch.int32).contiguous()
    saturated = float(((scores == 0) | (scores == 1)).float().mean())
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out_f = torch.empty((3, N_CLASSES), dtype=torch.float64, device="cuda")
    out_s = torch.empty((2, 10, N_CLASSES), dtype=torch.float64, device="cuda")

    def frame_entry(fn, need):
        ws = torch.empty(need(n, N_CLASSES), dtype=torch.uint8, device="cuda")
        return lambda: check(fn(p(scores), p(labels), n, N_CLASSES, p(out_f[0]), p(out_f[1]), p(out_f[2]), p(ws), ws.numel(), s))

    def stage_entry(fn, need):
        ws = torch.empty(need(n, N_CLASSES), dtype=torch.uint8, device="cuda")
        return lambda: check(fn(p(scores), p(labels), n, N_CLASSES, p(out_s[0]), p(out_s[1]), p(ws), ws.numel(), s))

    entries = {"perframe_cap_ms": frame_entry(lib.prego_perframe_cap_labels, lib.prego_perframe_cap_workspace_bytes),
               "perframe_ap_ms": frame_entry(lib.prego_perframe_ap_labels, lib.prego_perframe_ap_workspace_bytes),
               "perstage_cap_ms": stage_entry(lib.prego_perstage_cap_labels, lib.prego_perstage_cap_workspace_bytes),
               "perstage_ap_ms": stage_entry(lib.prego_perstage_ap_labels, lib.prego_perstage_ap_workspace_bytes)}
    times = {k: [] for k in entries}
    for fn in entries.values():                               # warm-up: every kernel of every entry has run twice
        fn(); fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in entries.items():
            for _ in range(args.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
    res = {"frames": n, "classes": N_CLASSES, "saturated_share": saturated, "calls_per_entry": args.rounds * args.steps}
    for name, t in times.items():
        res[name] = {"median": float(np.median(t)), "p10": float(np.percentile(t, 10)), "p90": float(np.percentile(t, 90))}
    if not args.no_host:
        target = torch.zeros(n, N_CLASSES, device="cuda")
        target[torch.arange(n, device="cuda"), labels.long()] = 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc_h, tg_h = scores.cpu().numpy(), target.cpu().numpy()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        host = calibrated_average_precision_columns(sc_h, tg_h != 0)
        t2 = time.perf_counter()
        entries["perframe_cap_ms"]()
        dev = out_f[0].cpu().numpy()
        res["host_path_ms"] = {"d2h_copy": (t1 - t0) * 1e3, "calibrated_average_precision_columns": (t2 - t1) * 1e3}
        res["full_set_max_abs_diff_vs_host"] = float(np.nanmax(np.abs(dev - host)))
    m = min(n, args.check_frames)
    sub = scores[:m].contiguous()
    ws = torch.empty(lib.prego_perstage_cap_workspace_bytes(m, N_CLASSES), dtype=torch.uint8, device="cuda")
    check(lib.prego_perstage_cap_labels(p(sub), p(labels), m, N_CLASSES, p(out_s[0]), p(out_s[1]), p(ws), ws.numel(), s))
    want, want_pos = perstage_ap_raw(sub.cpu().numpy(), labels[:m].cpu().numpy(), "cAP")
    got = out_s[0].cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(out_s[1].cpu().numpy().view(np.int64), want_pos)
    res["slice_perstage_max_abs_diff_vs_host"] = float(np.nanmax(np.abs(got - want)))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
