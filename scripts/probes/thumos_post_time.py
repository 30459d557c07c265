"""The THUMOS post-processing on the device (prego_thumos_postprocess, csrc/thumos_post.hip) alone, beside two yardsticks from outside
the code under test, at the bench eval-set frame count (2 306 143) x 86 and x 22 classes, dense fp32 targets whose column 21 is 1 on
about 5 % of the rows, for flags off and for smooth + switch:

  * clone       a device clone() of the same score and target matrices: the bandwidth floor for reading and writing those bytes once
  * host route  what the device path replaces: D2H copy of both matrices, the numpy form (prego_amd.postprocessing), H2D copy of its
                results (host clocks around steps that end in a synchronise), once per case

Device entries: `--steps` calls per round in alternating rounds, a device-event pair per call (median, p10-p90), after two warm-up calls
of every entry; one process.  A slice of every case is checked against the host form, bit for bit.  One JSON line.
usage: python scripts/probes/thumos_post_time.py [--frames N] [--steps 10] [--rounds 2] [--no-host] [--out FILE]"""
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
from prego_amd.postprocessing import ThumosPostprocessing    # noqa: E402

AMB = 21


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2_306_143)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--check-frames", type=int, default=20_000)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("thumos_post_time: no GPU (a device time cannot be measured without one)")
    lib = _lib.load()
    n = args.frames
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {"frames": n, "calls_per_entry": args.rounds * args.steps, "cases": {}}
    for ncls in (86, 22):
        g = torch.Generator(device="cuda")
        g.manual_seed(ncls)
        scores = torch.rand(n, ncls, device="cuda", generator=g)
        ids = torch.randint(0, AMB, (n,), device="cuda", generator=g)
        runs = torch.repeat_interleave(torch.rand(n // 20 + 1, device="cuda", generator=g) < 0.05, 20)[:n]      # ambiguous in runs of 20
        ids[runs] = AMB
        target = torch.zeros(n, ncls, device="cuda")
        target[torch.arange(n, device="cuda"), ids] = 1
        out_s, out_t = torch.empty_like(scores), torch.empty_like(target)
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        ws = torch.empty(lib.prego_thumos_postprocess_workspace_bytes(n, ncls), dtype=torch.uint8, device="cuda")

        def entry(flags):
            return lambda: check(lib.prego_thumos_postprocess(p(scores), ncls, p(target), ncls, n, ncls, flags, 5, 8, AMB, p(out_s), p(out_t),
                                                              p(cnt), p(ws), ws.numel(), s))

        def clone():
            scores.clone(); target.clone()
        entries = {"flags_off_ms": entry(0), "smooth_switch_ms": entry(3), "clone_ms": clone}
        times = {k: [] for k in entries}
        for fn in entries.values():                           # warm-up: every kernel of every entry has run twice
            fn(); fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name, fn in entries.items():
                for _ in range(args.steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(); fn(); e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1))
        kept = int(cnt.item())
        case = {"classes": ncls, "kept_rows": kept, "bytes_read": 2 * n * ncls * 4, "bytes_written": 2 * kept * ncls * 4}
        for name, t in times.items():
            case[name] = {"median": float(np.median(t)), "p10": float(np.percentile(t, 10)), "p90": float(np.percentile(t, 90))}
        for name in ("flags_off_ms", "smooth_switch_ms"):
            case[name]["ratio_to_clone"] = case[name]["median"] / case["clone_ms"]["median"]
        if not args.no_host:
            post = ThumosPostprocessing(True, True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sc_h, tg_h = scores.cpu().numpy(), target.cpu().numpy()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            gt_h, pr_h = post(tg_h, sc_h)
            t2 = time.perf_counter()
            back = torch.from_numpy(pr_h).cuda(), torch.from_numpy(gt_h).cuda()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            case["host_route_smooth_switch_ms"] = {"d2h_copy": (t1 - t0) * 1e3, "numpy": (t2 - t1) * 1e3, "h2d_copy": (t3 - t2) * 1e3,
                                                   "total": (t3 - t0) * 1e3}
            entries["smooth_switch_ms"]()
            torch.cuda.synchronize()
            case["full_set_equals_host_form"] = bool(torch.equal(out_s[:kept], back[0]) and torch.equal(out_t[:kept], back[1]))
            del back, sc_h, tg_h, gt_h, pr_h
        m = min(n, args.check_frames)
        for flags in (0, 3):                                  # a slice against the host form, bit for bit
            check(lib.prego_thumos_postprocess(p(scores), ncls, p(target), ncls, m, ncls, flags, 5, 8, AMB, p(out_s), p(out_t), p(cnt), p(ws),
                                               ws.numel(), s))
            k = int(cnt.item())
            gt_h, pr_h = ThumosPostprocessing(bool(flags & 1), bool(flags & 2))(target[:m].cpu().numpy(), scores[:m].cpu().numpy())
            assert k == gt_h.shape[0] and np.array_equal(out_s[:k].cpu().numpy(), pr_h) and np.array_equal(out_t[:k].cpu().numpy(), gt_h)
        case["slice_equals_host_form"] = True
        res["cases"][str(ncls)] = case
        del scores, target, out_s, out_t
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
