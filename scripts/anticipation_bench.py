#!/usr/bin/env python3
"""MiniROADA inference on the bench workload (workloads.assembly101_eval_lengths, anticipation_length 8): prints one JSON line with
MROADA and MROAD frames/s, the anticipation head's own time (MROADA pass - MROAD pass on the same handle), its TFLOP/s and share of the
2.5 PFLOP/s dense bf16 spec, and which pass ran.

    python scripts/anticipation_bench.py [--dtype bf16] [--steps 3] [--warmup 1] [--clips N]

--train: the training step instead (B 16, T 128, zero flow, FusedAdamW, the guarded loop's body: forward, OadAntLoss, backward, step) for
MiniROADA at L = 1 / 4 / 8 and MiniROAD's step in the same process, in alternating rounds; median step time from device events after
warm-up.  With PREGO_AMD_DEBUG_LIB=1 MiniROADA also runs with the head's backward forced over every packed row (prego_debug_ant_full_span)
for the span / full-range A/B.

    PREGO_AMD_DEBUG_LIB=1 python scripts/anticipation_bench.py --train [--steps 200] [--warmup 20] [--rounds 4]

--step: the online use, one frame per call for n = 1 / 4 / 16 streams at L = 1 / 4 / 8 (zero flow): (a) MROAD.step, (b) MROADA.step
(csrc/stream_ant.hip behind the streaming step), (c) the general forward at T = 1 with h0 / h_last and the anticipation head - what
MiniROADA streaming cost before (b) existed.  The --train protocol: warm-up, alternating rounds, a device-event pair around every frame,
median over all rounds (at least 200 frames per path and round); `round_us` is the whole round between two events divided by its frames
(what a caller that issues frames back to back sees, host issue rate included).

    python scripts/anticipation_bench.py --step [--steps 200] [--warmup 20] [--rounds 4]

--step --wide: more than 16 streams per frame time, n = 17 / 32 / 64 / 128 / 256 for MiniROAD and MiniROADA at L = 1 / 8 (zero flow), the
same protocol: (w) step_wide (csrc/stream_wide.hip), (g) ceil(n / 16) `step` calls over 16-row views of the same tensors on one stream -
what a caller had before (w) existed - and (c) the general forward at T = 1.  --models / --streams / --paths narrow the run.

    python scripts/anticipation_bench.py --step --wide [--steps 200] [--warmup 20] [--rounds 4] [--streams 17,256] [--models L0,L8] [--paths w,g]

--step --pool: the stream pool (prego_amd/stream_pool.py), n_active = 4 / 16 / 64 / 256 scattered slots of a 256-slot pool for MiniROAD and
MiniROADA at L = 8 (zero flow), the same protocol: (p) StreamPool.push, (w) the dense step_wide on the same streams - the lower bound, the
pool can only add to it - and (t) the route a caller has without the pool: index_select the active states out of a table, step_wide,
index_copy_ them back, argmax.cpu(), the window vote on the host.  `p_minus_w_us` stands beside two kernel boundaries.

    python scripts/anticipation_bench.py --step --pool [--steps 200] [--warmup 20] [--rounds 4] [--streams 4,256] [--models L0,L8]

--step --pool --frames: bursts (StreamPool.push_frames, csrc/stream_frames.hip), K = 2 / 4 / 8 / 16 frames for n_active = 1 / 4 / 16 slots
and K = 2 / 4 for n_active = 64, MiniROAD and MiniROADA at L = 8 (zero flow), the same protocol with a device-event pair around every
call: (f) ONE push_frames of K frames, (k) K successive push calls on the same slots - what a caller had before (f) existed.  Per cell:
both per call and per frame (/ K), and whether (f) lies below (k) by more than the p10..p90 widths of both.  `marginal_us_per_frame` is
the slope of (f) between the two largest K of an n_active: what one more frame per stream costs - the fused recurrent launch plus the frame's
share of the row-wise products.

    python scripts/anticipation_bench.py --step --pool --frames [--steps 200] [--warmup 20] [--rounds 4] [--models L0,L8]

--step --pool --ragged: ragged bursts (StreamPool.push_ragged, csrc/stream_frames.hip: frames_recur_ragged), 16 and 64 scattered slots,
the same protocol: (r) ONE push_ragged, (g) the route a caller had before it - one push_frames per group of equal count on the same
slots.  Workloads: counts uniform in 1..8 (seeded, about eight groups, at most 256 rows), one straggler with 32 frames beside streams with
one, and the control - all counts 4, where (g) is a single push_frames and (r) has nothing to gain: `r_within_control` says whether
|r - g| stays within the larger of the two p10..p90 widths.

    python scripts/anticipation_bench.py --step --pool --ragged [--steps 200] [--warmup 20] [--rounds 4] [--models L0,L8]

--step --pool --feed: the event feed (EventFeed, csrc/stream_feed.hip), n_active = 4 / 16 / 64 / 256 scattered slots of a 256-slot pool with
1 024 events per record and a vote window of --vote-window frames (1: every frame votes, so events occur on most ticks), the same protocol: (a) push + drain + reading
the ticket of the tick before, (b) the route a caller had before the feed - push, then events(slot) for every active slot, one blocking
record copy each - and (c) push alone.  `a_minus_c_us` / `b_minus_c_us`: what learning of the new events adds to a tick.  Every record is
emptied (outside the timed part) before a leg's round, so no record fills.

    python scripts/anticipation_bench.py --step --pool --feed [--steps 200] [--warmup 20] [--rounds 4] [--streams 4,256] [--models L0,L8]

--step --pool --snapshot: slot images (StreamPool.snapshot / restore, csrc/stream_image.hip), n = 4 / 16 / 64 / 256 scattered slots of a
256-slot pool that hold streams of 50 frames, the same protocol with a device-event pair per CALL: (s) snapshot of the n slots, (r) restore
of them into a second pool (the method, status copy included), (rc) the C restore alone, (t) the read route there was before - state(slot)
plus the record copy, per slot.  `floor_us`: the image bytes read and written once at the achievable HBM rate (scripts/pool_snapshot_legs.py).

    python scripts/anticipation_bench.py --step --pool --snapshot [--steps 100] [--warmup 20] [--rounds 4] [--streams 4,16,64,256]
                                         [--out profiles/stream_pool/snapshot_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
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
    ap.add_argument("--warmup", type=int, default=None, help="default: 1 inference pass, 20 training steps per configuration (--train)")
    ap.add_argument("--clips", type=int, default=0, help="first N clips of the workload (0 = all)")
    ap.add_argument("--L", type=int, default=8)
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--wide", action="store_true", help="with --step: step_wide against the loop of 16-stream steps")
    ap.add_argument("--pool", action="store_true", help="with --step: StreamPool.push against the dense step_wide and the torch route around it")
    ap.add_argument("--frames", action="store_true", help="with --step --pool: one push_frames of K frames against K push calls")
    ap.add_argument("--ragged", action="store_true", help="with --step --pool: one push_ragged against one push_frames per group of equal count")
    ap.add_argument("--feed", action="store_true", help="with --step --pool: push + EventFeed.drain against push + events(slot) per active slot")
    ap.add_argument("--snapshot", action="store_true", help="with --step --pool: snapshot / restore of n slots against state(slot) + record copy per slot")
    ap.add_argument("--out", default=None, help="with --snapshot: where the JSON line goes as well (default profiles/stream_pool/snapshot_bench.json)")
    ap.add_argument("--vote-window", type=int, default=1, help="with --feed: the pool's vote window, small so that events occur on most ticks")
    ap.add_argument("--streams", default=None, help="default: 17,32,64,128,256 (--wide), 4,16,64,256 (--pool)")
    ap.add_argument("--models", default=None, help="L0 = MiniROAD, Lk = MiniROADA with anticipation_length k; default: L0,L1,L8 (--wide), L0,L8 (--pool)")
    ap.add_argument("--paths", default="w,g,c")
    a = ap.parse_args()
    if a.warmup is None:
        a.warmup = 20 if (a.train or a.step) else 1
    if a.train:
        return train_bench(a)
    a.streams = a.streams or ("4,16,64,256" if a.pool else "17,32,64,128,256")
    a.models = a.models or ("L0,L8" if a.pool else "L0,L1,L8")
    if a.step:
        if a.pool and a.frames:
            return step_pool_frames_bench(a)
        if a.pool and a.ragged:
            return step_pool_ragged_bench(a)
        if a.pool and a.feed:
            return step_pool_feed_bench(a)
        if a.pool and a.snapshot:
            return step_pool_snapshot_bench(a)
        return step_pool_bench(a) if a.pool else step_wide_bench(a) if a.wide else step_bench(a)
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


def train_bench(a):
    from prego_amd import _lib
    from prego_amd.loss import OadAntLoss, OadLoss
    from prego_amd.optim import FusedAdamW
    dev, B, T = "cuda:0", 16, 128
    steps = max(a.steps, 200)
    dbg = _lib.load() if _lib.LIB_PATH == _lib.DEBUG_LIB_PATH else None
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    rgb = torch.randn((B, T, 2048), device=dev, generator=gen).clamp_(min=0)
    flow = torch.zeros_like(rgb)
    tgt = torch.nn.functional.one_hot(torch.randint(0, 86, (B, T), device=dev, generator=gen), 86).float()
    runs = {}
    base = assembly101_cfg(compute_dtype=a.dtype, assume_zero_flow=True)
    m0 = build_model(base, dev)
    m0.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_state_dict(base, 20).items()})
    runs["miniroad"] = (m0, FusedAdamW(m0.parameters(), lr=1e-4, weight_decay=0.05, model=m0), OadLoss(base), (tgt,), False)
    for L in (1, 4, 8):
        cfg = anticipation_cfg(base, L)
        m = build_model(cfg, dev)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_a_state_dict(cfg, 20).items()})
        ant = torch.nn.functional.one_hot(torch.randint(0, 86, (B, L), device=dev, generator=gen), 86).float()
        runs[f"mroada_L{L}"] = (m, FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.05, model=m), OadAntLoss(cfg), (tgt, ant), False)
        if dbg is not None:
            runs[f"mroada_L{L}_full"] = runs[f"mroada_L{L}"][:4] + (True,)
    times = {k: [] for k in runs}

    def step(m, opt, crit, targets):
        m.train()
        out = m(rgb, flow)
        loss = crit(out, *targets)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    for k, (m, opt, crit, targets, full) in runs.items():       # warm-up: workspaces, kernels, optimizer state
        for _ in range(a.warmup):
            step(m, opt, crit, targets)
    torch.cuda.synchronize()
    per_round = (steps + a.rounds - 1) // a.rounds
    for _ in range(a.rounds):
        for k, (m, opt, crit, targets, full) in runs.items():
            if dbg is not None:
                dbg.prego_debug_ant_full_span(1 if full else 0)
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(per_round)]
            for e0, e1 in evs:
                e0.record()
                step(m, opt, crit, targets)
                e1.record()
            torch.cuda.synchronize()
            times[k] += [e0.elapsed_time(e1) for e0, e1 in evs]
            m.check()
    if dbg is not None:
        dbg.prego_debug_ant_full_span(0)
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(json.dumps({"metric": "training step ms (median of device-event times, B 16, T 128, zero flow, FusedAdamW)", "dtype": a.dtype,
                      "steps_per_config": len(next(iter(times.values()))), "rounds": a.rounds, "median_ms": med,
                      "p10_ms": {k: float(np.percentile(v, 10)) for k, v in times.items()},
                      "p90_ms": {k: float(np.percentile(v, 90)) for k, v in times.items()}}))


def step_bench(a):
    dev, H, C = "cuda:0", 1024, 86
    frames = max(a.steps, 200)
    base = assembly101_cfg(compute_dtype=a.dtype, assume_zero_flow=True)
    m0 = build_model(base, dev)
    m0.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_state_dict(base, 20).items()})
    m0.eval()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x = torch.randn((64, 16, 2048), device=dev, generator=gen).clamp_(min=0)
    table = {}
    for L in (1, 4, 8):
        cfg = anticipation_cfg(base, L)
        m = build_model(cfg, dev)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0).items()})
        m.eval()
        e0, ea = m0.engine(), m.engine()
        for n in (1, 4, 16):
            xs = [x[i, :n].contiguous() for i in range(64)]
            rows = [xs[i][k:k + 1] for i in range(64) for k in range(n)]
            rows = [rows[i * n:(i + 1) * n] for i in range(64)]
            out, arg = torch.empty((n, C), device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
            ao, aa = torch.empty((n, L, C), device=dev), torch.empty((n, L), dtype=torch.int32, device=dev)
            hs = {k: torch.zeros((n, H), device=dev) for k in "abc"}

            def fa(i):
                e0.step(xs[i & 63], None, hs["a"], out=out, argmax=arg)

            def fb(i):
                ea.step(xs[i & 63], None, hs["b"], out=out, argmax=arg, want_ant=True, ant_out=ao, ant_argmax=aa)

            def fc(i):
                r = ea.forward_ragged(rows[i & 63], None, softmax=True, want_out=True, want_argmax=True, h0=hs["c"], want_h_last=True, want_ant=True)
                hs["c"] = r[2]
            paths = {"a_mroad_step": fa, "b_mroada_step": fb, "c_general_T1": fc}
            times, rounds = {k: [] for k in paths}, {k: [] for k in paths}
            for f in paths.values():
                for i in range(a.warmup):
                    f(i)
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for k, f in paths.items():
                    evs = [torch.cuda.Event(enable_timing=True) for _ in range(2 * frames)]
                    r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    r0.record()
                    for i in range(frames):
                        evs[2 * i].record()
                        f(i)
                        evs[2 * i + 1].record()
                    r1.record()
                    torch.cuda.synchronize()
                    times[k] += [evs[2 * i].elapsed_time(evs[2 * i + 1]) * 1e3 for i in range(frames)]
                    rounds[k].append(r0.elapsed_time(r1) * 1e3 / frames)
            e0.check(); ea.check()
            table[f"n{n}_L{L}"] = {k: {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)), "p90_us": float(np.percentile(v, 90)),
                                       "round_us": float(np.median(rounds[k]))} for k, v in times.items()}
            t = table[f"n{n}_L{L}"]
            t["b_minus_a_us"] = t["b_mroada_step"]["median_us"] - t["a_mroad_step"]["median_us"]
        del m
    print(json.dumps({"metric": "per-frame device time, us (median of device-event pairs around every frame; zero flow)", "dtype": a.dtype,
                      "frames_per_path_and_round": frames, "rounds": a.rounds, "table": table}))


def step_wide_bench(a):
    dev, H, C = "cuda:0", 1024, 86
    frames = max(a.steps, 200)
    base = assembly101_cfg(compute_dtype=a.dtype, assume_zero_flow=True)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x = torch.randn((16, 256, 2048), device=dev, generator=gen).clamp_(min=0)
    table = {}
    for name in a.models.split(","):
        L = int(name[1:])
        cfg = anticipation_cfg(base, L) if L else base
        sd = W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0) if L else W.miniroad_state_dict(base, 20, head_gain=8.0)
        m = build_model(cfg, dev)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.eval()
        eng, ant = m.engine(), L > 0
        for n in (int(s) for s in a.streams.split(",")):
            xs = [x[i, :n].contiguous() for i in range(16)]
            rows = [[xs[i][k:k + 1] for k in range(n)] for i in range(16)]
            out, arg = torch.empty((n, C), device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
            ao, aa = (torch.empty((n, L, C), device=dev), torch.empty((n, L), dtype=torch.int32, device=dev)) if ant else (None, None)
            hs = {k: torch.zeros((n, H), device=dev) for k in "wgc"}
            groups = [(lo, min(lo + 16, n)) for lo in range(0, n, 16)]
            views = [[xs[i][lo:hi] for lo, hi in groups] for i in range(16)]
            gv = [(hs["g"][lo:hi], out[lo:hi], arg[lo:hi], ao[lo:hi] if ant else None, aa[lo:hi] if ant else None) for lo, hi in groups]

            def fw(i):
                eng.step_wide(xs[i & 15], None, hs["w"], out=out, argmax=arg, want_ant=ant, ant_out=ao, ant_argmax=aa)

            def fg(i):
                for xv, (hv, ov, av, aov, aav) in zip(views[i & 15], gv):
                    eng.step(xv, None, hv, out=ov, argmax=av, want_ant=ant, ant_out=aov, ant_argmax=aav)

            def fc(i):
                r = eng.forward_ragged(rows[i & 15], None, softmax=True, want_out=True, want_argmax=True, h0=hs["c"], want_h_last=True, want_ant=ant)
                hs["c"] = r[2]
            paths = {k: f for k, f in (("w", fw), ("g", fg), ("c", fc)) if k in a.paths.split(",")}
            times, rounds = {k: [] for k in paths}, {k: [] for k in paths}
            for f in paths.values():
                for i in range(a.warmup):
                    f(i)
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for k, f in paths.items():
                    evs = [torch.cuda.Event(enable_timing=True) for _ in range(2 * frames)]
                    r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    r0.record()
                    for i in range(frames):
                        evs[2 * i].record()
                        f(i)
                        evs[2 * i + 1].record()
                    r1.record()
                    torch.cuda.synchronize()
                    times[k] += [evs[2 * i].elapsed_time(evs[2 * i + 1]) * 1e3 for i in range(frames)]
                    rounds[k].append(r0.elapsed_time(r1) * 1e3 / frames)
            eng.check()
            t = {k: {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)), "p90_us": float(np.percentile(v, 90)),
                     "round_us": float(np.median(rounds[k]))} for k, v in times.items()}
            if "w" in t and "g" in t:
                t["g_minus_w_us"] = t["g"]["median_us"] - t["w"]["median_us"]
                t["spreads_us"] = (t["g"]["p90_us"] - t["g"]["p10_us"]) + (t["w"]["p90_us"] - t["w"]["p10_us"])
                t["w_below_g_by_more_than_the_spreads"] = t["g_minus_w_us"] > t["spreads_us"]
            table[f"{name}_n{n}"] = t
            print(json.dumps({f"{name}_n{n}": t}), file=sys.stderr, flush=True)
        del m, eng
    print(json.dumps({"metric": "per-frame device time, us (median of device-event pairs around every frame; zero flow): w = step_wide, "
                                "g = ceil(n / 16) step calls, c = general forward at T = 1", "dtype": a.dtype,
                      "frames_per_path_and_round": frames, "rounds": a.rounds, "table": table}))


def step_pool_bench(a):
    import random

    from prego_amd.aggregate import OnlineRecord
    dev, H, C, cap = "cuda:0", 1024, 86, 256
    frames = max(a.steps, 200)
    base = assembly101_cfg(compute_dtype=a.dtype, assume_zero_flow=True)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x = torch.randn((16, 256, 2048), device=dev, generator=gen).clamp_(min=0)
    table = {}
    for name in a.models.split(","):
        L = int(name[1:])
        cfg = anticipation_cfg(base, L) if L else base
        sd = W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0) if L else W.miniroad_state_dict(base, 20, head_gain=8.0)
        m = build_model(cfg, dev)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.eval()
        eng, ant = m.engine(), L > 0
        for n in (int(s) for s in a.streams.split(",")):
            pool = m.stream_pool(capacity=cap)
            for _ in range(cap):
                pool.open()
            slots = random.Random(n).sample(range(cap), n)            # scattered, in no order
            xs = [x[i, :n].contiguous() for i in range(16)]
            out, arg = torch.empty((n, C), device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
            ao, aa = (torch.empty((n, L, C), device=dev), torch.empty((n, L), dtype=torch.int32, device=dev)) if ant else (None, None)
            hw = torch.zeros((n, H), device=dev)
            states, idx = torch.zeros((cap, H), device=dev), torch.tensor(slots, device=dev)
            recs = [OnlineRecord(200, C, 1024) for _ in range(n)]

            def fp(i):
                pool.push(slots, xs[i & 15], None, out=out, argmax=arg, want_ant=ant, ant_out=ao, ant_argmax=aa)

            def fw(i):
                eng.step_wide(xs[i & 15], None, hw, out=out, argmax=arg, want_ant=ant, ant_out=ao, ant_argmax=aa)

            def ft(i):
                h = states.index_select(0, idx)
                eng.step_wide(xs[i & 15], None, h, out=out, argmax=arg, want_ant=ant, ant_out=ao, ant_argmax=aa)
                states.index_copy_(0, idx, h)
                for r, v in zip(recs, arg.cpu().tolist()):
                    r.push(v)
            paths = {"p": fp, "w": fw, "t": ft}
            times, rounds = {k: [] for k in paths}, {k: [] for k in paths}
            for f in paths.values():
                for i in range(a.warmup):
                    f(i)
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for k, f in paths.items():
                    evs = [torch.cuda.Event(enable_timing=True) for _ in range(2 * frames)]
                    r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    r0.record()
                    for i in range(frames):
                        evs[2 * i].record()
                        f(i)
                        evs[2 * i + 1].record()
                    r1.record()
                    torch.cuda.synchronize()
                    times[k] += [evs[2 * i].elapsed_time(evs[2 * i + 1]) * 1e3 for i in range(frames)]
                    rounds[k].append(r0.elapsed_time(r1) * 1e3 / frames)
            eng.check()
            t = {k: {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)), "p90_us": float(np.percentile(v, 90)),
                     "round_us": float(np.median(rounds[k]))} for k, v in times.items()}
            t["p_minus_w_us"] = t["p"]["median_us"] - t["w"]["median_us"]
            t["p_spread_us"] = t["p"]["p90_us"] - t["p"]["p10_us"]
            t["p_below_t"] = t["p"]["median_us"] < t["t"]["median_us"]
            table[f"{name}_n{n}"] = t
            print(json.dumps({f"{name}_n{n}": t}), file=sys.stderr, flush=True)
            del pool
        del m, eng
    print(json.dumps({"metric": "per-tick device time, us (median of device-event pairs around every tick; zero flow; n_active scattered slots of a "
                                "256-slot pool): p = StreamPool.push, w = dense step_wide, t = index_select + step_wide + index_copy_ + "
                                "argmax.cpu() + host vote", "dtype": a.dtype, "frames_per_path_and_round": frames, "rounds": a.rounds,
                      "table": table}))


def step_pool_feed_bench(a):
    import ctypes as Ct
    import random

    dev, C, cap = "cuda:0", 86, 256
    frames = max(a.steps, 200)
    base = assembly101_cfg(compute_dtype=a.dtype, assume_zero_flow=True)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x = torch.randn((16, 256, 2048), device=dev, generator=gen).clamp_(min=0)
    table = {}
    for name in a.models.split(","):
        L = int(name[1:])
        cfg = anticipation_cfg(base, L) if L else base
        sd = W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0) if L else W.miniroad_state_dict(base, 20, head_gain=8.0)
        m = build_model(cfg, dev)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.eval()
        eng, ant = m.engine(), L > 0
        for n in (int(s) for s in a.streams.split(",")):
            pool = m.stream_pool(capacity=cap, window=a.vote_window)      # max_events 1024: the record events(slot) copies is 8.5 KB
            feed = pool.event_feed(max_out=1024, depth=2)
            for _ in range(cap):
                pool.open()
            slots = random.Random(n).sample(range(cap), n)            # scattered, in no order
            every = (Ct.c_int32 * cap)(*range(cap))
            xs = [x[i, :n].contiguous() for i in range(16)]
            out, arg = torch.empty((n, C), device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
            ao, aa = (torch.empty((n, L, C), device=dev), torch.empty((n, L), dtype=torch.int32, device=dev)) if ant else (None, None)
            seen = {"a": 0, "b": 0, "ticks": 0, "hit": 0, "prev": None, "last": {}}

            def fresh():
                """every record empty again, outside the timed part: a leg's frames never fill a record"""
                if seen["prev"] is not None:
                    seen["prev"].events()
                    seen["prev"] = None
                pool._check(pool.lib.prego_stream_pool_reset(pool.p, cap, every, None))
                feed.forget(range(cap))
                seen["last"] = {}
                torch.cuda.synchronize()

            def fc(i):
                pool.push(slots, xs[i & 15], None, out=out, argmax=arg, want_ant=ant, ant_out=ao, ant_argmax=aa)

            def fa(i):
                fc(i)
                t = feed.drain()
                if seen["prev"] is not None:                          # the ticket of the tick before: its copy has had a tick to land
                    got = len(seen["prev"].events())
                    seen["a"] += got
                    seen["hit"] += got > 0
                seen["prev"] = t
                seen["ticks"] += 1

            def fb(i):
                fc(i)
                for s in slots:                                       # one blocking record copy per slot, then the diff against the last poll
                    n_ev = len(pool.events(s)["pred"])
                    seen["b"] += n_ev - seen["last"].get(s, 0)
                    seen["last"][s] = n_ev
            paths = {"a": fa, "b": fb, "c": fc}
            times, rounds = {k: [] for k in paths}, {k: [] for k in paths}
            for f in paths.values():
                fresh()
                for i in range(a.warmup):
                    f(i)
            seen.update(a=0, b=0, ticks=0, hit=0)
            for _ in range(a.rounds):
                for k, f in paths.items():
                    fresh()
                    evs = [torch.cuda.Event(enable_timing=True) for _ in range(2 * frames)]
                    r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    r0.record()
                    for i in range(frames):
                        evs[2 * i].record()
                        f(i)
                        evs[2 * i + 1].record()
                    r1.record()
                    torch.cuda.synchronize()
                    times[k] += [evs[2 * i].elapsed_time(evs[2 * i + 1]) * 1e3 for i in range(frames)]
                    rounds[k].append(r0.elapsed_time(r1) * 1e3 / frames)
            fresh()
            eng.check()
            t = {k: {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)), "p90_us": float(np.percentile(v, 90)),
                     "round_us": float(np.median(rounds[k]))} for k, v in times.items()}
            t["a_minus_c_us"] = t["a"]["median_us"] - t["c"]["median_us"]
            t["b_minus_c_us"] = t["b"]["median_us"] - t["c"]["median_us"]
            t["a_minus_c_round_us"] = t["a"]["round_us"] - t["c"]["round_us"]
            t["b_minus_c_round_us"] = t["b"]["round_us"] - t["c"]["round_us"]
            t["c_spread_us"] = t["c"]["p90_us"] - t["c"]["p10_us"]
            t["events_per_tick"] = seen["a"] / max(seen["ticks"], 1)
            t["ticks_with_events"] = seen["hit"] / max(seen["ticks"], 1)
            t["events_a"], t["events_b"] = seen["a"], seen["b"]         # (a) reads one tick late: it may lack each round's last tick
            table[f"{name}_n{n}"] = t
            print(json.dumps({f"{name}_n{n}": t}), file=sys.stderr, flush=True)
            del feed, pool
        del m, eng
    print(json.dumps({"metric": "per-tick device time, us (median of device-event pairs around every tick; zero flow; n_active scattered slots of a "
                                "256-slot pool, 1024 events per record): a = push + EventFeed.drain + reading the previous tick's ticket, b = push + "
                                "events(slot) for every active slot, c = push alone; round_us = a whole round between two events / its ticks",
                      "dtype": a.dtype, "vote_window": a.vote_window, "frames_per_path_and_round": frames, "rounds": a.rounds, "table": table}))


def step_pool_snapshot_bench(a):
    import random

    from pool_snapshot_legs import snapshot_legs
    dev, cap = "cuda:0", 256
    calls = max(a.steps, 100)
    base = assembly101_cfg(compute_dtype=a.dtype, assume_zero_flow=True)
    m = build_model(base, dev)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_state_dict(base, 20, head_gain=8.0).items()})
    m.eval()
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x = torch.randn((16, 256, 2048), device=dev, generator=gen).clamp_(min=0)
    table = {}
    for n in (int(s) for s in a.streams.split(",")):
        pool_a, pool_b = m.stream_pool(capacity=cap, window=7), m.stream_pool(capacity=cap, window=7)
        for _ in range(cap):
            pool_a.open()
            pool_b.open()
        slots_a, slots_b = random.Random(n).sample(range(cap), n), random.Random(n + 1).sample(range(cap), n)
        for i in range(50):                                           # streams of 50 frames: a state row and a few events per slot
            pool_a.push(slots_a, x[i & 15, :n].contiguous(), None, want_ant=False)
        t = snapshot_legs(pool_a, pool_b, slots_a, slots_b, lambda p, s: p.state(s), calls, a.warmup, a.rounds)
        m.engine().check()
        table[f"n{n}"] = t
        print(json.dumps({f"n{n}": t}), file=sys.stderr, flush=True)
        del pool_a, pool_b
    line = json.dumps({"metric": "device time per call, us (median of device-event pairs around every call; n scattered slots of a 256-slot "
                                 "MiniROAD pool, 1024 events per record): s = StreamPool.snapshot, r = StreamPool.restore into a second pool "
                                 "(status copy included), rc = prego_stream_pool_restore alone, t = state(slot) + record copy per slot; "
                                 "floor_us = n images read and written once at 6.3 TB/s",
                       "device": torch.cuda.get_device_name(0), "dtype": a.dtype, "calls_per_path_and_round": calls, "rounds": a.rounds,
                       "warmup_calls": a.warmup, "table": table})
    print(line)
    out_path = a.out or os.path.join("profiles", "stream_pool", "snapshot_bench.json")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


def step_pool_frames_bench(a):
    import random
    dev, C, cap = "cuda:0", 86, 256
    ticks = max(a.steps, 200)
    base = assembly101_cfg(compute_dtype=a.dtype, assume_zero_flow=True)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    cells = [(n, K) for n in (1, 4, 16) for K in (2, 4, 8, 16)] + [(64, 2), (64, 4)]
    table = {}
    for name in a.models.split(","):
        L = int(name[1:])
        cfg = anticipation_cfg(base, L) if L else base
        sd = W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0) if L else W.miniroad_state_dict(base, 20, head_gain=8.0)
        m = build_model(cfg, dev)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.eval()
        eng, ant = m.engine(), L > 0
        for n, K in cells:
            pools = {k: m.stream_pool(capacity=cap) for k in "fk"}       # one pool per route: both streams of states advance alike
            for pool in pools.values():
                for _ in range(cap):
                    pool.open()
            slots = random.Random(n).sample(range(cap), n)            # scattered, in no order
            x = torch.randn((16, n, K, 2048), device=dev, generator=gen).clamp_(min=0)
            xt = [[x[i, :, t].contiguous() for t in range(K)] for i in range(16)]
            out, arg = torch.empty((n, K, C), device=dev), torch.empty((n, K), dtype=torch.int32, device=dev)
            ao, aa = (torch.empty((n, K, L, C), device=dev), torch.empty((n, K, L), dtype=torch.int32, device=dev)) if ant else (None, None)
            o1, a1 = torch.empty((n, C), device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
            ao1, aa1 = (torch.empty((n, L, C), device=dev), torch.empty((n, L), dtype=torch.int32, device=dev)) if ant else (None, None)

            def ff(i):
                pools["f"].push_frames(slots, x[i & 15], None, out=out, argmax=arg, want_ant=ant, ant_out=ao, ant_argmax=aa)

            def fk(i):
                for t in range(K):
                    pools["k"].push(slots, xt[i & 15][t], None, out=o1, argmax=a1, want_ant=ant, ant_out=ao1, ant_argmax=aa1)
            paths = {"f": ff, "k": fk}
            times, rounds = {k: [] for k in paths}, {k: [] for k in paths}
            for f in paths.values():
                for i in range(a.warmup):
                    f(i)
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for k, f in paths.items():
                    evs = [torch.cuda.Event(enable_timing=True) for _ in range(2 * ticks)]
                    r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    r0.record()
                    for i in range(ticks):
                        evs[2 * i].record()
                        f(i)
                        evs[2 * i + 1].record()
                    r1.record()
                    torch.cuda.synchronize()
                    times[k] += [evs[2 * i].elapsed_time(evs[2 * i + 1]) * 1e3 for i in range(ticks)]
                    rounds[k].append(r0.elapsed_time(r1) * 1e3 / ticks)
            eng.check()
            t = {k: {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)), "p90_us": float(np.percentile(v, 90)),
                     "round_us": float(np.median(rounds[k])), "median_us_per_frame": float(np.median(v)) / K} for k, v in times.items()}
            t["k_minus_f_us"] = t["k"]["median_us"] - t["f"]["median_us"]
            t["spreads_us"] = (t["k"]["p90_us"] - t["k"]["p10_us"]) + (t["f"]["p90_us"] - t["f"]["p10_us"])
            t["f_below_k_by_more_than_the_spreads"] = t["k_minus_f_us"] > t["spreads_us"]
            table[f"{name}_n{n}_K{K}"] = t
            print(json.dumps({f"{name}_n{n}_K{K}": t}), file=sys.stderr, flush=True)
            del pools
        for n in (1, 4, 16):
            hi, lo = table[f"{name}_n{n}_K16"]["f"]["median_us"], table[f"{name}_n{n}_K8"]["f"]["median_us"]
            table[f"{name}_n{n}_marginal_us_per_frame"] = (hi - lo) / 8.0
        del m, eng
    print(json.dumps({"metric": "per-call device time, us (median of device-event pairs around every call; zero flow; n_active scattered slots of a "
                                "256-slot pool): f = ONE StreamPool.push_frames of K frames, k = K successive StreamPool.push calls",
                      "dtype": a.dtype, "calls_per_path_and_round": ticks, "rounds": a.rounds, "table": table}))


def _ragged_workloads(n):
    """{name: counts} of the ragged leg for n streams, every sum <= 256"""
    import random
    seed = n
    while True:                                               # the first seed whose draw fits a call
        rng = random.Random(seed)
        uni = [rng.randint(1, 8) for _ in range(n)]
        if sum(uni) <= 256:
            break
        seed += 1
    return {"uniform1-8": uni, "straggler32": [1] * (n // 2) + [32] + [1] * (n - n // 2 - 1), "equal4": [4] * n}


def step_pool_ragged_bench(a):
    import random
    from prego_amd.stream_pool import burst_offsets
    dev, C, cap = "cuda:0", 86, 256
    ticks = max(a.steps, 200)
    base = assembly101_cfg(compute_dtype=a.dtype, assume_zero_flow=True)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    table = {}
    for name in a.models.split(","):
        L = int(name[1:])
        cfg = anticipation_cfg(base, L) if L else base
        sd = W.miniroad_a_state_dict(cfg, 20, head_gain=8.0, ant_gain=4.0) if L else W.miniroad_state_dict(base, 20, head_gain=8.0)
        m = build_model(cfg, dev)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.eval()
        eng, ant = m.engine(), L > 0
        for n in (16, 64):
            for wl, counts in _ragged_workloads(n).items():
                pools = {k: m.stream_pool(capacity=cap) for k in "rg"}       # one pool per route: both streams of states advance alike
                for pool in pools.values():
                    for _ in range(cap):
                        pool.open()
                slots = random.Random(n).sample(range(cap), n)            # scattered, in no order
                R, off = sum(counts), burst_offsets(counts)
                x = torch.randn((8, R, 2048), device=dev, generator=gen).clamp_(min=0)
                out, arg = torch.empty((R, C), device=dev), torch.empty((R,), dtype=torch.int32, device=dev)
                ao, aa = (torch.empty((R, L, C), device=dev), torch.empty((R, L), dtype=torch.int32, device=dev)) if ant else (None, None)
                # the grouped route's inputs and buffers are laid out ahead of the timed calls: [n_g, K, d] per group of equal count
                groups = {}
                for i, k in enumerate(counts):
                    groups.setdefault(k, []).append(i)
                gcalls = []
                for K, mem in groups.items():
                    rows = torch.tensor([off[i] + t for i in mem for t in range(K)], device=dev)
                    ng = len(mem)
                    gcalls.append(([slots[i] for i in mem], [x[j][rows].view(ng, K, 2048).contiguous() for j in range(8)],
                                   torch.empty((ng, K, C), device=dev), torch.empty((ng, K), dtype=torch.int32, device=dev),
                                   torch.empty((ng, K, L, C), device=dev) if ant else None,
                                   torch.empty((ng, K, L), dtype=torch.int32, device=dev) if ant else None))

                def fr(i):
                    pools["r"].push_ragged(slots, counts, x[i & 7], None, out=out, argmax=arg, want_ant=ant, ant_out=ao, ant_argmax=aa)

                def fg(i):
                    for gs, gx, go, ga, gao, gaa in gcalls:
                        pools["g"].push_frames(gs, gx[i & 7], None, out=go, argmax=ga, want_ant=ant, ant_out=gao, ant_argmax=gaa)
                paths = {"r": fr, "g": fg}
                times, rounds = {k: [] for k in paths}, {k: [] for k in paths}
                for f in paths.values():
                    for i in range(a.warmup):
                        f(i)
                torch.cuda.synchronize()
                for _ in range(a.rounds):
                    for k, f in paths.items():
                        evs = [torch.cuda.Event(enable_timing=True) for _ in range(2 * ticks)]
                        r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        r0.record()
                        for i in range(ticks):
                            evs[2 * i].record()
                            f(i)
                            evs[2 * i + 1].record()
                        r1.record()
                        torch.cuda.synchronize()
                        times[k] += [evs[2 * i].elapsed_time(evs[2 * i + 1]) * 1e3 for i in range(ticks)]
                        rounds[k].append(r0.elapsed_time(r1) * 1e3 / ticks)
                eng.check()
                t = {k: {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)), "p90_us": float(np.percentile(v, 90)),
                         "round_us": float(np.median(rounds[k]))} for k, v in times.items()}
                t.update(rows=R, groups=len(groups), max_count=max(counts), g_minus_r_us=t["g"]["median_us"] - t["r"]["median_us"])
                width = max(t["r"]["p90_us"] - t["r"]["p10_us"], t["g"]["p90_us"] - t["g"]["p10_us"])
                t["larger_p10_p90_width_us"] = width
                if wl == "equal4":
                    t["r_within_control"] = abs(t["g_minus_r_us"]) <= width
                table[f"{name}_n{n}_{wl}"] = t
                print(json.dumps({f"{name}_n{n}_{wl}": t}), file=sys.stderr, flush=True)
                del pools
        del m, eng
    print(json.dumps({"metric": "per-call device time, us (median of device-event pairs around every call; zero flow; n scattered slots of a "
                                "256-slot pool): r = ONE StreamPool.push_ragged, g = one StreamPool.push_frames per group of equal count",
                      "dtype": a.dtype, "calls_per_path_and_round": ticks, "rounds": a.rounds, "table": table}))


if __name__ == "__main__":
    main()
