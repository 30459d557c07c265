"""Live Transformer streams: `TransformerStreamPool.push` against the route a caller has without it.

    python scripts/vit_stream_bench.py [--streams 4,16,64,256] [--dtypes bf16,fp16] [--window 128] [--ticks 100] [--rounds 4]
                                       [--out profiles/vit_stream_pool/push_bench.json]
    python scripts/vit_stream_bench.py --bursts 4x64,8x64,4x256,8x256 [--out profiles/vit_stream_pool/bursts_bench.json]

(p) `push`: one call per tick for n_active scattered slots of a 256-slot pool - the frame is encoded once, the rings give the windows,
    the record takes the argmax on the device.
(t) the torch route: the caller keeps the last `window` raw feature rows of every stream, shifts the new frame in with torch.cat,
    runs `ViTEnc.forward` on the [n, window, 2048] + [n, window, 2048] windows (every frame encoded again each tick), copies the
    argmax to the host and votes there (`OnlineRecord`).
Protocol: 20 warm-up ticks per route, then alternating rounds, a device-event pair around every tick; median and p10 - p90 in us.  (t)'s
device-event time includes the host's wait for the argmax copy: that wait is in the caller's tick.  One JSON line on stdout, the same
object in --out.

--bursts KxR: a backlog of K frames on each of R / K scattered slots, R windows in all.
(b) `push_bursts`: one call - one encoding GEMM at M = R, one encoder batch of R windows.
(k) K `push` calls that deliver the same frames to the same slots - K encoding GEMMs at M = R / K, K launch chains, K encoder batches.
The same protocol; a tick is the whole backlog (one call of (b), K calls of (k)).

--snapshot: slot images of n = 4 / 16 / 64 scattered slots whose rings are full, a device-event pair per CALL:
(s) `snapshot` of the n slots, (r) `restore` of them into a second pool (status copy included), (rc) the C restore alone, (t) the read
route there was before - `window(slot)` plus the record copy, per slot.  `floor_us`: the image bytes read and written once at the
achievable HBM rate (scripts/pool_snapshot_legs.py).

    python scripts/vit_stream_bench.py --snapshot [--streams 4,16,64] [--dtypes fp16] [--out profiles/vit_stream_pool/snapshot_bench.json]"""
import argparse
import json
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prego_amd import weights as W                                 # noqa: E402
from prego_amd.aggregate import OnlineRecord                       # noqa: E402
from prego_amd.config import assembly101_cfg                       # noqa: E402
from prego_amd.registry import build_model                         # noqa: E402
import prego_amd.transformer                                       # noqa: E402,F401


def measure(paths, a):
    """the protocol: a.warmup ticks per route, then a.rounds alternating rounds of a.ticks ticks, a device-event pair around every tick"""
    times, rounds = {k: [] for k in paths}, {k: [] for k in paths}
    for f in paths.values():
        for i in range(a.warmup):
            f(i)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for k, f in paths.items():
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(2 * a.ticks)]
            r0, r1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            r0.record()
            for i in range(a.ticks):
                evs[2 * i].record()
                f(i)
                evs[2 * i + 1].record()
            r1.record()
            torch.cuda.synchronize()
            times[k] += [evs[2 * i].elapsed_time(evs[2 * i + 1]) * 1e3 for i in range(a.ticks)]
            rounds[k].append(r0.elapsed_time(r1) * 1e3 / a.ticks)
    return {k: {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)), "p90_us": float(np.percentile(v, 90)),
                "round_us": float(np.median(rounds[k]))} for k, v in times.items()}


def bursts_main(a):
    dev, C, cap, T = "cuda:0", 86, 256, a.window
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x = torch.randn((4, 256, 2, 2048), device=dev, generator=gen).clamp_(min=0)        # 4 backlogs of 256 packed rows, reused in turn
    table = {}
    for dtype in a.dtypes.split(","):
        cfg = assembly101_cfg(model="Transformer", window_size=T, patch_dim=1, num_heads=8, attn_dropout_rate=0.0, dropout=0.0,
                              num_layers=a.layers, compute_dtype=dtype)
        m = build_model(cfg, dev)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in W.vit_state_dict(cfg, 20).items()})
        m.eval()
        for K, R in (tuple(int(v) for v in cell.split("x")) for cell in a.bursts.split(",")):
            n = R // K
            assert n * K == R and R <= 256
            pools = {"b": m.stream_pool(capacity=cap), "k": m.stream_pool(capacity=cap)}
            for pool in pools.values():
                for _ in range(cap):
                    pool.open()
            slots = random.Random(R + K).sample(range(cap), n)        # scattered, in no order
            packed = [(x[i, :R, 0].contiguous(), x[i, :R, 1].contiguous()) for i in range(4)]          # slot i owns rows i K .. i K + K)
            frames = [[(r.view(n, K, 2048)[:, k].contiguous(), f.view(n, K, 2048)[:, k].contiguous()) for k in range(K)] for r, f in packed]
            out, arg = torch.empty((R, C), device=dev), torch.empty((R,), dtype=torch.int32, device=dev)
            out1, arg1 = torch.empty((n, C), device=dev), torch.empty((n,), dtype=torch.int32, device=dev)

            def fb(i):
                pools["b"].push_bursts(slots, K, packed[i & 3][0], packed[i & 3][1], out=out, argmax=arg)

            def fk(i):
                for r, f in frames[i & 3]:
                    pools["k"].push(slots, r, f, out=out1, argmax=arg1)
            t = measure({"b": fb, "k": fk}, a)
            t["k_over_b"] = t["k"]["median_us"] / t["b"]["median_us"]
            t["b_below_k"] = t["b"]["median_us"] < t["k"]["median_us"]
            table[f"{dtype}_K{K}_R{R}"] = t
            print(json.dumps({f"{dtype}_K{K}_R{R}": t}), file=sys.stderr, flush=True)
            del pools
        del m
    res = {"metric": "device time per backlog, us (median of device-event pairs around every tick; K frames on each of R / K scattered "
                     "slots of a 256-slot pool): b = one TransformerStreamPool.push_bursts, k = K TransformerStreamPool.push calls with the "
                     "same frames for the same slots",
           "device": torch.cuda.get_device_name(0), "window": T, "layers": a.layers, "ticks_per_path_and_round": a.ticks, "rounds": a.rounds,
           "warmup_ticks": a.warmup, "table": table}
    line = json.dumps(res)
    print(line)
    out_path = a.out or os.path.join("profiles", "vit_stream_pool", "bursts_bench.json")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


def snapshot_main(a):
    from pool_snapshot_legs import snapshot_legs
    dev, cap, T = "cuda:0", 256, a.window
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x = torch.randn((16, 64, 2, 2048), device=dev, generator=gen).clamp_(min=0)
    table = {}
    for dtype in a.dtypes.split(","):
        cfg = assembly101_cfg(model="Transformer", window_size=T, patch_dim=1, num_heads=8, attn_dropout_rate=0.0, dropout=0.0,
                              num_layers=a.layers, compute_dtype=dtype)
        m = build_model(cfg, dev)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in W.vit_state_dict(cfg, 20).items()})
        m.eval()
        for n in (int(s) for s in a.streams.split(",")):
            assert n <= 64
            pool_a, pool_b = m.stream_pool(capacity=cap), m.stream_pool(capacity=cap)
            for _ in range(cap):
                pool_a.open()
                pool_b.open()
            slots_a, slots_b = random.Random(n).sample(range(cap), n), random.Random(n + 1).sample(range(cap), n)
            for i in range(T + 5):                                    # every ring full and wrapped
                pool_a.push(slots_a, x[i & 15, :n, 0].contiguous(), x[i & 15, :n, 1].contiguous())
            t = snapshot_legs(pool_a, pool_b, slots_a, slots_b, lambda p, s: p.window(s), a.ticks, a.warmup, a.rounds)
            table[f"{dtype}_n{n}"] = t
            print(json.dumps({f"{dtype}_n{n}": t}), file=sys.stderr, flush=True)
            del pool_a, pool_b
        del m
    res = {"metric": "device time per call, us (median of device-event pairs around every call; n scattered slots of a 256-slot pool, rings "
                     "full): s = TransformerStreamPool.snapshot, r = restore into a second pool (status copy included), rc = "
                     "prego_vit_stream_pool_restore alone, t = window(slot) + record copy per slot; floor_us = n images read and written "
                     "once at 6.3 TB/s",
           "device": torch.cuda.get_device_name(0), "window": T, "layers": a.layers, "calls_per_path_and_round": a.ticks, "rounds": a.rounds,
           "warmup_calls": a.warmup, "table": table}
    line = json.dumps(res)
    print(line)
    out_path = a.out or os.path.join("profiles", "vit_stream_pool", "snapshot_bench.json")
    os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
    with open(out_path, "w") as f:
        f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snapshot", action="store_true", help="snapshot / restore of n slots against window(slot) + record copy per slot")
    ap.add_argument("--streams", default=None, help="default: 4,16,64,256; with --snapshot 4,16,64")
    ap.add_argument("--dtypes", default="bf16,fp16")
    ap.add_argument("--window", type=int, default=128)
    ap.add_argument("--layers", type=int, default=1)
    ap.add_argument("--ticks", type=int, default=100, help="ticks per route and round")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--bursts", default="", help="KxR cells, e.g. 4x64,8x64,4x256,8x256: push_bursts against K push calls instead of the push cells")
    ap.add_argument("--out", default=None, help="default: profiles/vit_stream_pool/push_bench.json, with --bursts bursts_bench.json")
    a = ap.parse_args()
    a.streams = a.streams or ("4,16,64" if a.snapshot else "4,16,64,256")
    if a.snapshot:
        return snapshot_main(a)
    if a.bursts:
        return bursts_main(a)
    a.out = a.out or os.path.join("profiles", "vit_stream_pool", "push_bench.json")
    dev, C, cap, T = "cuda:0", 86, 256, a.window
    gen = torch.Generator(device=dev)
    gen.manual_seed(1234)
    x = torch.randn((16, 256, 2, 2048), device=dev, generator=gen).clamp_(min=0)       # 16 ticks of frames, reused in turn
    table = {}
    for dtype in a.dtypes.split(","):
        cfg = assembly101_cfg(model="Transformer", window_size=T, patch_dim=1, num_heads=8, attn_dropout_rate=0.0, dropout=0.0,
                              num_layers=a.layers, compute_dtype=dtype)
        m = build_model(cfg, dev)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in W.vit_state_dict(cfg, 20).items()})
        m.eval()
        for n in (int(s) for s in a.streams.split(",")):
            pool = m.stream_pool(capacity=cap)
            for _ in range(cap):
                pool.open()
            slots = random.Random(n).sample(range(cap), n)            # scattered, in no order
            rgbs = [x[i, :n, 0].contiguous() for i in range(16)]
            flows = [x[i, :n, 1].contiguous() for i in range(16)]
            out, arg = torch.empty((n, C), device=dev), torch.empty((n,), dtype=torch.int32, device=dev)
            win = {"rgb": torch.zeros((n, T, 2048), device=dev), "flow": torch.zeros((n, T, 2048), device=dev)}
            recs = [OnlineRecord(200, C, 1024) for _ in range(n)]

            def fp(i):
                pool.push(slots, rgbs[i & 15], flows[i & 15], out=out, argmax=arg)

            def ft(i):
                win["rgb"] = torch.cat([win["rgb"][:, 1:], rgbs[i & 15][:, None]], dim=1)
                win["flow"] = torch.cat([win["flow"][:, 1:], flows[i & 15][:, None]], dim=1)
                with torch.no_grad():
                    ids = m(win["rgb"], win["flow"])["logits"][:, 0].argmax(1)
                for r, v in zip(recs, ids.cpu().tolist()):
                    r.push(v)
            t = measure({"p": fp, "t": ft}, a)
            t["t_over_p"] = t["t"]["median_us"] / t["p"]["median_us"]
            t["p_below_t"] = t["p"]["median_us"] < t["t"]["median_us"]
            table[f"{dtype}_n{n}"] = t
            print(json.dumps({f"{dtype}_n{n}": t}), file=sys.stderr, flush=True)
            del pool
        del m
    res = {"metric": "per-tick device time, us (median of device-event pairs around every tick; n_active scattered slots of a 256-slot pool): "
                     "p = TransformerStreamPool.push, t = torch.cat of the raw windows + ViTEnc.forward + argmax.cpu() + host vote",
           "device": torch.cuda.get_device_name(0), "window": T, "layers": a.layers, "ticks_per_path_and_round": a.ticks, "rounds": a.rounds,
           "warmup_ticks": a.warmup, "table": table}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
