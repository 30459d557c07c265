"""Live Transformer streams: `TransformerStreamPool.push` against the route a caller has without it.

    python scripts/vit_stream_bench.py [--streams 4,16,64,256] [--dtypes bf16,fp16] [--window 128] [--ticks 100] [--rounds 4]
                                       [--out profiles/vit_stream_pool/push_bench.json]

(p) `push`: one call per tick for n_active scattered slots of a 256-slot pool - the frame is encoded once, the rings give the windows,
    the record takes the argmax on the device.
(t) the torch route: the caller keeps the last `window` raw feature rows of every stream, shifts the new frame in with torch.cat,
    runs `ViTEnc.forward` on the [n, window, 2048] + [n, window, 2048] windows (every frame encoded again each tick), copies the
    argmax to the host and votes there (`OnlineRecord`).
Protocol: 20 warm-up ticks per route, then alternating rounds, a device-event pair around every tick; median and p10 - p90 in us.  (t)'s
device-event time includes the host's wait for the argmax copy: that wait is in the caller's tick.  One JSON line on stdout, the same
object in --out."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="4,16,64,256")
    ap.add_argument("--dtypes", default="bf16,fp16")
    ap.add_argument("--window", type=int, default=128)
    ap.add_argument("--layers", type=int, default=1)
    ap.add_argument("--ticks", type=int, default=100, help="ticks per route and round")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "vit_stream_pool", "push_bench.json"))
    a = ap.parse_args()
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
            paths = {"p": fp, "t": ft}
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
            t = {k: {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)), "p90_us": float(np.percentile(v, 90)),
                     "round_us": float(np.median(rounds[k]))} for k, v in times.items()}
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
