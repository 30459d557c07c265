#!/usr/bin/env python3
"""What a decode-pool push costs beside the recurrent tick it rides behind.  86 classes, uniform transitions (switch 2048,
stay 0), lag 64 and 256; the scores are what the stream pool's own push returns (softmax=True) for seeded features on real-sized seeded
weights.  Three call shapes: 256 slots x 1 frame (`push`), 8 slots x 32 frames (`push_frames`), 64 slots with 1..6 frames each
(`push_ragged`).  Beside each, in ONE process and in alternating order:
  decode   `DecodePool.push` of that shape, all three outputs written, the slots in steady state (more than `lag` frames behind them);
  tick     `StreamPool.push*` of the same shape: the step whose scores the decoder takes;
  clone    a device clone() of half the bytes the decode call touches (a clone reads and writes): rows, outputs, keys both ways, the
           ring rows staged and written - its memory floor.
A sample is a device-event pair around --batch calls, divided by the batch; median and p10 - p90 over --rounds samples.  Prints one
JSON line; --out PATH also writes it.
    python3 scripts/probes/decode_pool_time.py [--rounds 30] [--batch 20] [--out PATH]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CLASSES, SWITCH = 86, 2048


def stats(v):
    q = lambda p: sorted(v)[min(len(v) - 1, int(p * len(v)))]
    return {"median": round(q(0.5), 2), "p10": round(q(0.1), 2), "p90": round(q(0.9), 2), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("decode_pool_time: no GPU; a time is measured on the device or not at all")
    from prego_amd import weights as W
    from prego_amd.config import anticipation_cfg, assembly101_cfg
    from prego_amd.decode import uniform_transitions
    from prego_amd.engine import MiniRoadEngine
    from prego_amd.stream_pool import DecodePool, StreamPool
    dev = "cuda:0"
    cfg = anticipation_cfg(assembly101_cfg(hidden_dim=1024), 3)
    sd = {k: torch.from_numpy(v).to(dev) for k, v in W.miniroad_a_state_dict(cfg, 20).items()}
    eng = MiniRoadEngine(2048, 2048, 2048, 1024, CLASSES, dev, "bf16")
    eng.set_weights(sd)
    trans = uniform_transitions(CLASSES, SWITCH)
    rng = np.random.default_rng(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    feat = lambda rows: torch.randn((rows, 2048), device="cuda", generator=g).clamp_(min=0)
    shapes = {"256x1": [1] * 256, "8x32": [32] * 8, "ragged64": rng.integers(1, 7, 64).tolist()}
    assert sum(shapes["ragged64"]) <= 256
    out = {"probe": "decode_pool_time", "device": torch.cuda.get_device_name(0), "classes": CLASSES, "switch_cost": SWITCH,
           "batch": a.batch, "unit": "microseconds per call", "shapes": {}}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    for name, counts in shapes.items():
        n, R = len(counts), int(sum(counts))
        sp = StreamPool(eng, capacity=256)
        slots = [sp.open() for _ in range(n)]
        rgb, flow = feat(R), feat(R)
        if name == "256x1":
            tick = lambda: sp.push(slots, rgb, flow, want_ant=False)
        elif name == "8x32":
            r3, f3 = rgb.view(n, 32, 2048), flow.view(n, 32, 2048)
            tick = lambda: sp.push_frames(slots, r3, f3, want_ant=False)
        else:
            tick = lambda: sp.push_ragged(slots, counts, rgb, flow, want_ant=False)
        scores = tick()[0].reshape(R, CLASSES).contiguous()
        entry = {"slots": n, "rows": R}
        for lag in (64, 256):
            dp = DecodePool(CLASSES, trans, lag=lag, capacity=256, device=dev)
            for s in slots:
                dp.open(s)
            bufs = [torch.empty(R, dtype=torch.int32, device=dev), torch.empty((n, 2), dtype=torch.int32, device=dev),
                    torch.empty(R, dtype=torch.int32, device=dev)]
            decode = lambda: dp.push(slots, scores, counts=counts, labels=bufs[0], commit=bufs[1], now=bufs[2])
            row_bytes, keys = (CLASSES + 15) // 16 * 16, (CLASSES + 3) // 4 * 4 * 8
            touched = R * CLASSES * 4 + 2 * R * 4 + n * 8 + n * (2 * keys + 64) + (n * lag + R) * row_bytes + R * row_bytes
            floor_src = torch.empty(touched // 2, dtype=torch.uint8, device=dev)
            clone = lambda: floor_src.clone()
            for _ in range((lag + 40) // min(counts) + 3):          # steady state: more than `lag` frames behind every slot
                decode()
            for f in (tick, clone):
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            t = {"decode": [], "tick": [], "clone": []}
            order = [("decode", decode), ("tick", tick), ("clone", clone)]
            for r in range(a.rounds):
                rot = order[r % 3:] + order[:r % 3]                  # alternating order
                for k, (_, f) in enumerate(rot):
                    ev[2 * k].record()
                    for _ in range(a.batch):
                        f()
                    ev[2 * k + 1].record()
                torch.cuda.synchronize()
                for k, (what, _) in enumerate(rot):
                    t[what].append(ev[2 * k].elapsed_time(ev[2 * k + 1]) * 1e3 / a.batch)
            st = dp.status(slots[0])
            entry[f"lag{lag}"] = {"decode_us": stats(t["decode"]), "tick_us": stats(t["tick"]), "clone_us": stats(t["clone"]),
                                  "touched_bytes": int(touched), "frames_behind_slot0": st["frames"], "dead": st["dead"]}
        out["shapes"][name] = entry
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
