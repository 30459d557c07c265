#!/usr/bin/env python3
"""What the segmental metrics cost on the eval-set shape: 182 videos, 2.3 M frames, seeded synthetic labels whose run lengths
resemble tests/golden/g8_output_miniROAD.json.gz (gt runs of about a thousand frames, pred = gt with stretches redrawn in runs of about
fifty: some hundred pred segments against a dozen gt segments per video).  Three figures from ONE process, the rounds interleaved:
  entry    prego_segmental_scores alone (workspace and records allocated outside), a device-event pair per call;
  clone    a device clone() of the two label vectors: the memory floor (every frame read once, written once);
  host     the route the entry replaces: the D2H copy of both vectors into pinned memory plus the host model
           (prego_amd.segmental.segmental_records), host clock around work that ends in a synchronise.
Median and p10 - p90 of each; the device records are compared with the host model's once.  Prints one JSON line; --out PATH also writes it.
    python3 scripts/probes/segmental_time.py [--rounds 30] [--host-rounds 3] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

VIDEOS, FRAMES, CLASSES = 182, 2_300_000, 86


def runs(rng, n, mean, ids):
    lens = rng.geometric(1.0 / mean, size=max(4, 4 * n // mean + 16))
    while lens.sum() < n:
        lens = np.concatenate((lens, rng.geometric(1.0 / mean, size=lens.size)))
    return np.repeat(rng.integers(0, ids, size=lens.size), lens)[:n].astype(np.int32)


def eval_set(seed=0):
    rng = np.random.default_rng(seed)
    cut = np.sort(rng.choice(np.arange(1, FRAMES), size=VIDEOS - 1, replace=False))
    lens = np.diff(np.concatenate(([0], cut, [FRAMES])))
    P, G = [], []
    for n in lens:
        g = runs(rng, int(n), 1000, CLASSES)
        p = g.copy()
        redo = runs(rng, int(n), 300, 2).astype(bool)
        noise = runs(rng, int(n), 50, CLASSES)
        p[redo] = noise[redo]
        P.append(p)
        G.append(g)
    return P, G


def stats(v):
    q = lambda p: sorted(v)[min(len(v) - 1, int(p * len(v)))]
    return {"median": round(q(0.5), 4), "p10": round(q(0.1), 4), "p90": round(q(0.9), 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--host-rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("segmental_time: no GPU; a time is measured on the device or not at all")
    from prego_amd import _lib
    from prego_amd.segmental import segmental_records
    lib = _lib.load()
    P, G = eval_set()
    off = np.concatenate(([0], np.cumsum([len(p) for p in P]))).astype(np.int32)
    pred, gt, offs = (torch.from_numpy(x).cuda() for x in (np.concatenate(P), np.concatenate(G), off))
    n = pred.numel()
    ws = torch.empty(lib.prego_segmental_workspace_bytes(n, VIDEOS), dtype=torch.uint8, device="cuda")
    rec = torch.empty((VIDEOS, 8), dtype=torch.int32, device="cuda")
    pin = torch.empty((2, n), dtype=torch.int32, pin_memory=True)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def entry():
        assert lib.prego_segmental_scores(p(pred), p(gt), p(offs), VIDEOS, n, None, None, None, p(rec), p(ws), ws.numel(), stream) == 0

    def host_route():
        pin[0].copy_(pred, non_blocking=True)
        pin[1].copy_(gt, non_blocking=True)
        torch.cuda.synchronize()
        hp, hg = pin[0].numpy(), pin[1].numpy()
        return segmental_records(np.split(hp, off[1:-1]), np.split(hg, off[1:-1]))

    for _ in range(3):                                           # every shape of the timed window, warm
        entry()
        pred.clone(), gt.clone()
    torch.cuda.synchronize()
    want = host_route()
    assert np.array_equal(rec.cpu().numpy(), want), "the device records differ from the host model's"
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t_entry, t_clone, t_host, t_copy = [], [], [], []
    for r in range(a.rounds):
        first = r % 2
        for k in (first, 1 - first):                             # alternating order
            ev[2 * k].record()
            if k == 0:
                entry()
            else:
                _keep = (pred.clone(), gt.clone())
            ev[2 * k + 1].record()
        torch.cuda.synchronize()
        t_entry.append(ev[0].elapsed_time(ev[1]))
        t_clone.append(ev[2].elapsed_time(ev[3]))
        if r < a.host_rounds:
            t0 = time.perf_counter()
            pin[0].copy_(pred, non_blocking=True)
            pin[1].copy_(gt, non_blocking=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            segmental_records(np.split(pin[0].numpy(), off[1:-1]), np.split(pin[1].numpy(), off[1:-1]))
            t_copy.append((t1 - t0) * 1e3)
            t_host.append((time.perf_counter() - t0) * 1e3)
    segs = want[:, 2:4]
    out = {"probe": "segmental_time", "device": torch.cuda.get_device_name(0), "videos": VIDEOS, "frames": n,
           "pred_segments_per_video": {"min": int(segs[:, 0].min()), "median": int(np.median(segs[:, 0])), "max": int(segs[:, 0].max())},
           "gt_segments_per_video": {"min": int(segs[:, 1].min()), "median": int(np.median(segs[:, 1])), "max": int(segs[:, 1].max())},
           "longest_video": int(np.diff(off).max()), "workspace_bytes": int(ws.numel()),
           "entry_ms": stats(t_entry), "clone_ms": stats(t_clone), "host_route_ms": stats(t_host), "host_route_d2h_ms": stats(t_copy),
           "entry_beats_host_route": stats(t_entry)["median"] < stats(t_host)["median"], "records_equal_host_model": True}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
