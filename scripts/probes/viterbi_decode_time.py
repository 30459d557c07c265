#!/usr/bin/env python3
"""What the Viterbi decode costs on the eval-set shape: 182 videos of the bench's seeded lengths (2.3 M frames), 86 classes,
uniform transitions (switch 2048, stay 0), seeded synthetic probabilities: the softmax of noise plus a gain on a label track with runs
of about a thousand frames, a fifth of the frames redrawn in runs of about fifty.  Figures from ONE process, the rounds interleaved:
  entry    prego_viterbi_decode alone (workspace, labels and records allocated outside), a device-event pair per call;
  clone    a device clone() of the score matrix: the memory floor (every score read once, written once);
  host     the route the entry replaces: the D2H copy of the score matrix into pinned memory (timed whole) plus the numpy model
           (prego_amd.decode.viterbi_decode) - timed on a SUBSET of the videos (--host-frames, the shortest videos first) and SCALED
           by frames to the whole set: the model is linear in the frames, the figure is labelled as scaled.
Median and p10 - p90 of each; the device labels and records of the subset are compared with the host model's once.  Prints one JSON
line; --out PATH also writes it.
    python3 scripts/probes/viterbi_decode_time.py [--rounds 20] [--host-frames 20000] [--out PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CLASSES, SWITCH, STAY = 86, 2048, 0


def runs(rng, n, mean, ids):
    lens = rng.geometric(1.0 / mean, size=max(4, 4 * n // mean + 16))
    while lens.sum() < n:
        lens = np.concatenate((lens, rng.geometric(1.0 / mean, size=lens.size)))
    return np.repeat(rng.integers(0, ids, size=lens.size), lens)[:n].astype(np.int64)


def stats(v):
    q = lambda p: sorted(v)[min(len(v) - 1, int(p * len(v)))]
    return {"median": round(q(0.5), 4), "p10": round(q(0.1), 4), "p90": round(q(0.9), 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--host-frames", type=int, default=20000)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("viterbi_decode_time: no GPU; a time is measured on the device or not at all")
    from prego_amd import _lib
    from prego_amd.decode import uniform_transitions, viterbi_decode
    from prego_amd.workloads import assembly101_eval_lengths
    lib = _lib.load()
    lens = assembly101_eval_lengths()
    V, n = len(lens), int(sum(lens))
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    rng = np.random.default_rng(0)
    track = runs(rng, n, 1000, CLASSES)
    redo = runs(rng, n, 250, 5) == 0
    track[redo] = runs(rng, n, 50, CLASSES)[redo]
    g = torch.Generator(device="cuda").manual_seed(0)
    probs = torch.randn((n, CLASSES), device="cuda", generator=g)
    probs[torch.arange(n, device="cuda"), torch.from_numpy(track).cuda()] += 4.0
    probs = torch.softmax(probs, dim=1).contiguous()
    trans_h = uniform_transitions(CLASSES, SWITCH, STAY)
    trans, offs = torch.from_numpy(trans_h).cuda(), torch.from_numpy(off).cuda()
    ws = torch.empty(lib.prego_viterbi_workspace_bytes(n, V, CLASSES), dtype=torch.uint8, device="cuda")
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    rec = torch.empty((V, 2), dtype=torch.int64, device="cuda")
    pin = torch.empty((n, CLASSES), dtype=torch.float32, pin_memory=True)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def entry():
        assert lib.prego_viterbi_decode(p(probs), CLASSES, p(offs), V, n, CLASSES, p(trans), None, p(labels), p(rec), p(ws), ws.numel(), stream) == 0

    for _ in range(2):                                           # every shape of the timed window, warm
        entry()
        probs.clone()
    torch.cuda.synchronize()
    # the subset the host model is timed on: the shortest videos up to --host-frames frames (at least one)
    order, subset, frames = np.argsort(lens, kind="stable"), [], 0
    for v in order:
        if subset and frames + lens[v] > a.host_frames:
            break
        subset.append(int(v))
        frames += lens[v]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    t_entry, t_clone, t_copy, t_model = [], [], [], []
    for r in range(a.rounds):
        first = r % 2
        for k in (first, 1 - first):                             # alternating order
            ev[2 * k].record()
            if k == 0:
                entry()
            else:
                _keep = probs.clone()
            ev[2 * k + 1].record()
        torch.cuda.synchronize()
        t_entry.append(ev[0].elapsed_time(ev[1]))
        t_clone.append(ev[2].elapsed_time(ev[3]))
        if r < 3:
            t0 = time.perf_counter()
            pin.copy_(probs, non_blocking=True)
            torch.cuda.synchronize()
            t_copy.append((time.perf_counter() - t0) * 1e3)
    host = pin.numpy()
    got_l, got_r = labels.cpu().numpy(), rec.cpu().numpy()
    t0 = time.perf_counter()
    want = [viterbi_decode(host[off[v]:off[v + 1]], trans_h) for v in subset]
    t_model.append((time.perf_counter() - t0) * 1e3)
    for v, (lab, r_) in zip(subset, want):
        assert np.array_equal(got_l[off[v]:off[v + 1]], lab) and tuple(got_r[v]) == r_, f"video {v}: the device differs from the host model"
    segs = [1 + int(np.count_nonzero(np.diff(got_l[off[v]:off[v + 1]]))) for v in range(V)]
    raw = probs.argmax(1).cpu().numpy()
    raw_segs = [1 + int(np.count_nonzero(np.diff(raw[off[v]:off[v + 1]]))) for v in range(V)]
    scaled = t_model[0] * n / frames
    out = {"probe": "viterbi_decode_time", "device": torch.cuda.get_device_name(0), "videos": V, "frames": n, "classes": CLASSES,
           "switch_cost": SWITCH, "stay_cost": STAY, "longest_video": int(max(lens)), "workspace_bytes": int(ws.numel()),
           "decoded_segments_per_video": {"median": int(np.median(segs)), "max": int(max(segs))},
           "argmax_segments_per_video": {"median": int(np.median(raw_segs)), "max": int(max(raw_segs))},
           "entry_ms": stats(t_entry), "clone_ms": stats(t_clone), "host_route_d2h_ms": stats(t_copy),
           "host_model_subset": {"videos": len(subset), "frames": int(frames), "ms": round(t_model[0], 1)},
           "host_model_scaled_to_the_set_ms": round(scaled, 0), "host_route_scaled_ms": round(scaled + stats(t_copy)["median"], 0),
           "subset_equals_host_model": True}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
