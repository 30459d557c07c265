"""train_one_epoch through the REAL loader against the device-resident training set (cfg['train_cache_device'], prego_amd/train_cache.py).

Writes an Assembly101-O-shaped feature tree to a temporary directory (86 classes, --videos videos of --frames frames of 2048 fp32
values, the shipped zero-flow config) and times TRAINER["OAD"] (MiniROAD, bf16, FusedAdamW, guarded loop) in ms per step through
    loader-w<N>   build_data_loader with the shipped num_workers (capped by --max-workers)        - the parent's code path, unchanged
    loader-w0     build_data_loader with num_workers=0                                           - the same
    cached        train_cache.device_loader over the same loader
One warm-up epoch per leg, then --rounds rounds that alternate the legs; median and p10-p90 of the rounds.  Beside it the gather launch
alone (device events over --reps launches of one 16-window batch, enqueued behind a busy device) and a device clone() of the same output bytes.

    python scripts/probes/train_cache_time.py --out profiles/train_cache/train_cache_time.json"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from prego_amd import train_cache as TC  # noqa: E402
from prego_amd import weights as W  # noqa: E402
from prego_amd.config import assembly101_cfg  # noqa: E402
from prego_amd.data import build_data_loader  # noqa: E402
from prego_amd.optim import FusedAdamW  # noqa: E402
from prego_amd.registry import build_criterion, build_model, build_trainer  # noqa: E402
import prego_amd.loss, prego_amd.model, prego_amd.trainer  # noqa: E402,E401,F401

DEV = "cuda:0"


def write_tree(root, videos, frames):
    rng = np.random.default_rng(1)
    vids = [f"session{k}" for k in range(videos)]
    for sub in ("rgb_anet_resnet50", "target_perframe"):
        os.makedirs(os.path.join(root, sub))
    for k, vid in enumerate(vids):
        T = frames + 37 * k
        np.save(os.path.join(root, "rgb_anet_resnet50", vid + ".npy"), np.maximum(rng.standard_normal((T, 2048), np.float32), 0))
        tgt = np.zeros((T, 86), np.float32)
        tgt[np.arange(T), (np.arange(T) // 150 + k) % 86] = 1.0
        np.save(os.path.join(root, "target_perframe", vid + ".npy"), tgt)
    vl = os.path.join(root, "video_list.json")
    json.dump({"ASSEMBLY101-O": {"train_session_set": vids, "test_session_set": vids[:1]}}, open(vl, "w"))
    return vl


def spread(xs):
    return dict(median=float(np.median(xs)), p10=float(np.percentile(xs, 10)), p90=float(np.percentile(xs, 90)), rounds=[float(x) for x in xs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=4)
    ap.add_argument("--frames", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--max-workers", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_cache_time: needs the GPU; there is no CPU figure to report")
    root = tempfile.mkdtemp(prefix="train_cache_time_")
    try:
        vl = write_tree(root, args.videos, args.frames)
        cfg = assembly101_cfg(root_path=root, video_list_path=vl, compute_dtype="bf16", assume_zero_flow=True, exclude_videos=())
        shipped = min(cfg["num_workers"], args.max_workers)
        model = build_model(cfg, DEV)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_state_dict(cfg, 20).items()})
        crit = build_criterion(cfg, DEV)
        opt = FusedAdamW([{"params": list(model.parameters())}], lr=1e-4, weight_decay=0.05, model=model)
        train = build_trainer(cfg)
        np.random.seed(20)
        torch.manual_seed(20)
        loaders = {f"loader-w{shipped}": build_data_loader(dict(cfg, num_workers=shipped), "train"),
                   "loader-w0": build_data_loader(dict(cfg, num_workers=0), "train")}
        t0 = time.perf_counter()
        loaders["cached"] = TC.device_loader(loaders["loader-w0"], DEV, cfg, None)
        torch.cuda.synchronize()
        fill_s = time.perf_counter() - t0
        if not isinstance(loaders["cached"], TC.DeviceWindowLoader):
            raise SystemExit(f"train_cache_time: the cache disabled itself: {TC.cache_info()}")

        def epoch(name, e):
            loader = loaders[name]
            torch.cuda.synchronize()
            t = time.perf_counter()
            train(loader, model, crit, opt, None, e, DEV, None, scheduler=None)
            torch.cuda.synchronize()
            per_step = (time.perf_counter() - t) * 1e3 / len(loader)
            print(f"{name} epoch {e}: {per_step:.3f} ms per step over {len(loader)} steps", file=sys.stderr, flush=True)
            return per_step

        ms = {name: [] for name in loaders}
        for name in loaders:
            epoch(name, 0)                                   # warm-up: code objects, workspaces, the allocator's blocks
        for r in range(args.rounds):
            for name in loaders:
                ms[name].append(epoch(name, r + 1))
        model.engine(train=True).check()
        legs = {name: spread(v) for name, v in ms.items()}

        # the gather launch alone, and a clone() of the same bytes
        dl, cache = loaders["cached"], loaders["cached"].cache
        lay = cache.layout
        host_table = TC.window_table(dl.dataset, lay, 0)
        table, order = TC.epoch_table(host_table, np.random.permutation(len(host_table)))
        table_d, order_d = torch.from_numpy(table).to(DEV), torch.from_numpy(order).to(DEV)
        n = cfg["batch_size"]
        zf = torch.zeros((n, lay["window_size"], 2048), device=DEV)
        out = cache.gather(table_d, len(table), order_d, 0, n, zf)
        twin = torch.empty(out[0].numel() + out[2].numel(), device=DEV)
        out_bytes = twin.numel() * 4

        big = torch.randn(8192, 8192, device=DEV)

        def timed(fn):
            """us per call on the DEVICE: the calls are enqueued while two large matrix products keep it busy, so they run back to back
            and the events do not time the host's enqueue rate"""
            for k in range(10):
                fn(k)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            for _ in range(2):
                big @ big
            a.record()
            for k in range(args.reps):
                fn(k)
            b.record()
            b.synchronize()
            return a.elapsed_time(b) * 1e3 / args.reps       # us per call

        steps = len(order) // n
        gather_us = [timed(lambda k: cache.gather(table_d, len(table), order_d, (k % steps) * n, n, zf)) for _ in range(args.rounds)]
        clone_us = [timed(lambda k: twin.clone()) for _ in range(args.rounds)]
        res = dict(device=torch.cuda.get_device_name(0), videos=args.videos, frames=int(lay["n_rows"]), windows=len(host_table),
                   steps_per_epoch=len(dl), batch=n, window=lay["window_size"], resident_bytes=cache.bytes, fill_seconds=fill_s,
                   cpus=len(os.sched_getaffinity(0)), ms_per_step=legs,
                   gather=dict(output_bytes=out_bytes, us=spread(gather_us), clone_us=spread(clone_us),
                               ratio_to_clone=float(np.median(gather_us) / np.median(clone_us)),
                               GBps_written=float(out_bytes / np.median(gather_us) / 1e3)))
        feds = [k for k in legs if k != "cached"]
        best_fed = min(feds, key=lambda k: legs[k]["median"])
        gap = legs[best_fed]["median"] - legs["cached"]["median"]
        spreads = (legs[best_fed]["p90"] - legs[best_fed]["p10"]) + (legs["cached"]["p90"] - legs["cached"]["p10"])
        res["claim"] = dict(best_loader_leg=best_fed, gap_ms=gap, spreads_ms=spreads, cached_below_loader_by_more_than_the_spreads=bool(gap > spreads))
        text = json.dumps(res, indent=1)
        print(text)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            open(args.out, "w").write(text + "\n")
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
