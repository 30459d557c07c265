"""The snapshot / restore legs both pool benches share (`anticipation_bench.py --step --pool --snapshot`,
`vit_stream_bench.py --snapshot`).  For n scattered open slots of pool A and n open slots of a second pool B:
(s)  `pool_a.snapshot(slots)`: one launch, the images tensor allocated by the call.
(r)  `pool_b.restore(snap, slots=...)`: one launch, then the status copy the method waits for - that wait is in the caller's call.
(rc) the C restore alone (`prego_*_stream_pool_restore`, status written, not read): what (r) costs on the device.
(t)  the only read route there was before: per slot `state(slot)` (GRU pool) or `window(slot)` (Transformer pool) plus the blocking
     record copy `events` / `close` make.
Protocol of sections 13e / 13h: warm-up calls per route, alternating rounds, a device-event pair per call; median and p10 - p90 in us.
`floor_us`: image bytes each way (n images read + n images written) at the ~6.3 TB/s achievable HBM rate section 13c uses."""
import ctypes as C

import numpy as np
import torch

HBM_BYTES_PER_US = 6.3e6          # ~6.3 TB/s


def _measure(paths, calls, warmup, rounds):
    times = {k: [] for k in paths}
    for f in paths.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, f in paths.items():
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(2 * calls)]
            for i in range(calls):
                evs[2 * i].record()
                f()
                evs[2 * i + 1].record()
            torch.cuda.synchronize()
            times[k] += [evs[2 * i].elapsed_time(evs[2 * i + 1]) * 1e3 for i in range(calls)]
    return {k: {"median_us": float(np.median(v)), "p10_us": float(np.percentile(v, 10)), "p90_us": float(np.percentile(v, 90))}
            for k, v in times.items()}


def snapshot_legs(pool_a, pool_b, slots_a, slots_b, read_slot, calls, warmup, rounds):
    """one cell: the four legs for the open slots `slots_a` of pool_a (which hold streams) and the open slots `slots_b` of pool_b;
    read_slot(pool, slot) is the state / window read of route (t)"""
    n = len(slots_a)
    snap = pool_a.snapshot(slots_a)
    nb = snap.images.shape[1]
    status = torch.empty((n,), dtype=torch.int32, device=pool_b.device)
    arr_b = pool_b._slot_array(slots_b)
    c_restore = getattr(pool_b.lib, pool_b._C["restore"])

    def fs():
        pool_a.snapshot(slots_a)

    def fr():
        pool_b.restore(snap, slots=slots_b)

    def frc():
        with torch.cuda.device(pool_b.device):
            pool_b._check(c_restore(pool_b.p, None, n, arr_b, C.c_void_p(snap.images.data_ptr()), n * nb, C.c_void_p(status.data_ptr()),
                                    C.c_void_p(pool_b._stream_ptr(pool_b.device))))

    def ft():
        for s in slots_a:
            read_slot(pool_a, s)
            pool_a._record(s)
    t = _measure({"s": fs, "r": fr, "rc": frc, "t": ft}, calls, warmup, rounds)
    t["image_bytes"] = int(nb)
    t["floor_us"] = 2.0 * n * nb / HBM_BYTES_PER_US
    for k in ("s", "rc", "r"):
        t[f"{k}_over_floor"] = t[k]["median_us"] / t["floor_us"]
    spreads = (t["s"]["p90_us"] - t["s"]["p10_us"]) + (t["t"]["p90_us"] - t["t"]["p10_us"])
    t["t_minus_s_us"] = t["t"]["median_us"] - t["s"]["median_us"]
    t["s_below_t_by_more_than_the_spreads"] = t["t_minus_s_us"] > spreads
    return t
