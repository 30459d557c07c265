#!/usr/bin/env python3
"""What forecasting costs behind the drain, in the setup of procedure_judge_time.py: a pool of 1024 slots, vote
window 1 and a new step id in every slot at every tick, so 1024 entries are due per drain.  Two consumers sit on the same pool and see the
same events: a `MistakeMonitor` (drain + judge + both copies) and a `ForecastMonitor` (drain + judge + forecast + three copies).  Each tick
times both drains with a device-event pair, in alternating order, and then `forecast_slots` over all 1024 slots (one launch, two copies);
the ids are voted outside the timed part.  Legs as in procedure_judge_time.py: the Assembly101-O corpus, a synthetic corpus of 65 536
examples in 16 groups, and the same with every slot at group -1.  Prints one JSON line; --out PATH also writes it.
    python3 scripts/probes/procedure_forecast_time.py [--ticks 200] [--out PATH]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from procedure_judge_time import CAP, WARM, golden_model, synthetic_model, walks      # noqa: E402  the same corpora and walks


def leg(torch, net, name, model, groups, ticks):
    pool = net.stream_pool(capacity=CAP, window=1, max_events=1024)
    slots = [pool.open() for _ in range(CAP)]
    plain = pool.mistake_monitor(model, max_out=CAP)
    mon = pool.forecast_monitor(plain.model, max_out=CAP)
    for m in (plain, mon):
        m.set_group(slots, groups)
    walk = walks(model, [g if g >= 0 else k % max(model.n_groups, 1) for k, g in enumerate(groups)])
    ids = [torch.tensor([w[t % len(w)] for w in walk], dtype=torch.int32, device="cuda:0") for t in range(WARM + ticks)]
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(3)]
    us, counts, hit, unknown = ([], [], []), [], 0, 0
    for t in range(WARM + ticks):
        for a in range(0, CAP, 256):
            pool.vote(slots[a:a + 256], ids[t][a:a + 256].contiguous())
        tickets = [None, None, None]
        for k in ((0, 1) if t % 2 == 0 else (1, 0)):
            ev[k][0].record()
            tickets[k] = plain.drain() if k == 0 else mon.drain()
            ev[k][1].record()
        ev[2][0].record()
        tickets[2] = mon.forecast_slots(slots)
        ev[2][1].record()
        torch.cuda.synchronize()
        judged, forecast = tickets[0].events(), tickets[1].events()
        assert judged == forecast, "the two monitors disagree on the events"
        assert [v.words() for v in tickets[0].verdicts()] == [v.words() for v in tickets[1].verdicts()], "the two monitors disagree on the verdicts"
        fs, by_slot = tickets[1].forecasts(), tickets[2].forecasts()
        assert [f.words() for f in fs] == [by_slot[e[0]].words() for e in forecast], "forecast_slots disagrees with the drain's forecasts"
        if t >= WARM:
            for k in (0, 1, 2):
                us[k].append(ev[k][0].elapsed_time(ev[k][1]) * 1e3)
            counts.append(len(forecast))
            unknown += sum(f.unknown for f in fs)
            nxt = ids[t + 1].tolist() if t + 1 < WARM + ticks else None
            hit += sum(nxt[e[0]] in f.ids[:1] for e, f in zip(forecast, fs)) if nxt else 0
    q = lambda v, p: sorted(v)[min(len(v) - 1, int(p * len(v)))]
    row = {"leg": name, "examples": model.n_examples, "groups": model.n_groups, "order": model.order, "ticks": ticks,
           "entries_per_drain": sum(counts) / len(counts), "unknown_share": unknown / max(1, sum(counts)),
           "top1_share_of_the_walk": hit / max(1, sum(counts[:-1]))}
    for k, what in ((0, "drain_judge_us"), (1, "drain_judge_forecast_us"), (2, "forecast_slots_us")):
        row[what] = {"median": round(q(us[k], 0.5), 1), "p10": round(q(us[k], 0.1), 1), "p90": round(q(us[k], 0.9), 1)}
    row["forecast_added_us"] = round(row["drain_judge_forecast_us"]["median"] - row["drain_judge_us"]["median"], 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("procedure_forecast_time: no GPU; a time is measured on the device or not at all")
    from prego_amd import weights as W
    from prego_amd.config import assembly101_cfg
    from prego_amd.registry import build_model
    import prego_amd.model  # noqa: F401
    cfg = assembly101_cfg(compute_dtype="bf16")
    net = build_model(cfg, "cuda:0")
    net.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_state_dict(cfg, 20).items()})
    net.eval()
    gold, synth = golden_model(a.order), synthetic_model(a.order)
    rows = [leg(torch, net, "assembly101o", gold, [s % gold.n_groups for s in range(CAP)], a.ticks),
            leg(torch, net, "synthetic 65536, a group per slot", synth, [s % synth.n_groups for s in range(CAP)], a.ticks),
            leg(torch, net, "synthetic 65536, every group", synth, [-1] * CAP, a.ticks)]
    out = {"probe": "procedure_forecast_time", "device": torch.cuda.get_device_name(0), "capacity": CAP, "max_out": CAP, "rows": rows}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
