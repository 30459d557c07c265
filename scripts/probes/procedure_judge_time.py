#!/usr/bin/env python3
"""What judging costs behind the drain: a pool of 1024 slots, vote window 1 and a new step id in every slot at every tick, so
1024 entries are due per drain.  Two consumers sit on the same pool and see the same events: a plain `EventFeed` (drain + report copy) and
a `MistakeMonitor` (drain + judge + both copies).  Each tick times both with a device-event pair, in alternating order; the ids are voted
outside the timed part.  Legs: the Assembly101-O corpus of tests/golden/procedure_assembly101o.json (970 examples in 15 groups; 1105
symbols with the STARTs), a synthetic corpus of 65 536 examples in 16 groups, and the same with every slot at group -1 (each entry scans
all 65 536 examples).  Prints one JSON line; --out PATH also writes it.
    python3 scripts/probes/procedure_judge_time.py [--ticks 200] [--out PATH]"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CAP, WARM = 1024, 20


def golden_model(order):
    from prego_amd.procedure import ProcedureModel
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "procedure_assembly101o.json")))
    m = ProcedureModel(g["n_classes"], order=order)
    for t in g["transcripts"]:
        m.add(t["symbols"], t["group"])
    return m


def synthetic_model(order, n_examples=65536, n_groups=16, ncls=86):
    from prego_amd.procedure import ProcedureModel
    rng = random.Random(7)
    m = ProcedureModel(ncls, order=order)
    for g in range(n_groups):
        base = [rng.randrange(ncls) for _ in range(16)]
        left = n_examples // n_groups
        while left > 0:
            t = [s if rng.random() < 0.85 else rng.randrange(ncls) for s in base][:left]
            m.add(t, g)
            left -= len(t)
    return m


def walks(model, groups):
    """per slot a transcript of its group to walk along (cyclically), with no step repeated in a row: every vote is an event"""
    by_group = {}
    for g, seq, _ in model.transcripts:
        s = [v for i, v in enumerate(seq) if i == 0 or v != seq[i - 1]]
        if len(s) >= 3 and s[0] != s[-1]:
            by_group.setdefault(g, []).append(s)
    every = [s for v in by_group.values() for s in v]
    return [(by_group.get(g) or every)[k % len(by_group.get(g) or every)] for k, g in enumerate(groups)]


def leg(torch, net, name, model, groups, ticks):
    pool = net.stream_pool(capacity=CAP, window=1, max_events=1024)
    slots = [pool.open() for _ in range(CAP)]
    feed, mon = pool.event_feed(max_out=CAP), pool.mistake_monitor(model, max_out=CAP)
    mon.set_group(slots, groups)
    walk = walks(model, [g if g >= 0 else k % max(model.n_groups, 1) for k, g in enumerate(groups)])
    ids = [torch.tensor([w[t % len(w)] for w in walk], dtype=torch.int32, device="cuda:0") for t in range(WARM + ticks)]
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(2)]
    us, counts, mistakes, unknown = ([], []), [], 0, 0
    for t in range(WARM + ticks):
        for a in range(0, CAP, 256):
            pool.vote(slots[a:a + 256], ids[t][a:a + 256].contiguous())
        tickets = [None, None]
        for k in ((0, 1) if t % 2 == 0 else (1, 0)):
            ev[k][0].record()
            tickets[k] = feed.drain() if k == 0 else mon.drain()
            ev[k][1].record()
        torch.cuda.synchronize()
        plain, judged = tickets[0].events(), tickets[1].events()
        assert plain == judged, "the two feeds disagree"
        if t >= WARM:
            for k in (0, 1):
                us[k].append(ev[k][0].elapsed_time(ev[k][1]) * 1e3)
            counts.append(len(judged))
            vs = tickets[1].verdicts()
            mistakes += sum(v.mistake for v in vs)
            unknown += sum(v.unknown for v in vs)
    q = lambda v, p: sorted(v)[min(len(v) - 1, int(p * len(v)))]
    row = {"leg": name, "examples": model.n_examples, "groups": model.n_groups, "order": model.order, "ticks": ticks,
           "entries_per_drain": sum(counts) / len(counts), "mistake_share": mistakes / max(1, sum(counts)), "unknown_share": unknown / max(1, sum(counts))}
    for k, what in ((0, "drain_us"), (1, "drain_judge_us")):
        row[what] = {"median": round(q(us[k], 0.5), 1), "p10": round(q(us[k], 0.1), 1), "p90": round(q(us[k], 0.9), 1)}
    row["judge_added_us"] = round(row["drain_judge_us"]["median"] - row["drain_us"]["median"], 1)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--order", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("procedure_judge_time: no GPU; a time is measured on the device or not at all")
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
    out = {"probe": "procedure_judge_time", "device": torch.cuda.get_device_name(0), "capacity": CAP, "max_out": CAP, "rows": rows}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fp:
            fp.write(line + "\n")


if __name__ == "__main__":
    main()
