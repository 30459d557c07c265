"""Writes tests/golden/segmental_epic_tent.json: the segmental records (correct | frames | m | n | dist | tp@1/10 | tp@1/4 | tp@1/2) of
the fifteen Epic-tent-O videos of tests/golden/g8_output_miniROAD.json.gz, on the raw per-frame argmax ("frames") and on the 200-frame
vote expanded back to frames ("vote"), computed with the host model (prego_amd/segmental.py; no background class, overlaps 1/10, 1/4,
1/2).  tests/test_segmental_cpu.py holds the host model to it, tests/test_gpu_segmental.py the kernel.

    python scripts/gen_segmental_golden.py [--print]      # --print: also the table of DESIGN section 9"""
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from prego_amd.segmental import segmental_records, segmental_report, segmental_scores, voted_frames      # noqa: E402

WINDOW = 200


def main():
    golden = os.path.join(ROOT, "tests", "golden")
    g = json.load(gzip.open(os.path.join(golden, "g8_output_miniROAD.json.gz")))
    pred = [np.asarray(v["pred"]) for v in g.values()]
    gt = [np.asarray(v["gt"]) for v in g.values()]
    frames = segmental_records(pred, gt)
    vote = segmental_records([voted_frames(p, WINDOW) for p in pred], gt)
    out = {"source": "tests/golden/g8_output_miniROAD.json.gz", "window": WINDOW, "bg": [], "overlaps": [[1, 10], [1, 4], [1, 2]],
           "fields": ["correct", "frames", "m", "n", "dist", "tp_0", "tp_1", "tp_2"], "videos": list(g.keys()),
           "frames": frames.tolist(), "vote": vote.tolist()}
    with open(os.path.join(golden, "segmental_epic_tent.json"), "w") as f:
        json.dump(out, f, indent=1)
    if "--print" in sys.argv:
        for name, rec in (("frames", frames), ("vote", vote)):
            rep = segmental_report(rec)
            print(name, {k: round(v, 2) for k, v in rep.items() if k not in ("per_video", "videos")})
            for vid, r, pv in zip(g.keys(), rec, rep["per_video"]):
                print(f"  {vid:16} {r.tolist()} Edit {pv['Edit']:.1f}")
        d = json.load(open(os.path.join(golden, "procedure_assembly101o.json")))
        rep = segmental_scores([s["pred"] for s in d["sequences"]], [s["gt"] for s in d["sequences"]], transcripts=True)
        dist = sum(v["dist"] for v in rep["per_video"])
        print(f"Assembly101-O transcripts: {rep['videos']} sequences, Edit {rep['Edit']:.2f}, total distance {dist}, "
              f"pred symbols {sum(v['m'] for v in rep['per_video'])}, gt symbols {sum(v['n'] for v in rep['per_video'])}")


if __name__ == "__main__":
    main()
