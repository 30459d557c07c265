"""From a rocprofv3 --kernel-trace CSV of scripts/probes/ant_step_profile.py: the last 200 frames of MROADA.step as the device saw them.
Per kernel of a frame (in launch order): median duration and median gap to the previous kernel's end; per frame: median span from the
first kernel's start to the last kernel's end, and the same for the trunk alone (up to stream_gates_head) - one JSON line.
usage: python scripts/probes/ant_step_frames.py <trace dir> [label]"""
import csv, glob, json, sys
import numpy as np
f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
rows = [r for r in rows if "stream_" in r["Kernel_Name"] or "ln_relu_rows" in r["Kernel_Name"]]
ends = [i for i, r in enumerate(rows) if "stream_ant_head" in r["Kernel_Name"]]
K = ends[-1] - ends[-2]                                       # kernels per frame
fr = [rows[e - K + 1:e + 1] for e in ends[-200:]]
assert all(len(x) == K and [r["Kernel_Name"] for r in x] == [r["Kernel_Name"] for r in fr[0]] for x in fr)
S = np.array([[int(r["Start_Timestamp"]) for r in x] for x in fr], dtype=np.int64)
E = np.array([[int(r["End_Timestamp"]) for r in x] for x in fr], dtype=np.int64)
names = [r["Kernel_Name"].split("(")[0].replace("void ", "")[:48] for r in fr[0]]
gh = max(i for i, nm in enumerate(names) if "stream_gates_head" in nm)
us = lambda a: round(float(np.median(a)) / 1e3, 2)
print(json.dumps({"label": sys.argv[2] if len(sys.argv) > 2 else "", "frames": len(fr),
                  "kernels": [{"name": names[i], "us": us(E[:, i] - S[:, i]), "gap_before_us": us(S[:, i] - E[:, i - 1]) if i else None}
                              for i in range(K)],
                  "frame_span_us": us(E[:, -1] - S[:, 0]), "trunk_span_us": us(E[:, gh] - S[:, 0]),
                  "ant_span_us": us(E[:, -1] - E[:, gh]), "frame_period_us": us(S[1:, 0] - S[:-1, 0])}))
