"""Writes tests/golden/procedure_assembly101o.json from a checkout of the reference project's step_anticipation data:

    python scripts/gen_procedure_golden.py --reference /path/to/reference [--recogniser miniROAD]

Data only: the correct-procedure transcripts of data/context_prompt/assembly_context_prompt_train.json parsed per toy class (the 'num'
prompts), the recogniser's aggregated sequences of data/predictions/output_<recogniser>_Assembly101-O.json with the toy class of each
video (data/utils/toy2class.json), and the mistake counts `ProcedureModel.mistake_metrics` gives on them - which
tests/test_procedure_cpu.py holds against the numbers of the issue that introduced the model."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from prego_amd.procedure import ProcedureModel      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference project (holds step_anticipation/)")
    ap.add_argument("--recogniser", default="miniROAD")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "procedure_assembly101o.json"))
    a = ap.parse_args()
    data = os.path.join(a.reference, "step_anticipation", "data")
    prompts = json.load(open(os.path.join(data, "context_prompt", "assembly_context_prompt_train.json")))
    toy2class = json.load(open(os.path.join(data, "utils", "toy2class.json")))
    seqs = json.load(open(os.path.join(data, "predictions", f"output_{a.recogniser}_Assembly101-O.json")))

    group_names = list(prompts)                              # the file's order: group id = position
    transcripts = []
    for g, name in enumerate(group_names):
        transcripts += [{"group": g, "symbols": s} for s in ProcedureModel.parse_context_prompt(prompts[name]["num"])]
    sequences = []
    for video, v in seqs.items():
        toy = video.split("-")[2].split("_")[0]
        sequences.append({"video": video, "group": group_names.index(toy2class[toy]), "pred": [int(x) for x in v["pred"]],
                          "gt": [int(x) for x in v["gt"]]})
    n_classes = 1 + max(max(t["symbols"]) for t in transcripts)
    n_classes = max(n_classes, 1 + max(max(s["pred"] + s["gt"]) for s in sequences))

    expected = []
    for order, targets in ((1, "all"), (2, "all"), (1, "last")):
        m = ProcedureModel(n_classes, order=order, threshold=(0, 1), targets=targets)
        for t in transcripts:
            m.add(t["symbols"], t["group"])
        for which in ("gt", "pred"):
            r = m.mistake_metrics([s[which] for s in sequences], [s["group"] for s in sequences])
            expected.append({"order": order, "targets": targets, "sequences": which, **{k: r[k] for k in ("tp", "fp", "fn", "tn", "unknown")}})
    out = {"dataset": "Assembly101-O", "recogniser": a.recogniser, "n_classes": n_classes, "group_names": group_names,
           "n_symbols": sum(len(t["symbols"]) for t in transcripts), "transcripts": transcripts, "sequences": sequences, "expected": expected}
    with open(a.out, "w") as fp:
        json.dump(out, fp, separators=(",", ":"))
        fp.write("\n")
    for e in expected:
        print(e)
    print(f"{a.out}: {len(transcripts)} transcripts, {out['n_symbols']} symbols, {len(group_names)} groups, {len(sequences)} sequences, "
          f"{n_classes} classes, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
