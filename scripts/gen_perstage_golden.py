"""Writes tests/golden/perstage_ap_mixed.npz: a small labelled score matrix and the per-stage AP the REFERENCE computes on it.

    python scripts/gen_perstage_golden.py --reference /path/to/step_recognition/utils/metrics.py

The reference's file is imported by path (it needs numpy and scikit-learn only) and `perstage_average_precision(..., None,
metrics='AP')` is called on the one-hot form of the labels.  It never scores class 0, so it is called a second time on the columns
rotated by one, which yields the reference's own figure for column 0 as well: `ap` is the full [10, classes] table.  The recorded
0.0 of the class that never occurs is what scikit-learn 1.7 answers for a set without positives (other versions differ; the tests
read the fixture, not scikit-learn, for that class).

The 600 frames x 6 classes hold: a class that never occurs (5); runs of 1 and 2 frames; a run of 91 frames (len 90: stage 7 starts
at offset 62, not 63) that starts at frame 0; a run of 171 frames; a run that ends at the last frame; frames with id -1 (negatives
of every class); neighbouring runs of different classes; column 2 quantised to eighths, column 4 constant, column 3 of +-0.0."""
import argparse
import importlib.util
import os
import warnings

import numpy as np

RUNS = [(1, 91), (0, 20), (2, 1), (0, 3), (2, 2), (-1, 15), (3, 171), (0, 30), (4, 40), (1, 1), (2, 57), (-1, 9), (4, 2), (3, 1),
        (0, 60), (1, 33), (4, 25), (2, 39)]
N_CLASSES = 6


def inputs():
    labels = np.concatenate([np.full(m, c, np.int32) for c, m in RUNS])
    n = labels.shape[0]
    assert n == 600
    rng = np.random.default_rng(1808)
    scores = rng.random((n, N_CLASSES)).astype(np.float32)
    scores[np.arange(n)[labels >= 0], labels[labels >= 0]] += 0.25            # a detector that is right more often than not
    scores[:, 2] = np.round(scores[:, 2] * 8) / 8                             # heavy ties
    scores[:, 4] = 0.5                                                        # one threshold
    scores[:, 3] = np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(np.float32)
    return scores, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="path of the reference's step_recognition/utils/metrics.py")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                  "perstage_ap_mixed.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_metrics", args.reference)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    scores, labels = inputs()
    n = labels.shape[0]
    onehot = np.zeros((n, N_CLASSES), np.float32)
    onehot[np.arange(n)[labels >= 0], labels[labels >= 0]] = 1
    names = [f"c{i}" for i in range(N_CLASSES)]
    table = np.full((10, N_CLASSES), np.nan)
    mean = np.zeros(10)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                       # scikit-learn: "no positive class found"
        res = ref.perstage_average_precision(scores, onehot, names, None, metrics="AP")
        rot = ref.perstage_average_precision(np.roll(scores, 1, axis=1), np.roll(onehot, 1, axis=1), names[-1:] + names[:-1], None,
                                             metrics="AP")
    stages = list(res)
    for s, stage in enumerate(stages):
        for c in range(1, N_CLASSES):
            table[s, c] = res[stage]["per_class_AP"][names[c]]
        table[s, 0] = rot[stage]["per_class_AP"][names[0]]
        mean[s] = res[stage]["mean_AP"]
    assert not np.isnan(table).any()
    np.savez(args.out, scores=scores, labels=labels, ap=table, mean_ap=mean, stage_names=np.array(stages))
    print(args.out, os.path.getsize(args.out), "bytes")
    print(np.round(table, 4))


if __name__ == "__main__":
    main()
