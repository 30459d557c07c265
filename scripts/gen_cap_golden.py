"""Writes tests/golden/cap_mixed.npz: a small labelled score matrix and the calibrated average precision (cAP) the REFERENCE computes
on it, per class and per (stage, class).

    python scripts/gen_cap_golden.py --reference /path/to/step_recognition/utils/metrics.py

The reference's file is imported by path (it needs numpy and scikit-learn only).  `calibrated_average_precision_score` is called on
every column of the one-hot form of the labels -> `cap` [classes]; `perstage_average_precision(..., None, metrics='cAP')` never
scores class 0, so it is called a second time on the columns rotated by one -> `stage_cap` [10, classes].  The class that never occurs
is 0 / 0 = NaN in both (numpy warns; the warnings are silenced here).

The reference sorts with numpy's default unstable argsort, so with equal scores its answer is undefined: every column here is
tie-free, and the script asserts it.  The 2400 frames x 8 classes hold: a class that never occurs (6); runs of 1 and 2 frames; a run
of 91 frames (len 90) that starts at frame 0; a run that ends at the last frame; frames with id -1 (negatives of every class);
neighbouring runs of different classes; column 3 holds negative scores too."""
import argparse
import importlib.util
import os
import warnings

import numpy as np

N_CLASSES = 8
ABSENT = 6
N_FRAMES = 2400


def inputs():
    rng = np.random.default_rng(2210)
    runs = [(1, 91), (0, 20), (2, 1), (0, 3), (2, 2), (-1, 15), (3, 171), (7, 1), (5, 1)]
    classes = [c for c in range(N_CLASSES) if c != ABSENT] + [-1]
    while sum(m for _, m in runs) < N_FRAMES:
        c = classes[int(rng.integers(0, len(classes)))]
        if runs[-1][0] == c:                                                  # neighbours of one class would be one run
            continue
        runs.append((c, int(rng.choice([1, 1, 2, 3, 7, 10, 11, 24, 57, 90, 140]))))
    labels = np.concatenate([np.full(m, c, np.int32) for c, m in runs])[:N_FRAMES]
    labels[-5:] = 4                                                           # a run that ends at the last frame
    n = labels.shape[0]
    scores = rng.random((n, N_CLASSES)).astype(np.float32)
    scores[np.arange(n)[labels >= 0], labels[labels >= 0]] += 0.25            # a detector that is right more often than not
    scores[:, 3] = (scores[:, 3] - 0.5) * 30                                  # negative scores too
    for c in range(N_CLASSES):                                                # tie-free columns: redraw what collides
        while True:
            _, first, counts = np.unique(scores[:, c], return_index=True, return_counts=True)
            if counts.max() == 1:
                break
            dup = np.setdiff1d(np.arange(n), first)
            scores[dup, c] = rng.random(dup.shape[0]).astype(np.float32)
    return scores, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="path of the reference's step_recognition/utils/metrics.py")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                  "cap_mixed.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_metrics", args.reference)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    scores, labels = inputs()
    n = labels.shape[0]
    for c in range(N_CLASSES):                                                # with ties the reference's answer is undefined
        assert np.unique(scores[:, c]).shape[0] == n, f"column {c} has equal scores"
    assert not (labels == ABSENT).any() and all((labels == c).any() for c in range(N_CLASSES) if c != ABSENT)
    onehot = np.zeros((n, N_CLASSES), np.float32)
    onehot[np.arange(n)[labels >= 0], labels[labels >= 0]] = 1
    names = [f"c{i}" for i in range(N_CLASSES)]
    stage_cap = np.full((10, N_CLASSES), np.nan)
    stage_mean = np.zeros(10)
    import contextlib
    import io
    with warnings.catch_warnings(), np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")                                       # 0 / 0 of the class that never occurs
        cap = np.array([ref.calibrated_average_precision_score(onehot[:, c], scores[:, c]) for c in range(N_CLASSES)])
        frame = ref.perframe_average_precision(scores, onehot, names, None, metrics="cAP")
        res = ref.perstage_average_precision(scores, onehot, names, None, metrics="cAP")
        rot = ref.perstage_average_precision(np.roll(scores, 1, axis=1), np.roll(onehot, 1, axis=1), names[-1:] + names[:-1], None,
                                             metrics="cAP")
    stages = list(res)
    for s, stage in enumerate(stages):
        for c in range(1, N_CLASSES):
            stage_cap[s, c] = res[stage]["per_class_AP"][names[c]]
        stage_cap[s, 0] = rot[stage]["per_class_AP"][names[0]]
        stage_mean[s] = res[stage]["mean_AP"]
    assert np.isnan(cap[ABSENT]) and not np.isnan(np.delete(cap, ABSENT)).any()
    assert np.isnan(stage_cap[:, ABSENT]).all() and not np.isnan(np.delete(stage_cap, ABSENT, axis=1)).any()
    np.savez_compressed(args.out, scores=scores, labels=labels, cap=cap, mean_cap=np.float64(frame["mean_AP"]), stage_cap=stage_cap,
                        stage_mean_cap=stage_mean, stage_names=np.array(stages))
    size = os.path.getsize(args.out)
    print(args.out, size, "bytes")
    assert size < 100_000
    print(np.round(cap, 4))
    print(np.round(stage_cap, 4))


if __name__ == "__main__":
    main()
