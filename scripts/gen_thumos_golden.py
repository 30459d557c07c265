"""Writes tests/golden/thumos_post.npz: a THUMOS-shaped score matrix with multi-label targets, what the REFERENCE's
`thumos_postprocessing` makes of them for the four (smooth, switch) combinations, and the reports of the reference's
`perframe_average_precision` with that post-processing.

    python scripts/gen_thumos_golden.py --reference /path/to/step_recognition/utils

The reference's postprocessing.py and metrics.py are imported by path at run time (numpy and scikit-learn only); none of their text is
copied.  Contents:

  scores [600, 22] f32   all 13 200 entries distinct (k / 16384 for distinct integers k: exact in fp32), so every column is tie-free
                         before and after `switch` (column 8 takes values of column 5) and after the removal of rows
  target [600, 22] f32   multi-label rows; column 21 ("ambiguous") is 1 on 5-10 % of the rows - the first row, the last row, runs that
                         straddle rows 127 / 128 and 255 / 256 / 257 (tile borders of the device kernel), single rows - and 0.5 on two rows,
                         which are kept (the reference removes `== 1` only)
  labels [600] i32       one class id per frame that says the same about column 21: 21 exactly where target[:, 21] == 1
  gt_out, pred_out_{s}{w}  the reference's (ground_truth, prediction) outputs, s / w = 0 / 1 for smooth / switch; gt_out is the same for
                         all four (asserted)
  ap_{s}{w} [22], mean_ap_{s}{w}       the reference's per-class AP (NaN: not reported) and mean_AP, metrics='AP', all four combinations
  cap_0{w} [22], mean_cap_0{w}         the same with metrics='cAP', smooth=False only: smoothing makes neighbouring frames share a score
                         and the reference's unstable argsort leaves tied frames to chance under cAP

The reference is asked for the classes 0 .. 20 (21 names): it scores every named column that has a nonzero target, and sklearn refuses
the 0.5 of column 21; on real THUMOS targets that column is all zero after the removal and is skipped anyway."""
import argparse
import contextlib
import importlib.util
import io
import os
import warnings
from functools import partial

import numpy as np

N, C, AMB = 600, 22, 21
HALF_ROWS = (40, 300)                                     # column 21 == 0.5: kept
AMB_RUNS = [(0, 3), (60, 61), (125, 130), (200, 201), (253, 259), (383, 386), (444, 452), (511, 513), (590, 600)]


def inputs():
    rng = np.random.default_rng(1906)
    k = rng.permutation(16384)[:N * C]
    scores = (k.astype(np.float32) / np.float32(16384)).reshape(N, C)
    target = np.zeros((N, C), np.float32)
    runs, cls = [], 0
    while sum(runs) < N:
        runs.append(int(rng.choice([1, 2, 3, 7, 11, 24, 40])))
    ids = np.concatenate([np.full(m, (0 if i % 3 == 0 else 1 + (i * 7) % 20), np.int32) for i, m in enumerate(runs)])[:N]
    target[np.arange(N), ids] = 1
    extra = rng.random(N) < 0.15                          # a second label on some rows
    target[np.arange(N)[extra], 1 + rng.integers(0, 20, N)[extra]] = 1
    labels = ids.copy()
    for a, b in AMB_RUNS:
        target[a:b] = 0
        target[a:b, AMB] = 1
        labels[a:b] = AMB
    target[AMB_RUNS[4][0], 3] = 1                         # an ambiguous row that carries a class as well
    for r in HALF_ROWS:
        target[r, AMB] = 0.5
    return scores, target, labels


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's step_recognition/utils directory")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                  "thumos_post.npz"))
    args = ap.parse_args()
    post = _load(os.path.join(args.reference, "postprocessing.py"), "reference_postprocessing")
    met = _load(os.path.join(args.reference, "metrics.py"), "reference_metrics")
    scores, target, labels = inputs()
    assert np.unique(scores).shape[0] == N * C, "equal scores"
    amb = target[:, AMB] == 1
    assert 0.05 <= amb.mean() <= 0.10, amb.mean()
    assert amb[0] and amb[-1] and amb[127] and amb[128] and amb[255] and amb[256] and amb[257]
    assert (target[:, AMB] == 0.5).sum() == 2 and np.array_equal(labels == AMB, amb)
    assert all(target[~amb][:, c].any() for c in range(1, AMB)), "a class without a kept positive"
    names = [f"c{i}" for i in range(AMB)]                 # classes 0 .. 20: see the module docstring
    out = {"scores": scores, "target": target, "labels": labels}
    for s in (0, 1):
        for w in (0, 1):
            sc, tg = scores.copy(), target.copy()         # the reference writes its argument with switch and no smooth
            gt, pr = post.thumos_postprocessing(tg, sc, smooth=bool(s), switch=bool(w))
            assert pr.dtype == np.float32 and gt.shape == ((~amb).sum(), C) and pr.shape == gt.shape
            if "gt_out" in out:
                assert np.array_equal(out["gt_out"], gt)
            out["gt_out"] = gt
            out[f"pred_out_{s}{w}"] = pr
            if not s:
                assert all(np.unique(pr[:, c]).shape[0] == pr.shape[0] for c in range(C)), "a tie after the post-processing"
            for metric in ("AP",) + (("cAP",) if not s else ()):
                with warnings.catch_warnings(), np.errstate(all="ignore"), contextlib.redirect_stdout(io.StringIO()):
                    warnings.simplefilter("ignore")
                    rep = met.perframe_average_precision(scores.copy(), target.copy(), names,
                                                         partial(post.thumos_postprocessing, smooth=bool(s), switch=bool(w)), metrics=metric)
                per = np.full(C, np.nan)
                for c in range(1, AMB):
                    per[c] = rep["per_class_AP"][names[c]]
                assert not np.isnan(per[1:AMB]).any()
                key = metric.lower()
                out[f"{key}_{s}{w}"] = per
                out[f"mean_{key}_{s}{w}"] = np.float64(rep["mean_AP"])
    np.savez_compressed(args.out, **out)
    size = os.path.getsize(args.out)
    print(args.out, size, "bytes;", int((~amb).sum()), "of", N, "rows kept")
    assert size < 150_000
    for k_ in sorted(out):
        if k_.startswith("mean_"):
            print(k_, float(out[k_]))


if __name__ == "__main__":
    main()
