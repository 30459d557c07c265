"""Per-frame average precision, the metric behind `metric: 'AP'` of both shipped configs (the reference computes it in
step_recognition/utils/metrics.py:25-62 with one sklearn call per class), SURVEY.md section 8 row f3.

The definition is sklearn's `average_precision_score`: per class, thresholds at the DISTINCT score values in descending order
(ties share a threshold), AP = sum_k (R_k - R_{k-1}) P_k; classes without a positive are skipped and so is class 0, which the
reference always treats as background (metrics.py:44-48).  Two routes to the same numbers:

  * `perframe_average_precision`         - numpy on the host, all classes at once (one argsort of the score matrix); the CPU
                                           tests hold it to sklearn.
  * `perframe_average_precision_device`  - the HIP path: `prego_perframe_ap` / `prego_perframe_ap_labels` (csrc/metrics.hip: the
                                           positives of every class sorted, every score counted against them), used by `Evaluate`
                                           so that the [frames x classes] score matrix of an eval pass never leaves the device.
                                           No CPU fallback.

`metric: 'cAP'` (the reference's calibrated variant for TVSeries, metrics.py:10-22) has the same two routes:
`calibrated_average_precision_columns` on the host and `perframe_average_precision_device(..., metrics='cAP')`
(`prego_perframe_cap` / `prego_perframe_cap_labels`) on the device.  Both rank frames of equal score in frame order (the reference's
unstable argsort leaves ties to chance), so they agree up to the order of one fp64 sum.

Per-stage average precision (the reference's `perstage_average_precision`, metrics.py:64-130, from LSTR):
how early inside an action it is recognised.  Per class the action instances are the maximal runs of positive frames over the whole
concatenated axis; a run with first frame a and last frame b has len = b - a and its stage s = 0..9 holds the frames
[a + int(len * (s / 10)), max(that + 1, a + int(len * ((s + 1) / 10)))) - float products, so len 90, s 7 starts at offset 62; a
one-frame run is in all ten stages and the last frame of a longer run in none.  The sample set of (class, stage) is every negative
frame of the class plus the stage's frames of every run; its AP is the one above.  A class without a run scores 0.0 (what sklearn
1.7 answers for a set without positives) and counts in the stage's mean over the classes 1.. .  Two routes again:

  * `perstage_average_precision`         - numpy on the host; metrics 'AP' or 'cAP' (cAP: ties in input order, NaN without
                                           positives, as `calibrated_average_precision_columns` documents); dense targets or ids.
  * `perstage_average_precision_device`  - the HIP path, `prego_perstage_ap_labels` (csrc/metrics.hip): runs and stage masks from
                                           one class id per frame, the per-frame pipeline's ranks, one counter per (stage, positive).
                                           'AP' or 'cAP' (`prego_perstage_cap_labels`: ties in frame order, NaN without a
                                           member, as the host form), no CPU fallback; used by `Evaluate` under cfg
                                           `eval_perstage` (`eval_perstage_metric`).

`postprocessing`: the host functions take any callable (ground_truth, prediction) -> (ground_truth, prediction), as the reference; the
device functions take None or a `ThumosPostprocessing` (prego_amd/postprocessing.py), which they run on the device
(`prego_thumos_postprocess`) in front of the same metric entries."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np


def average_precision_columns(scores: np.ndarray, positive: np.ndarray) -> np.ndarray:
    """AP of every column: scores [frames, classes] (any float dtype), positive [frames, classes] bool -> float64 [classes],
    NaN where a column has no positive."""
    scores = np.asarray(scores)
    positive = np.asarray(positive, dtype=bool)
    n = scores.shape[0]
    order = np.argsort(-scores, axis=0, kind="stable")
    ranked = np.take_along_axis(scores, order, axis=0)
    hits = np.cumsum(np.take_along_axis(positive, order, axis=0), axis=0, dtype=np.int64)      # positives at or above each rank
    closes = np.ones_like(positive)                                                            # rank closes a run of equal scores
    closes[:-1] = ranked[:-1] != ranked[1:]
    # positives at the previous threshold: the running maximum of `hits` over the earlier run ends (hits is monotone)
    at_end = np.where(closes, hits, 0)
    before = np.zeros_like(hits)
    before[1:] = np.maximum.accumulate(at_end, axis=0)[:-1]
    seen = np.arange(1, n + 1, dtype=np.float64)[:, None]
    total = hits[-1].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ap = np.where(closes, (hits - before) * (hits / seen), 0.0).sum(axis=0) / total
    return np.where(total > 0, ap, np.nan)


def calibrated_average_precision_columns(scores: np.ndarray, positive: np.ndarray) -> np.ndarray:
    """cAP of every column (metrics.py:10-22 of the reference, all classes at once): precision re-weighted by the negative /
    positive ratio w, cprec_k = TP_k / (TP_k + FP_k / (w + eps) + eps), averaged over the ranks that hold a positive.  Rows of equal
    score keep their input order (stable sort; the reference's unstable argsort leaves ties to chance)."""
    scores = np.asarray(scores)
    positive = np.asarray(positive, dtype=bool)
    eps = np.finfo(float).eps
    order = np.argsort(-scores, axis=0, kind="stable")
    tp = np.take_along_axis(positive, order, axis=0).astype(np.float64)
    tps = np.cumsum(tp, axis=0)
    fps = np.cumsum(1.0 - tp, axis=0)
    total = tp.sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = (tp.shape[0] - total) / total
        cprec = tps / (tps + fps / (ratio + eps) + eps)
        cap = (cprec * tp).sum(axis=0) / total
    return np.where(total > 0, cap, np.nan)


def _report(ap, n_true, score_sum, class_names):
    """the reference's result dict: per-class AP (classes 1.. that have a positive), its log strings, and their mean"""
    res = OrderedDict(per_class_AP=OrderedDict(), num=OrderedDict())
    for c in range(1, len(class_names)):                    # class 0 = background, never scored (metrics.py:44-48)
        if n_true[c] > 0:
            name = class_names[c]
            res["per_class_AP"][name] = float(ap[c])
            res["num"][name] = f"[true: {int(n_true[c])}, pred:{int(score_sum[c])}, AP:{ap[c] * 100:.1f}]"
    with np.errstate(invalid="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            res["mean_AP"] = np.mean(list(res["per_class_AP"].values())) if res["per_class_AP"] else float("nan")
    return res


def perframe_ap_raw(pred: np.ndarray, truth: np.ndarray, metrics="AP"):
    """(AP or cAP per column, positives per column, score mass per column) of host matrices [frames, classes]: the three vectors the
    report is built from (class-sharded multi-rank eval computes them for its own columns and gathers only these)"""
    cols = average_precision_columns if metrics == "AP" else calibrated_average_precision_columns
    if pred.shape[0] == 0:
        z = np.zeros(pred.shape[1])
        return z, z.astype(np.int64), z.copy()
    return cols(pred, truth != 0), (truth != 0).sum(0), pred.sum(0, dtype=np.float64)


def report_from_raw(ap, n_true, score_sum, class_names):
    return _report(np.asarray(ap), np.asarray(n_true), np.asarray(score_sum), class_names)


def perframe_average_precision(prediction, ground_truth, class_names, postprocessing=None, metrics="AP"):
    """Host path: prediction / ground_truth [frames, classes] (lists of rows or arrays, as trainer/eval.py collects them)."""
    if metrics not in ("AP", "cAP"):
        raise RuntimeError(f"Unknown metrics: {metrics}")
    truth = np.asarray(ground_truth)
    pred = np.asarray(prediction)
    if postprocessing is not None:
        truth, pred = postprocessing(truth, pred)
    if truth.ndim != 2 or truth.shape[0] == 0:          # an empty eval set: the reference's np.mean([]) = nan, no per-class entries
        return _report(np.zeros(len(class_names)), np.zeros(len(class_names), np.int64), np.zeros(len(class_names)), class_names)
    cols = average_precision_columns if metrics == "AP" else calibrated_average_precision_columns
    return _report(cols(pred, truth != 0), (truth != 0).sum(0), pred.sum(0, dtype=np.float64), class_names)


def perframe_ap_raw_device(pred, truth, metrics="AP"):
    """device counterpart of perframe_ap_raw (metric 'AP' or 'cAP'): fp32 CUDA matrices [frames, classes] (truth: or class ids [frames]) -> three host vectors"""
    ncls = int(pred.shape[1])
    fin = perframe_average_precision_device(pred, truth, [str(i) for i in range(ncls)], None, metrics, defer=True, raw=True)
    return fin()


def _postprocess_device(what, prediction, ground_truth, postprocessing, n_valid):
    """the device metrics' `postprocessing` argument: None, or a ThumosPostprocessing (prego_thumos_postprocess in front of the
    unchanged metric entries).  Returns (prediction, ground_truth, check): `check` compares the device's count of kept rows with the
    `n_valid` hint once the metric's kernels are done (None: nothing to compare)."""
    from ._lib import PregoError
    from .postprocessing import ThumosPostprocessing, thumos_postprocessing_device
    if postprocessing is None:
        if n_valid is not None:
            raise PregoError(f"{what}: n_valid is the hint of a ThumosPostprocessing")
        return prediction, ground_truth, None
    if not isinstance(postprocessing, ThumosPostprocessing):
        raise PregoError(f"{what}: the only postprocessing on the device is a ThumosPostprocessing (any other callable: the host "
                         "functions)")
    if not (prediction.is_cuda and ground_truth.is_cuda):
        raise PregoError(f"{what} needs CUDA tensors; there is no CPU fallback")
    res = thumos_postprocessing_device(prediction, ground_truth, postprocessing, n_valid)
    return res[1], res[0], (res.check if n_valid is not None else None)


def _need_cuda(what, *tensors):
    from ._lib import PregoError
    if not all(t.is_cuda for t in tensors):
        raise PregoError(f"{what} needs CUDA tensors; there is no CPU fallback (host arrays: {what[:-len('_device')]})")


def _device_metric(what, kind, prediction, truth, class_names, postprocessing, n_valid, cal, rows, n_out, report, defer, raw):
    """What the two device functions share behind their own argument checks: the post-processing, fp32 scores and the targets as the
    entry wants them, the shape check, workspace and outputs, the call of prego_<kind>_ap / _cap (`cal`) (`_labels`: one id per
    frame) on the current stream, and the function that collects the result.  The entry writes `n_out` arrays of shape `rows` +
    (classes,) - the metric, the positives (int64), per frame also the score mass -; an empty set gives zeros without a call.
    raw: those arrays; else report(*arrays, class_names).  defer: the collecting function is returned instead of called."""
    import ctypes as C

    import torch

    from . import _lib
    from ._lib import PregoError, check
    prediction, truth, count_check = _postprocess_device(what, prediction, truth, postprocessing, n_valid)
    _need_cuda(what, prediction, truth)
    pred = prediction.detach().to(torch.float32).contiguous()
    by_label = truth.dim() == 1 and not truth.dtype.is_floating_point      # one class id per frame
    truth = truth.detach().to(torch.int32 if by_label else torch.float32).contiguous()
    if pred.dim() != 2 or pred.shape[1] != len(class_names) or (truth.shape != pred.shape[:1] if by_label else truth.shape != pred.shape):
        raise PregoError(f"{what}: shapes {tuple(pred.shape)} / {tuple(truth.shape)} for {len(class_names)} classes")
    n, ncls = pred.shape
    out = ws = None
    if n > 0:                                           # an empty eval set: same empty report as the host path
        lib = _lib.load()
        dev = pred.device
        stem = f"prego_{kind}_{'cap' if cal else 'ap'}"
        ws = torch.empty(getattr(lib, stem + "_workspace_bytes")(n, ncls), dtype=torch.uint8, device=dev)
        out = torch.empty((n_out,) + rows + (ncls,), dtype=torch.float64, device=dev)      # the positives as int64 bits
        p = lambda t: C.c_void_p(t.data_ptr())
        with torch.cuda.device(dev):
            check(getattr(lib, stem + ("_labels" if by_label else ""))(p(pred), p(truth), n, ncls, *[p(o) for o in out], p(ws), ws.numel(),
                                                                       C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

    def finish(_keep=(pred, truth, ws)):
        host = out.cpu().numpy() if n > 0 else np.zeros((n_out,) + rows + (ncls,))
        if count_check is not None:
            count_check()
        arrays = [h.view(np.int64) if i == 1 else h for i, h in enumerate(host)]
        return tuple(a.copy() for a in arrays) if raw else report(*arrays, class_names)
    return finish if defer else finish()


def perframe_average_precision_device(prediction, ground_truth, class_names, postprocessing=None, metrics="AP", defer=False, raw=False,
                                      n_valid=None):
    """Device path: prediction / ground_truth fp32 CUDA tensors [frames, classes] - or ground_truth = an integer CUDA tensor [frames],
    one class id per frame (what one-hot targets say; an id outside the classes = no positive) -; the sort and the scan run in
    libprego_amd.so (`prego_perframe_ap`), one small device -> host transfer brings back AP, positives and score mass.
    metrics='cAP': the calibrated metric (`prego_perframe_cap` / `prego_perframe_cap_labels`), frames of equal score in frame order as
    `calibrated_average_precision_columns` ranks them.
    postprocessing: None or a `ThumosPostprocessing` (prego_amd/postprocessing.py): the scores and targets are post-processed on the
    device (`prego_thumos_postprocess`) and the same metric entries run on the compacted matrices.  n_valid: the rows it keeps, when the
    caller knows them (ThumosPostprocessing.count_valid on host targets) - then nothing here waits for the device, and the count is
    compared when the result is collected (PregoError on a mismatch); without it the count is read back before the metric is enqueued.
    defer=True: the kernels are only ENQUEUED and a function is returned that waits for them and builds the report (Evaluate writes
    its output file while the GPU sorts)."""
    from ._lib import PregoError
    if metrics not in ("AP", "cAP"):
        raise PregoError("perframe_average_precision_device: metric 'AP' or 'cAP' only")
    return _device_metric("perframe_average_precision_device", "perframe", prediction, ground_truth, class_names, postprocessing, n_valid,
                          metrics == "cAP", (), 3, _report, defer, raw)


# ------------------------------------------------------------------------------------------------------------------------------
# per-stage average precision (metrics.py:64-130 of the reference)
# ------------------------------------------------------------------------------------------------------------------------------
N_STAGES = 10
STAGE_NAMES = tuple("{:2}%_{:3}%".format(s * 10, (s + 1) * 10) for s in range(N_STAGES))


def stage_members(positive: np.ndarray) -> np.ndarray:
    """positive [frames] bool -> [10, frames] bool: the frames of each stage of every maximal run of positives"""
    g = np.asarray(positive, dtype=bool)
    n = g.shape[0]
    out = np.zeros((N_STAGES, n), dtype=bool)
    if n == 0 or not g.any():
        return out
    prev = np.concatenate(([False], g[:-1]))
    nxt = np.concatenate((g[1:], [False]))
    starts = np.flatnonzero(g & ~prev)
    lens = np.flatnonzero(g & ~nxt) - starts                   # last - first: one less than the frame count
    for s in range(N_STAGES):
        lo = starts + (lens * (s / 10)).astype(np.int64)       # the reference's int(len * perc): a float64 product, truncated
        hi = np.maximum(lo + 1, starts + (lens * ((s + 1) / 10)).astype(np.int64))
        edge = np.zeros(n + 1, dtype=np.int64)                 # runs do not overlap, nor do their stages
        edge[lo] += 1
        edge[hi] -= 1
        out[s] = np.cumsum(edge[:n]) > 0
    return out


def _class_positive(truth: np.ndarray, c: int) -> np.ndarray:
    """frames of class c: the column == 1 of a dense target matrix (metrics.py:120) or the ids == c of one id per frame"""
    return truth == c if truth.ndim == 1 else truth[:, c] == 1


def perstage_ap_raw(pred: np.ndarray, truth: np.ndarray, metrics="AP"):
    """(AP or cAP [10, classes], positives [10, classes]) of host scores [frames, classes] and targets [frames, classes] or ids
    [frames]; every class, class 0 included.  'AP': 0.0 for a set without positives; 'cAP': NaN."""
    if metrics not in ("AP", "cAP"):
        raise RuntimeError(f"Unknown metrics: {metrics}")
    pred = np.asarray(pred)
    truth = np.asarray(truth)
    n, ncls = pred.shape
    ap = np.zeros((N_STAGES, ncls))
    n_pos = np.zeros((N_STAGES, ncls), dtype=np.int64)
    cols = average_precision_columns if metrics == "AP" else calibrated_average_precision_columns
    for c in range(ncls):
        g = _class_positive(truth, c)
        member = stage_members(g)
        order = np.argsort(-pred[:, c], kind="stable")         # once per class: every stage's set is a subset in this order
        for s in range(N_STAGES):
            keep = order[(~g | member[s])[order]]
            n_pos[s, c] = int(member[s].sum())
            if n_pos[s, c] == 0:
                ap[s, c] = 0.0 if metrics == "AP" else np.nan
            else:
                ap[s, c] = cols(pred[keep, c][:, None], member[s][keep][:, None])[0]
    return ap, n_pos


def perstage_report(ap, class_names):
    """the reference's result dict from AP [10, classes]: per stage the AP of every class 1.. and their mean"""
    ap = np.asarray(ap)
    res = OrderedDict()
    for s, name in enumerate(STAGE_NAMES):
        per = OrderedDict((class_names[c], float(ap[s, c])) for c in range(1, len(class_names)))     # class 0 = background
        with np.errstate(invalid="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                mean = np.mean(list(per.values())) if per else float("nan")
        res[name] = OrderedDict(per_class_AP=per, mean_AP=mean)
    return res


def perstage_average_precision(prediction, ground_truth, class_names, postprocessing=None, metrics="AP"):
    """Host path: prediction [frames, classes]; ground_truth [frames, classes] (positive: == 1, as the reference) or one class id per
    frame [frames].  The frames are in evaluation order: a run is not cut where two videos meet."""
    if metrics not in ("AP", "cAP"):
        raise RuntimeError(f"Unknown metrics: {metrics}")
    truth = np.asarray(ground_truth)
    pred = np.asarray(prediction)
    if postprocessing is not None:
        truth, pred = postprocessing(truth, pred)
    if pred.ndim != 2 or pred.shape[0] == 0:
        return perstage_report(np.zeros((N_STAGES, len(class_names))), class_names)
    return perstage_report(perstage_ap_raw(pred, truth, metrics)[0], class_names)


def perstage_average_precision_device(prediction, labels, class_names, defer=False, raw=False, metrics="AP", postprocessing=None,
                                      n_valid=None):
    """Device path: prediction fp32 CUDA tensor [frames, classes], labels an integer CUDA tensor [frames] with one class
    id per frame in evaluation order (an id outside the classes = a negative of every class); `prego_perstage_ap_labels` in
    libprego_amd.so, one small device -> host transfer brings back AP and positives [10, classes].  No CPU fallback.
    metrics='cAP': the calibrated metric (`prego_perstage_cap_labels`), frames of equal score in frame order; a (class, stage)
    without a member is NaN, as on the host.
    raw=True: (AP [10, classes], positives [10, classes]) of every class instead of the report.
    defer=True: the kernels are only ENQUEUED and a function is returned that waits for them and builds the result.
    postprocessing / n_valid: None or a `ThumosPostprocessing` and its hint, as perframe_average_precision_device (the runs are those
    of the frames that are left: removing a frame makes its neighbours adjacent)."""
    import torch

    from ._lib import PregoError
    if metrics not in ("AP", "cAP"):
        raise PregoError(f"perstage_average_precision_device: metrics {metrics!r} ('AP' or 'cAP')")
    _need_cuda("perstage_average_precision_device", prediction, labels)
    if labels.dim() != 1 or labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise PregoError("perstage_average_precision_device: labels must be one integer class id per frame [frames] "
                         "(dense target matrices: perstage_average_precision on the host)")
    return _device_metric("perstage_average_precision_device", "perstage", prediction, labels, class_names, postprocessing, n_valid,
                          metrics == "cAP", (N_STAGES,), 2, lambda ap, n_pos, names: perstage_report(ap, names), defer, raw)
