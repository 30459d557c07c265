"""THUMOS post-processing (the reference's utils/postprocessing.py:4-29, from Shou et al. 2017), applied in front of every metric when
the data set is THUMOS: an optional 5-frame temporal max ("smooth"), the optional CliffDiving (5) -> Diving (8) merge ("switch"), and
the removal of the frames whose "ambiguous" target column (21) is 1.  Two routes to the same bits:

  * `thumos_postprocessing` / `ThumosPostprocessing.__call__`  - numpy on the host, the `postprocessing` argument of the host metrics.
  * `thumos_postprocessing_device`                             - the HIP path (`prego_thumos_postprocess(_labels)`,
                                                                 csrc/thumos_post.hip); no CPU fallback.

The definition (include/prego_amd.h says the same): s'[i][c] = max over d in (0, -1, +1, -2, +2) of s[j][c] with j = i + d inside
[0, n) and j = i otherwise - bit for bit the reference's five shifted copies for n >= 2, and the definition for n == 1, where the
reference's np.squeeze drops the frame axis; then s'[i][to] = s'[i][from] where that is greater; then the rows with
target[i][ambiguous] != 1 (or id != ambiguous) are kept, in frame order.  Unlike the reference (switch without smooth) nothing here
writes its arguments."""
from __future__ import annotations

import numpy as np


def _smooth(pred: np.ndarray) -> np.ndarray:
    n = pred.shape[0]
    i = np.arange(n)
    out = pred.copy()
    for d in (-1, 1, -2, 2):                                   # the reference's order of its five copies
        j = i + d
        out = np.maximum(out, pred[np.where((j >= 0) & (j < n), j, i)])
    return out


def _host(ground_truth, prediction, smooth, switch, switch_from, switch_to, ambiguous):
    truth = np.asarray(ground_truth)
    pred = np.asarray(prediction)
    if pred.ndim != 2 or truth.shape[:1] != pred.shape[:1] or truth.ndim not in (1, 2):
        raise ValueError(f"thumos_postprocessing: prediction {pred.shape}, ground_truth {truth.shape}")
    if smooth:
        pred = _smooth(pred)
    if switch:
        pred = pred.copy()
        pred[:, switch_to] = np.where(pred[:, switch_from] > pred[:, switch_to], pred[:, switch_from], pred[:, switch_to])
    if ambiguous < 0:
        valid = np.arange(pred.shape[0])
    else:
        valid = np.where((truth if truth.ndim == 1 else truth[:, ambiguous]) != (ambiguous if truth.ndim == 1 else 1))[0]
    return truth[valid], pred[valid]


def thumos_postprocessing(ground_truth, prediction, smooth=False, switch=False):
    """The reference's signature and return order: (ground_truth[valid], prediction[valid]).  ground_truth: [frames, classes], or one
    class id per frame [frames]."""
    return _host(ground_truth, prediction, smooth, switch, 5, 8, 21)


class ThumosPostprocessing:
    """The post-processing as an object: called on host arrays it is `thumos_postprocessing` (so it is a `postprocessing` argument of
    the host metrics); the device metrics recognise it by type and run `prego_thumos_postprocess`.  ambiguous = -1 keeps every row."""

    def __init__(self, smooth=False, switch=False, switch_from=5, switch_to=8, ambiguous=21):
        self.smooth, self.switch = bool(smooth), bool(switch)
        self.switch_from, self.switch_to, self.ambiguous = int(switch_from), int(switch_to), int(ambiguous)

    def __call__(self, ground_truth, prediction):
        return _host(ground_truth, prediction, self.smooth, self.switch, self.switch_from, self.switch_to, self.ambiguous)

    def count_valid(self, ground_truth) -> int:
        """the rows `__call__` keeps, from host targets ([frames, classes] or ids): the `n_valid` hint of the device functions"""
        t = np.asarray(ground_truth)
        if self.ambiguous < 0:
            return int(t.shape[0])
        return int(np.count_nonzero((t != self.ambiguous) if t.ndim == 1 else (t[:, self.ambiguous] != 1)))

    def __repr__(self):
        return (f"ThumosPostprocessing(smooth={self.smooth}, switch={self.switch}, switch_from={self.switch_from}, "
                f"switch_to={self.switch_to}, ambiguous={self.ambiguous})")


class Postprocessed(tuple):
    """(ground_truth, prediction) of `thumos_postprocessing_device`; `count` is the device int64 holding the kept rows and `check()`
    compares it with the `n_valid` hint the tensors were sized by (one 8-byte copy that waits for the kernels)."""

    def __new__(cls, ground_truth, prediction, count, hint, keep):
        self = super().__new__(cls, (ground_truth, prediction))
        self.count, self.hint, self._keep = count, hint, keep
        return self

    def check(self, count=None):
        """count: the device count's value when the caller has already brought it to the host"""
        from ._lib import PregoError
        got = int(self.count.item()) if count is None else int(count)
        if self.hint is not None and got != self.hint:
            raise PregoError(f"thumos_postprocessing_device: n_valid={self.hint} was given but the device kept {got} rows; the tensors "
                             "sized by the hint do not hold the result")
        return got


def _rows(t, dtype):
    """a [n, C] tensor as the C entry reads it: (tensor, row stride in elements) - a [:, l, :] view of an [n, L, C] tensor stays a view"""
    t = t.detach()
    if t.dtype != dtype:
        t = t.to(dtype)
    if t.dim() == 2 and t.shape[0] > 1 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return t, int(t.stride(0))
    t = t.contiguous()
    return t, int(t.shape[1])


def thumos_postprocessing_device(prediction, ground_truth, post: ThumosPostprocessing, n_valid=None) -> Postprocessed:
    """prediction: fp32 CUDA tensor [frames, classes]; ground_truth: fp32 CUDA tensor [frames, classes] or an integer CUDA tensor
    [frames] (one class id per frame); strided [:, l, :] views are read in place.  Returns (ground_truth, prediction) compacted, on the
    current stream.  n_valid given (the kept rows, counted where the targets were on the host: `post.count_valid`): the results are
    sized by it and nothing waits for the device; `.check()` - or the metric that collects them - compares it with the device's count
    and raises PregoError on a mismatch.  Without it the count is read back: one 8-byte copy that waits for the kernels."""
    import ctypes as C

    import torch

    from . import _lib
    from ._lib import PregoError, check
    if not isinstance(post, ThumosPostprocessing):
        raise PregoError("thumos_postprocessing_device: post must be a ThumosPostprocessing")
    if not (prediction.is_cuda and ground_truth.is_cuda):
        raise PregoError("thumos_postprocessing_device needs CUDA tensors; there is no CPU fallback (host arrays: thumos_postprocessing)")
    by_label = ground_truth.dim() == 1 and not ground_truth.dtype.is_floating_point and ground_truth.dtype != torch.bool
    if prediction.dim() != 2 or (ground_truth.shape != prediction.shape[:1] if by_label else ground_truth.shape != prediction.shape):
        raise PregoError(f"thumos_postprocessing_device: shapes {tuple(prediction.shape)} / {tuple(ground_truth.shape)}")
    pred, ld_p = _rows(prediction, torch.float32)
    if by_label:
        truth, ld_t = ground_truth.detach().to(torch.int32).contiguous(), 0
    else:
        truth, ld_t = _rows(ground_truth, torch.float32)
    n, ncls = (int(x) for x in pred.shape)
    dev = pred.device
    if n_valid is not None and not 0 <= int(n_valid) <= n:
        raise PregoError(f"thumos_postprocessing_device: n_valid={n_valid} for {n} frames")
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    if n == 0:
        return Postprocessed(truth, pred, cnt, None if n_valid is None else int(n_valid), ())
    lib = _lib.load()
    pred_out = torch.empty((n, ncls), dtype=torch.float32, device=dev)
    truth_out = torch.empty(truth.shape, dtype=truth.dtype, device=dev)
    ws = torch.empty(lib.prego_thumos_postprocess_workspace_bytes(n, ncls), dtype=torch.uint8, device=dev)
    flags = (_lib.THUMOS_SMOOTH if post.smooth else 0) | (_lib.THUMOS_SWITCH if post.switch else 0)
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if by_label:
            check(lib.prego_thumos_postprocess_labels(p(pred), ld_p, p(truth), n, ncls, flags, post.switch_from, post.switch_to, post.ambiguous,
                                                      p(pred_out), p(truth_out), p(cnt), p(ws), ws.numel(), s))
        else:
            check(lib.prego_thumos_postprocess(p(pred), ld_p, p(truth), ld_t, n, ncls, flags, post.switch_from, post.switch_to, post.ambiguous,
                                               p(pred_out), p(truth_out), p(cnt), p(ws), ws.numel(), s))
    hint = None if n_valid is None else int(n_valid)
    kept = int(cnt.item()) if hint is None else hint
    return Postprocessed(truth_out[:kept], pred_out[:kept], cnt, hint, (pred, truth, ws, pred_out, truth_out))
