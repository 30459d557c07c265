"""Segmental metrics: frame accuracy (MoF), segmental Edit score and segmental F1 at three overlaps - what step-recognition results
on Assembly101 are reported in, and the first figures of this project that judge the TRANSCRIPT a recogniser's per-frame ids spell out
(the 200-frame vote, the stream pools' records and the procedure model all read transcripts; per-frame AP does not see them).

Definitions (include/prego_amd.h, prego_segmental_scores, carries them word for word).  The segments of one video's label sequence are
its maximal runs of equal id, in frame order, never across a video boundary; runs of a background id (ids in [0, 128) named in `bg`)
are dropped, and two runs of one id around a dropped run stay two segments.  Per video: correct / frames (background frames count),
m / n segments of pred / gt, dist = the Levenshtein distance of the two segment-id lists, and tp_k for three overlaps num_k / den_k: a
pred segment p looks at the same-id gt segments it intersects, takes the one with the largest inter / union (64-bit cross products, the
earliest on a tie) and qualifies at k when inter * den_k >= union * num_k; tp_k counts the gt segments that are some qualifying p's
best.  The record of a video is the 8 integers correct | frames | m | n | dist | tp_0 | tp_1 | tp_2.

  * `segments`, `edit_distance`, `segmental_records`   - the host model, in integers (numpy): the oracle of the kernel.
  * `segmental_report`                                 - records -> MoF, Edit, F1@.. in fp64 (pooled over the videos).
  * `segmental_scores`                                 - host lists / arrays of per-frame ids (or transcripts: Edit only) -> report.
  * `segmental_scores_device`                          - the HIP path, `prego_segmental_scores` (csrc/segmental.hip): one launch, one
                                                         workgroup per video, 32 bytes per video come back.  No CPU fallback."""
from __future__ import annotations

import numpy as np

DEFAULT_OVERLAPS = ((1, 10), (1, 4), (1, 2))
RECORD_FIELDS = ("correct", "frames", "m", "n", "dist", "tp_0", "tp_1", "tp_2")


def _overlaps(overlaps):
    """three (num, den) pairs, 0 < num <= den <= 32768"""
    out = []
    for o in overlaps:
        num, den = int(o[0]), int(o[1])
        if not 0 < num <= den <= 32768:
            raise ValueError(f"segmental: overlap {o!r} (0 < num <= den <= 32768)")
        out.append((num, den))
    if len(out) != 3:
        raise ValueError(f"segmental: {len(out)} overlaps (exactly three)")
    return tuple(out)


def _bg_words(bg):
    """the 128-bit background mask as four 32-bit words"""
    words = [0, 0, 0, 0]
    for c in bg:
        c = int(c)
        if not 0 <= c < 128:
            raise ValueError(f"segmental: background id {c} (only ids in [0, 128) can be background)")
        words[c >> 5] |= 1 << (c & 31)
    return words


def _overlap_name(num, den):
    """'F1@10' for 1/10, 'F1@25' for 1/4; an overlap that is no whole percentage keeps its fraction: 'F1@1/3'"""
    return f"F1@{100 * num // den}" if (100 * num) % den == 0 else f"F1@{num}/{den}"


def voted_frames(labels, window: int = 200) -> np.ndarray:
    """the per-frame sequence the anticipator reads (utils/aggregate.py:55-72): every window of `window` frames replaced by its most
    frequent id (ties: the lowest), the last window as long as it is.  Host form of prego_window_vote expanded back to frames."""
    x = np.asarray(labels, dtype=np.int64).reshape(-1)
    out = np.empty_like(x)
    for s in range(0, x.size, window):
        out[s:s + window] = np.argmax(np.bincount(x[s:s + window]))
    return out


def segments(labels, bg=()) -> np.ndarray:
    """labels: the ids of ONE video, one per frame -> int64 [k, 3], rows (id, start, end) with end exclusive: its maximal runs of equal id
    in frame order, the runs of an id in `bg` dropped."""
    x = np.asarray(labels, dtype=np.int64).reshape(-1)
    if x.size == 0:
        return np.zeros((0, 3), np.int64)
    head = np.flatnonzero(np.concatenate(([True], x[1:] != x[:-1])))
    seg = np.stack([x[head], head, np.concatenate((head[1:], [x.size]))], axis=1)
    words = _bg_words(bg)
    if any(words):
        drop = np.isin(seg[:, 0], [c for c in range(128) if words[c >> 5] >> (c & 31) & 1])
        seg = seg[~drop]
    return seg


def edit_distance(a, b) -> int:
    """Levenshtein distance of two id lists: insert, delete, substitute 1, match 0.  Row by row; the insertions of a row are a running
    minimum: cur[j] = min over k <= j of (t[k] + j - k)."""
    a = np.asarray(a, dtype=np.int64).reshape(-1)
    b = np.asarray(b, dtype=np.int64).reshape(-1)
    if a.size < b.size:
        a, b = b, a
    if b.size == 0:
        return int(a.size)
    ramp = np.arange(b.size + 1, dtype=np.int64)
    row = ramp.copy()
    for i in range(a.size):
        t = np.empty_like(row)
        t[0] = i + 1
        t[1:] = np.minimum(row[1:] + 1, row[:-1] + (b != a[i]))
        row = np.minimum.accumulate(t - ramp) + ramp
    return int(row[-1])


def _true_positives(ps, gs, overlaps):
    """tp_k of one video from its pred / gt segments [k, 3]"""
    hit = np.zeros(gs.shape[0], np.int64)
    if gs.shape[0]:
        g_lab, g_st, g_en = gs[:, 0], gs[:, 1], gs[:, 2]
        first = np.searchsorted(g_en, ps[:, 1], side="right")          # the first gt segment that ends behind the pred segment's start
        last = np.searchsorted(g_st, ps[:, 2], side="left")            # ... and the first that starts at or behind its end
        for (lab, s, e), lo, hi in zip(ps.tolist(), first.tolist(), last.tolist()):
            best, bi, bu = -1, 0, 1
            for g in range(lo, hi):
                if g_lab[g] != lab:
                    continue
                inter = min(e, int(g_en[g])) - max(s, int(g_st[g]))
                union = max(e, int(g_en[g])) - min(s, int(g_st[g]))
                if best < 0 or inter * bu > bi * union:                  # Python integers: exact
                    best, bi, bu = g, inter, union
            if best >= 0:
                for k, (num, den) in enumerate(overlaps):
                    if bi * den >= bu * num:
                        hit[best] |= 1 << k
    return [int(np.count_nonzero(hit >> k & 1)) for k in range(3)]


def segmental_records(pred_videos, gt_videos, bg=(), overlaps=DEFAULT_OVERLAPS) -> np.ndarray:
    """pred_videos / gt_videos: one sequence of per-frame ids per video (equal lengths pairwise) -> int32 [videos, 8], the records."""
    overlaps = _overlaps(overlaps)
    if len(pred_videos) != len(gt_videos):
        raise ValueError(f"segmental: {len(pred_videos)} pred videos, {len(gt_videos)} gt videos")
    rec = np.zeros((len(pred_videos), 8), np.int32)
    for v, (p, g) in enumerate(zip(pred_videos, gt_videos)):
        p = np.asarray(p, dtype=np.int64).reshape(-1)
        g = np.asarray(g, dtype=np.int64).reshape(-1)
        if p.size != g.size:
            raise ValueError(f"segmental: video {v} has {p.size} pred and {g.size} gt frames")
        ps, gs = segments(p, bg), segments(g, bg)
        rec[v, :5] = (int(np.count_nonzero(p == g)), p.size, ps.shape[0], gs.shape[0], edit_distance(ps[:, 0], gs[:, 0]))
        rec[v, 5:] = _true_positives(ps, gs, overlaps)
    return rec


def segmental_report(records, overlaps=DEFAULT_OVERLAPS) -> dict:
    """records [videos, 8] -> {"MoF", "Edit", "F1@10", "F1@25", "F1@50", "videos", "per_video"} (the F1 keys named from `overlaps`), fp64:
    MoF = 100 * sum(correct) / sum(frames) (0.0 without frames); Edit = the mean over the videos of 100 * (1 - dist / max(m, n, 1));
    F1@k = 200 * TP_k / (M + N) over the sums (0.0 when M + N == 0) = 2PR / (P + R) with P = TP / M, R = TP / N pooled over the videos.
    per_video: the records as dicts with the video's own Edit."""
    overlaps = _overlaps(overlaps)
    rec = np.asarray(records, dtype=np.int64).reshape(-1, 8)
    tot = rec.sum(axis=0)
    edits = [100.0 * (1.0 - float(r[4]) / float(max(int(r[2]), int(r[3]), 1))) for r in rec]
    rep = {"MoF": 100.0 * float(tot[0]) / float(tot[1]) if tot[1] > 0 else 0.0,
           "Edit": float(np.mean(np.asarray(edits, dtype=np.float64))) if edits else 0.0}
    for k, (num, den) in enumerate(overlaps):
        rep[_overlap_name(num, den)] = 200.0 * float(tot[5 + k]) / float(tot[2] + tot[3]) if tot[2] + tot[3] > 0 else 0.0
    rep["videos"] = int(rec.shape[0])
    rep["per_video"] = [dict(zip(RECORD_FIELDS, (int(x) for x in r)), Edit=e) for r, e in zip(rec, edits)]
    return rep


def segmental_scores(pred_videos, gt_videos, bg=(), overlaps=DEFAULT_OVERLAPS, transcripts=False) -> dict:
    """Host path: per-frame ids per video (lists or arrays) -> `segmental_report` of `segmental_records`.
    transcripts=True: every sequence IS a segment-id list without extents - a stream pool's `close()['pred']`, the sequences of
    tests/golden/procedure_assembly101o.json - and pred / gt of a video may differ in length: only the Edit score is defined.  Every
    entry is one segment (no merging; entries of a `bg` id dropped); the report holds "Edit", "videos" and "per_video" (m, n, dist, Edit)."""
    if not transcripts:
        return segmental_report(segmental_records(pred_videos, gt_videos, bg, overlaps), overlaps)
    if len(pred_videos) != len(gt_videos):
        raise ValueError(f"segmental: {len(pred_videos)} pred transcripts, {len(gt_videos)} gt transcripts")
    bg_ids = [c for c in range(128) if _bg_words(bg)[c >> 5] >> (c & 31) & 1]
    per = []
    for p, g in zip(pred_videos, gt_videos):
        p = np.asarray(p, dtype=np.int64).reshape(-1)
        g = np.asarray(g, dtype=np.int64).reshape(-1)
        p, g = p[~np.isin(p, bg_ids)], g[~np.isin(g, bg_ids)]
        d = edit_distance(p, g)
        per.append({"m": int(p.size), "n": int(g.size), "dist": d, "Edit": 100.0 * (1.0 - float(d) / float(max(p.size, g.size, 1)))})
    return {"Edit": float(np.mean(np.asarray([v["Edit"] for v in per], dtype=np.float64))) if per else 0.0, "videos": len(per),
            "per_video": per}


def segmental_scores_device(pred, gt, offsets, bg=(), overlaps=DEFAULT_OVERLAPS, defer=False, raw=False):
    """Device path: pred / gt int32 CUDA tensors [frames] (one id per frame, the videos one after the other), offsets an int32 CUDA tensor
    [videos + 1] (video v = frames [offsets[v], offsets[v + 1]), ascending); `prego_segmental_scores` on the current stream, 32 bytes per
    video come back.  No CPU fallback (host lists: `segmental_scores`).
    raw=True: the records int32 [videos, 8] instead of the report.  defer=True: the kernel is only ENQUEUED and a function is returned
    that waits for it and builds the result."""
    import ctypes as C

    import torch

    from . import _lib
    from ._lib import PregoError, check
    what = "segmental_scores_device"
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in (pred, gt, offsets)):
        raise PregoError(f"{what} needs CUDA tensors; there is no CPU fallback (host arrays: segmental_scores)")
    if any(t.dtype != torch.int32 or t.dim() != 1 for t in (pred, gt, offsets)):
        raise PregoError(f"{what}: pred, gt and offsets must be one-dimensional int32 tensors")
    if pred.shape != gt.shape or offsets.numel() < 2:
        raise PregoError(f"{what}: {pred.numel()} pred and {gt.numel()} gt frames, {offsets.numel()} offsets (videos + 1, at least 2)")
    overlaps = _overlaps(overlaps)
    words = _bg_words(bg)
    pred, gt, offsets = pred.contiguous(), gt.contiguous(), offsets.contiguous()
    n, nv = int(pred.numel()), int(offsets.numel()) - 1
    lib = _lib.load()
    dev = pred.device
    if n == 0:                                          # an empty tensor has no address; the entry wants non-NULL arrays and reads nothing
        pred = gt = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.prego_segmental_workspace_bytes(n, nv), dtype=torch.uint8, device=dev)
    out = torch.empty((nv, 8), dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        check(lib.prego_segmental_scores(p(pred), p(gt), p(offsets), nv, n, (C.c_uint32 * 4)(*words), (C.c_int32 * 3)(*[o[0] for o in overlaps]),
                                         (C.c_int32 * 3)(*[o[1] for o in overlaps]), p(out), p(ws) if n > 0 else None, ws.numel(),
                                         C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

    def finish(_keep=(pred, gt, offsets, ws)):
        rec = out.cpu().numpy()
        return rec if raw else segmental_report(rec, overlaps)
    return finish if defer else finish()
