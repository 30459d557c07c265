"""Per-frame argmax -> 200-frame majority vote -> step sequence (utils/aggregate.py:46-90), the wire format
into step_anticipation.  `aggregate` is the host (numpy) form over the JSON the eval loop wrote;
`aggregate_device` takes the int32 per-frame argmax tensors the head kernel left in HBM and runs the majority vote there
(`prego_window_vote`, csrc/postproc.hip): one int32 per 200-frame window crosses PCIe instead of one per frame.
`aggregate_online` / `OnlineRecord` is the same rule fed one id at a time, or a burst at a time (`push_frames`): the host model of the record a stream pool keeps per slot
(prego_amd/stream_pool.py, csrc/stream_pool.hip)."""
from __future__ import annotations

import json

import numpy as np


def _changes(a):
    r = [i for i in range(1, len(a)) if a[i] != a[i - 1]]
    r.append(len(a))
    return r


def _dedup(a):
    r = [a[0]]
    for i in range(1, len(a)):
        if a[i] != a[i - 1]:
            r.append(a[i])
    return r


def aggregate(data: dict, output_path: str | None = None, window_size: int = 200) -> dict:
    out = {}
    for key, value in data.items():
        pred = np.asarray(value["pred"])
        gt = list(value["gt"])
        new = np.zeros_like(pred)
        for s in range(0, len(pred), window_size):
            e = min(s + window_size, len(pred))
            new[s:e] = np.argmax(np.bincount(pred[s:e]))       # ties: lowest class id
        out[key] = {"pred": [int(v) for v in _dedup(list(new))], "gt": [int(v) for v in _dedup(gt)],
                    "changes_pred": _changes(list(new)), "changes_gt": _changes(gt)}
    if output_path:
        with open(output_path, "w") as fp:
            json.dump(out, fp)
    return out


OVERFLOW_FULL, OVERFLOW_BAD_ID = 1, 2          # bits of a stream-pool record's `overflow` word (csrc/stream_pool.hip)


class OnlineRecord:
    """Host model of one slot's vote record in a stream pool (csrc/stream_pool.hip: pool_vote_update / pool_flush), fed one id at a time:
    utils/aggregate.py:55-78 without the per-frame list.  `counts` holds the votes of the unfinished window, an event is (id, frame at
    which its window began); a full record or an id outside [0, n_classes) sets a bit of `overflow` instead of writing."""

    def __init__(self, window: int = 200, n_classes: int = 128, max_events: int = 1024):
        if window < 1 or max_events < 1 or not 1 <= n_classes <= 128:
            raise ValueError(f"OnlineRecord: window {window}, n_classes {n_classes} (1..128), max_events {max_events}")
        self.window, self.n_classes, self.max_events = int(window), int(n_classes), int(max_events)
        self.frames, self.counts, self.last_vote, self.overflow = 0, [0] * self.n_classes, None, 0
        self.event_id, self.event_start, self.voted_to = [], [], 0

    def _close_window(self, start: int):
        vote = max(range(self.n_classes), key=lambda c: (self.counts[c], -c))        # np.argmax(np.bincount(.)): the lowest id wins a tie
        self.counts = [0] * self.n_classes
        if vote != self.last_vote:
            if len(self.event_id) < self.max_events:
                self.event_id.append(vote)
                self.event_start.append(start)
            else:
                self.overflow |= OVERFLOW_FULL
        self.last_vote, self.voted_to = vote, self.frames

    def push(self, idx: int):
        idx = int(idx)
        if not 0 <= idx < self.n_classes:
            self.overflow |= OVERFLOW_BAD_ID
            return
        self.counts[idx] += 1
        self.frames += 1
        if self.frames % self.window == 0:
            self._close_window(self.frames - self.window)

    def push_frames(self, ids):
        """a burst: the host model of the pool's K-frame commit (csrc/stream_pool.hip: pool_commit) - the slot's lane takes the
        ids in frame order, so a window may end inside the burst any number of times"""
        for i in ids:
            self.push(i)

    def flush(self):
        """the reference's shorter last window (aggregate.py:57-58: e = min(s + window, len))"""
        rest = self.frames % self.window
        if rest and any(self.counts):
            self._close_window(self.frames - rest)

    def to_words(self, n_classes=None, max_events=None) -> list:
        """the record as the device lays it out (csrc/stream_pool.hip), rec_words ints: frames | last vote + 1 | n_events | overflow |
        counts[n_classes rounded up to 4] | event_id[max_events] | event_start[max_events], rounded up to 4 words - a slot image's record
        part (csrc/pool_image.h).  n_classes / max_events: the pool's, when they are not the record's own"""
        ncls = self.n_classes if n_classes is None else int(n_classes)
        mev = self.max_events if max_events is None else int(max_events)
        if ncls < self.n_classes or mev < len(self.event_id):
            raise ValueError(f"OnlineRecord.to_words: n_classes {ncls} / max_events {mev} below the record's {self.n_classes} / {len(self.event_id)} events")
        pad = (ncls + 3) // 4 * 4
        n = len(self.event_id)
        w = [self.frames, 0 if self.last_vote is None else self.last_vote + 1, n, self.overflow]
        w += self.counts + [0] * (pad - self.n_classes)
        w += self.event_id + [0] * (mev - n) + self.event_start + [0] * (mev - n)
        return w + [0] * (-len(w) % 4)

    @classmethod
    def from_words(cls, words, window: int, n_classes: int, max_events: int) -> "OnlineRecord":
        """the record the words of `to_words` describe.  `voted_to` is not a word of the device record: it is rebuilt as the end of the
        last window the words show voted - `frames` when no count is pending (a window boundary, or a flush), else the last boundary"""
        w = [int(v) for v in words]
        pad = (int(n_classes) + 3) // 4 * 4
        need = (4 + pad + 2 * int(max_events) + 3) // 4 * 4
        if len(w) < need:
            raise ValueError(f"OnlineRecord.from_words: {len(w)} words, a record of {n_classes} classes and {max_events} events has {need}")
        rec = cls(window, n_classes, max_events)
        n = w[2]
        if not 0 <= n <= rec.max_events:
            raise ValueError(f"OnlineRecord.from_words: n_events {n} (0..{rec.max_events})")
        rec.frames, rec.last_vote, rec.overflow = w[0], (w[1] - 1 if w[1] else None), w[3]
        rec.counts = w[4:4 + rec.n_classes]
        rec.event_id, rec.event_start = w[4 + pad:4 + pad + n], w[4 + pad + rec.max_events:4 + pad + rec.max_events + n]
        rec.voted_to = 0 if rec.last_vote is None else rec.frames if not any(rec.counts) else rec.frames - rec.frames % rec.window
        return rec

    def result(self) -> dict:
        """{'pred', 'changes_pred'} of the windows voted so far (an unfinished window counts once flushed) and the frames fed"""
        return {"pred": list(self.event_id), "changes_pred": list(self.event_start[1:]) + [self.voted_to], "frames": self.frames}


def aggregate_online(ids, window: int = 200, n_classes: int = 128, max_events: int = 1 << 30, bursts=None) -> dict:
    """`aggregate`'s 'pred' / 'changes_pred' of one stream from its per-frame ids, fed one id at a time through the record a stream pool
    keeps per slot and flushed at the end.  bursts: an int K or a sequence of burst sizes (cycled; the last burst is whatever is left) -
    the ids are fed as StreamPool.push_frames feeds them, K at a time; the result does not depend on it."""
    rec = OnlineRecord(window, n_classes, max_events)
    ids = list(ids)
    if bursts is None:
        for i in ids:
            rec.push(i)
    else:
        sizes = [int(bursts)] if isinstance(bursts, int) else [int(b) for b in bursts]
        if not sizes or min(sizes) < 1:
            raise ValueError(f"aggregate_online: burst sizes {sizes} (each >= 1)")
        at, k = 0, 0
        while at < len(ids):
            rec.push_frames(ids[at:at + sizes[k % len(sizes)]])
            at += sizes[k % len(sizes)]
            k += 1
    rec.flush()
    if rec.overflow:
        raise ValueError(f"aggregate_online: overflow {rec.overflow} (1: more than {max_events} events, 2: an id outside [0, {n_classes}))")
    r = rec.result()
    return {"pred": r["pred"], "changes_pred": r["changes_pred"]}


def aggregate_device(preds: dict, gts: dict, output_path: str | None = None, window_size: int = 200, n_classes: int | None = None) -> dict:
    """preds: {vid: int32 CUDA tensor [T]} (per-frame argmax on the device); gts: {vid: sequence of per-frame ground-truth ids}.
    n_classes: the model's num_classes (ids outside [0, n_classes) are an error, as np.bincount's negative ids are in
    utils/aggregate.py:60); None = 128, the kernel's limit.  Same result dict as `aggregate` / utils/aggregate.py:46-90."""
    if n_classes is None:
        n_classes = 128
    import ctypes as C

    import torch

    from . import _lib
    from ._lib import PregoError, check
    from .engine import _stream_ptr
    lib = _lib.load()
    votes = {}
    for key, pred in preds.items():
        if not pred.is_cuda or pred.dtype != torch.int32 or not pred.is_contiguous() or pred.dim() != 1:
            raise PregoError(f"aggregate_device: pred[{key!r}] must be a contiguous int32 CUDA vector")
        T = pred.numel()
        v = torch.empty(((T + window_size - 1) // window_size,), dtype=torch.int32, device=pred.device)
        with torch.cuda.device(pred.device):
            check(lib.prego_window_vote(C.c_void_p(pred.data_ptr()), T, window_size, n_classes, C.c_void_p(v.data_ptr()),
                                        C.c_void_p(_stream_ptr(pred.device))))
        votes[key] = (v, T)
    out = {}
    for key, (v, T) in votes.items():
        w = v.cpu().numpy()
        if (w < 0).any():
            raise PregoError(f"aggregate_device: pred[{key!r}] holds a class id outside [0, {n_classes}) "
                             "(np.bincount of utils/aggregate.py:60 would raise / count a class the model does not have)")
        gt = list(gts[key])
        # the per-frame sequence is constant inside a window: duplicates and change points follow from the window values
        keep = np.concatenate(([True], w[1:] != w[:-1]))
        changes = [int(i) * window_size for i in np.nonzero(keep)[0][1:]] + [T]
        out[key] = {"pred": [int(x) for x in w[keep]], "gt": [int(x) for x in _dedup(gt)], "changes_pred": changes,
                    "changes_gt": _changes(gt)}
    if output_path:
        with open(output_path, "w") as fp:
            json.dump(out, fp)
    return out
