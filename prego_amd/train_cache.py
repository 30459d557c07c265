"""The training set in device memory (cfg['train_cache_device'], off by default): every training batch is cut by one kernel launch.

`main.py` alternates a training epoch with an `Evaluate` call.  The training features do not change between steps or epochs, only the
choice of windows does - yet the loader slices 16 windows out of host arrays, stacks them, pins them and ships them over the link at
every step.  With the switch on, the training set is uploaded once and a batch is `prego_gather_windows` (csrc/train_cache.hip): the same
tensors, bit for bit and in the same order, that `build_data_loader`'s loader delivers under the same seeds.  Model, criterion, trainers
and optimizer see ordinary CUDA tensors and cannot tell the difference (`trainer._device_batches`: `.to(device)` is the identity).

Layout (TrainWindowCache).  The datasets keep every training video with window_size - 1 zero rows in front (dataset.py:53-55); the cache
holds the videos WITHOUT that pad, one after the other: rgb_rows [R, d_rgb] fp32, flow_rows [R, d_flow] fp32 (absent for the zero-flow
config, whose flow batch is a zero tensor made once), and the targets as int32 class ids [R] where every row of every video is all-zero
(-1) or has a single 1.0 (the id) - else as dense fp32 rows [R, C].  vid_row0 / vid_len [V] say where a video's rows are.

Row rule (gather_numpy is the model, the kernel the implementation).  A window is (video v, start s) with s in the datasets' padded
coordinates.  Row r of the window is padded row p = s + r, row l of its ant_target is p = s + W + l:
    p < W - 1 or p >= vid_len[v] + W - 1    a row of zeros
    otherwise                               resident row vid_row0[v] + p - (W - 1)
A PAD entry of EpochWindowSampler (index >= len(dataset): bit 31 of the table's video word) has the window's features and all-zero targets.

Order (DeviceWindowLoader).  The windows must come in the loader's order under the same RNG state, so the order is drawn by a real
DataLoader - same batch_size, same shuffle or the same EpochWindowSampler object, num_workers=0 - over a view of the dataset whose items
are their own indices.  It consumes the torch RNG exactly as the feature loader does: one base-seed draw per `__iter__`, one seed draw by
RandomSampler, everything else from private generators - and all of it before the first batch, as with the feature loader, so the
per-step dropout-seed draws of the model interleave identically.  At every `__iter__` the window table is rebuilt from `dataset.inputs`
(the phase re-draw of `_init_features()` is seen), validated on the host, and uploaded with the epoch's order, once; every `__next__` is
one launch on the current stream into fresh tensors of torch's caching allocator.

Under torch.distributed EVERY rank holds the whole training set: any rank may draw any window."""
from __future__ import annotations

import ctypes as C
import logging

import numpy as np
import torch
import torch.utils.data as data

PAD_BIT = 1 << 31
_ATTRS = ("inputs", "rgb_inputs", "flow_inputs", "target_all", "window_size")
_last = None          # the cache of the latest device_loader() call: cache_info() without an argument


# ---- the documented row rule, on the host --------------------------------------------------------------------------------------------
def resident_layout(dataset):
    """The dataset's training arrays as the cache keeps them, without copying a feature: per-video views without the front pad.
    Returns dict(vids, rgb [V views], flow [V views] or None, target [V views], vid_row0 int64 [V], vid_len int32 [V], d_rgb, d_flow,
    n_classes, n_rows).  Raises ValueError for arrays the cache does not take."""
    W = int(dataset.window_size)
    vids = list(dataset.vids)
    if not vids:
        raise ValueError("no training video")
    rgb, flow, target, lens = [], [], [], []
    for vid in vids:
        r, f, t = dataset.rgb_inputs[vid], dataset.flow_inputs[vid], dataset.target_all[vid]
        if not isinstance(r, np.ndarray) or r.dtype != np.float32 or t.dtype != np.float32 or (f is not None and f.dtype != np.float32):
            raise ValueError(f"video {vid!r}: features and targets must be fp32 numpy arrays")
        if r.shape[0] < W - 1 or t.shape[0] != r.shape[0] or (f is not None and f.shape[0] != r.shape[0]):
            raise ValueError(f"video {vid!r}: arrays are not front-padded training arrays of one length")
        rgb.append(r[W - 1:])
        flow.append(None if f is None else f[W - 1:])
        target.append(t[W - 1:])
        lens.append(r.shape[0] - (W - 1))
    if any(f is None for f in flow) != all(f is None for f in flow):
        raise ValueError("some videos have flow features and some have none")
    has_flow = flow[0] is not None
    d_rgb, n_classes = int(rgb[0].shape[1]), int(target[0].shape[1])
    d_flow = int(flow[0].shape[1]) if has_flow else 0
    if any(r.shape[1] != d_rgb for r in rgb) or any(t.shape[1] != n_classes for t in target) or \
            (has_flow and any(f.shape[1] != d_flow for f in flow)):
        raise ValueError("feature or class dimensions differ between videos")
    if d_rgb % 4 or d_flow % 4:
        raise ValueError(f"feature dimensions {d_rgb}, {d_flow}: prego_gather_windows takes multiples of 4")
    vid_len = np.asarray(lens, np.int32)
    vid_row0 = np.concatenate(([0], np.cumsum(vid_len[:-1], dtype=np.int64))).astype(np.int64)
    return dict(vids=vids, rgb=rgb, flow=flow if has_flow else None, target=target, vid_row0=vid_row0, vid_len=vid_len, d_rgb=d_rgb,
                d_flow=d_flow, n_classes=n_classes, n_rows=int(vid_len.sum(dtype=np.int64)), window_size=W)


def class_ids(target):
    """int32 class id per row of a [T, C] fp32 target (-1: an all-zero row) - or None unless every row is all-zero or has a single 1.0,
    the rows the kernel rebuilds exactly from 4 bytes.  (`prego_onehot_labels` asks the same of an eval video, without the zero rows.)"""
    nz = target != 0
    if (nz.sum(1) > 1).any() or (target[nz] != 1.0).any():
        return None
    return np.where(nz.any(1), nz.argmax(1), -1).astype(np.int32)


def resident_targets(layout):
    """(labels int32 [R], None) when every video's rows are one-hot or zero, else (None, dense fp32 [R, C])"""
    ids = []
    for t in layout["target"]:
        ids.append(class_ids(t))
        if ids[-1] is None:
            return None, np.concatenate(layout["target"], 0) if layout["n_rows"] else np.zeros((0, layout["n_classes"]), np.float32)
    return np.concatenate(ids), None


def window_table(dataset, layout, ant_len=0):
    """int32 [n_windows, 2] (video index, padded start) of dataset.inputs, every entry validated: a known video, 0 <= start, end = start
    + W and start + W + ant_len within the video's padded length."""
    W, L = layout["window_size"], int(ant_len)
    index = {vid: k for k, vid in enumerate(layout["vids"])}
    n = len(dataset.inputs)
    v = np.fromiter((index.get(it[0], -1) for it in dataset.inputs), np.int64, n)
    start = np.fromiter((it[1] for it in dataset.inputs), np.int64, n)
    end = np.fromiter((it[2] for it in dataset.inputs), np.int64, n)
    bad = (v < 0) | (start < 0) | (end != start + W) | (start + W + L > layout["vid_len"].astype(np.int64)[np.maximum(v, 0)] + W - 1)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f"window {k} {tuple(dataset.inputs[k][:3])!r}: outside the videos of the resident training set")
    table = np.stack((v, start), 1).astype(np.int32)
    return table


def epoch_table(table, order):
    """(table with the PAD entries the order needs, order as int32 indices into it).  An order index i >= n_windows is EpochWindowSampler's
    PAD entry of window i - n_windows: it becomes entry n_windows + (i - n_windows), a copy with bit 31 set in the video word."""
    n = len(table)
    order = np.asarray(order, np.int64).reshape(-1)
    if order.size and (order.min() < 0 or order.max() >= 2 * max(n, 1) or n == 0):
        raise ValueError(f"order entries outside [0, {2 * n}) for {n} windows")
    if order.size and order.max() >= n:
        pads = table.copy()
        pads[:, 0] = (pads[:, 0].astype(np.int64) | PAD_BIT).astype(np.uint32).view(np.int32)
        table = np.concatenate((table, pads), 0)
    return np.ascontiguousarray(table, np.int32), order.astype(np.int32)


def gather_numpy(layout, labels, dense, table, order, first, n, ant_len=0):
    """The row rule in numpy: (rgb [n, W, d_rgb], flow [n, W, d_flow] or None, target [n, W, C], ant_target [n, L, C] or None) for
    order[first : first + n] - what prego_gather_windows writes."""
    W, Cn, L = layout["window_size"], layout["n_classes"], int(ant_len)
    rgb_rows = np.concatenate(layout["rgb"], 0)
    flow_rows = None if layout["flow"] is None else np.concatenate(layout["flow"], 0)
    rgb = np.zeros((n, W, layout["d_rgb"]), np.float32)
    flow = None if flow_rows is None else np.zeros((n, W, layout["d_flow"]), np.float32)
    target = np.zeros((n, W, Cn), np.float32)
    ant = np.zeros((n, L, Cn), np.float32) if L else None
    for i in range(n):
        vw, s = (int(x) for x in table[order[first + i]])
        pad, v = vw < 0, vw & 0x7FFFFFFF
        for r in range(W + L):
            q = s + r - (W - 1)
            if q < 0 or q >= layout["vid_len"][v]:
                continue
            row = int(layout["vid_row0"][v]) + q
            if r < W:
                rgb[i, r] = rgb_rows[row]
                if flow is not None:
                    flow[i, r] = flow_rows[row]
            if not pad:
                out = target[i, r] if r < W else ant[i, r - W]
                if labels is None:
                    out[:] = dense[row]
                elif labels[row] >= 0:
                    out[labels[row]] = 1.0
    return rgb, flow, target, ant


# ---- the resident set ------------------------------------------------------------------------------------------------------------------
class TrainWindowCache:
    """The resident training set of one dataset object on one device.  state: 'filled' or 'disabled' (with `reason`); 'empty' after
    drop_cache() - the next epoch of a DeviceWindowLoader fills it again."""

    def __init__(self, dataset, device, max_bytes=None, logger=None):
        self.dataset, self.device = dataset, torch.device(device)
        self.max_bytes = None if max_bytes is None else int(max_bytes)        # None: half of the free device memory when filling
        self.logger = logger or logging.getLogger("prego_amd.null")
        self.ant_len = int(getattr(dataset, "anticipation_length", 0))
        self._release("empty", None)
        self.fill()

    def _release(self, state, reason):
        self.state, self.reason = state, reason
        self.rgb = self.flow = self.labels = self.dense = self.vid_row0 = self.vid_len = self.layout = None
        self.bytes = self.frames = self.videos = 0

    def _disable(self, reason):
        self._release("disabled", reason)
        self.logger.info(f"train cache disabled ({reason}): training runs from the loader")
        return False

    def drop_cache(self):
        """release the resident set; the next epoch uploads it again"""
        self._release("empty", None)

    def cache_info(self) -> dict:
        return dict(enabled=True, state=self.state, reason=self.reason, videos=self.videos, frames=self.frames, bytes=self.bytes,
                    targets=None if self.state != "filled" else ("labels" if self.labels is not None else "dense"))

    def fill(self) -> bool:
        ds = self.dataset
        missing = [a for a in _ATTRS if not hasattr(ds, a)]
        if missing:
            return self._disable(f"the dataset has no {', '.join(missing)}")
        if not getattr(ds, "training", True):
            return self._disable("not a training-mode dataset")
        try:
            lay = resident_layout(ds)
        except (ValueError, AttributeError, KeyError, TypeError) as e:
            return self._disable(str(e))
        if lay["flow"] is None and getattr(ds, "_zero_row", None) is None:
            return self._disable("a dataset without flow features and without a zero flow row")
        labels, dense = resident_targets(lay)
        R = lay["n_rows"]
        need = R * (lay["d_rgb"] + lay["d_flow"]) * 4 + (R * 4 if labels is not None else R * lay["n_classes"] * 4) + 12 * len(lay["vids"])
        cuda = self.device.type == "cuda"
        budget = self.max_bytes if self.max_bytes is not None else (torch.cuda.mem_get_info(self.device)[0] // 2 if cuda else need)
        if need > budget:
            return self._disable(f"budget: the training set needs {need} bytes, train_cache_max_bytes is {budget}")
        if not cuda:
            return self._disable("cpu")
        dev = self.device
        self.rgb = torch.empty((R, lay["d_rgb"]), dtype=torch.float32, device=dev)
        self.flow = None if lay["flow"] is None else torch.empty((R, lay["d_flow"]), dtype=torch.float32, device=dev)
        for k, r0 in enumerate(lay["vid_row0"].tolist()):
            n = int(lay["vid_len"][k])
            if n:
                self.rgb[r0:r0 + n].copy_(torch.from_numpy(lay["rgb"][k]))
                if self.flow is not None:
                    self.flow[r0:r0 + n].copy_(torch.from_numpy(lay["flow"][k]))
        self.labels = None if labels is None else torch.from_numpy(labels).to(dev)
        self.dense = None if dense is None else torch.from_numpy(dense).to(dev)
        self.vid_row0, self.vid_len = torch.from_numpy(lay["vid_row0"]).to(dev), torch.from_numpy(lay["vid_len"]).to(dev)
        self.layout = dict(lay, rgb=None, flow=None, target=None)        # geometry only: the host arrays stay the dataset's
        self.state, self.reason, self.bytes, self.frames, self.videos = "filled", None, need, R, len(lay["vids"])
        self.logger.info(f"train cache: {self.videos} videos, {R} frames, {need} bytes stay in device memory "
                         f"({'class ids' if labels is not None else 'dense targets'})")
        return True

    def gather(self, table, n_windows, order, first, n, zero_flow=None):
        """one batch: (rgb, flow, target, ant_target or None) of order[first : first + n], one launch on the current stream"""
        from . import _lib
        lay, dev, L = self.layout, self.device, self.ant_len
        W, Cn = lay["window_size"], lay["n_classes"]
        rgb = torch.empty((n, W, lay["d_rgb"]), dtype=torch.float32, device=dev)
        flow = zero_flow if self.flow is None else torch.empty((n, W, lay["d_flow"]), dtype=torch.float32, device=dev)
        target = torch.empty((n, W, Cn), dtype=torch.float32, device=dev)
        ant = torch.empty((n, L, Cn), dtype=torch.float32, device=dev) if L else None
        ptr = lambda t: C.c_void_p(None if t is None else t.data_ptr())      # noqa: E731
        with torch.cuda.device(dev):
            _lib.check(_lib.load().prego_gather_windows(
                ptr(self.rgb), ptr(self.flow), lay["n_rows"], lay["d_rgb"], lay["d_flow"], ptr(self.labels), ptr(self.dense),
                ptr(self.vid_row0), ptr(self.vid_len), self.videos, ptr(table), n_windows, ptr(order), order.numel(), first, n, W, Cn, L,
                ptr(rgb), ptr(None if self.flow is None else flow), ptr(target), ptr(ant),
                C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return rgb, flow, target, ant


# ---- the loader ------------------------------------------------------------------------------------------------------------------------
class _IndexView(data.Dataset):
    """the dataset as the samplers see it - its current length - with items that are their own index"""

    def __init__(self, dataset):
        self.dataset = dataset

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, index):
        return index


def index_loader(trainloader):
    """A DataLoader that yields the index batches of `trainloader` under the same RNG state: same batch_size, the same kind of default
    sampler (RandomSampler / SequentialSampler over the dataset's CURRENT length) or the very sampler object otherwise."""
    s = trainloader.sampler
    view = _IndexView(trainloader.dataset)
    if type(s) is data.RandomSampler and s.generator is None and not s.replacement and s._num_samples is None:
        kw = dict(shuffle=True)
    elif type(s) is data.SequentialSampler:
        kw = dict(shuffle=False)
    else:
        kw = dict(sampler=s)
    return data.DataLoader(view, batch_size=trainloader.batch_size, num_workers=0, drop_last=trainloader.drop_last,
                           generator=trainloader.generator, **kw)


class DeviceWindowLoader:
    """What the trainer iterates instead of the feature loader: batches (rgb, flow, target, vids, starts, ends) for
    StepRecognitionDataset, (rgb, flow, target, ant_target) for AnticipationDataset, the leading tensors on the device."""

    def __init__(self, trainloader, cache: TrainWindowCache):
        self.loader, self.cache = trainloader, cache
        self.dataset, self.batch_size = trainloader.dataset, trainloader.batch_size
        self._index = index_loader(trainloader)
        self.sampler = self._index.sampler           # the loader's own sampler object unless it is a default Random / SequentialSampler
        self._zero_flow = None

    def __len__(self):
        return len(self._index)

    def cache_info(self):
        return self.cache.cache_info()

    def drop_cache(self):
        self.cache.drop_cache()

    def __iter__(self):
        cache = self.cache
        if cache.state == "empty":
            cache.fill()
        if cache.state != "filled":            # disabled on a refill: the feature loader, which draws the same order
            return iter(self.loader)
        return self._epoch()

    def _epoch(self):
        """everything an epoch does once, NOW (not at the first batch): the order is drawn - every RNG draw of the epoch -, the window
        table is built from the dataset's current windows and validated, both are uploaded"""
        cache, ds = self.cache, self.dataset
        lay, dev, bs = cache.layout, cache.device, self.batch_size
        if list(ds.vids) != lay["vids"]:
            raise ValueError("the dataset's video list changed under the train cache: call drop_cache()")
        inputs = ds.inputs
        host_table = window_table(ds, lay, cache.ant_len)
        order = [int(i) for batch in self._index for i in batch.tolist()]
        table, order32 = epoch_table(host_table, order)
        table_d, order_d = torch.from_numpy(table).to(dev), torch.from_numpy(order32).to(dev)
        if cache.flow is None and (self._zero_flow is None or self._zero_flow.shape[0] < bs):
            self._zero_flow = torch.zeros((bs, lay["window_size"], int(ds._zero_row.shape[1])), dtype=torch.float32, device=dev)
        return self._batches(inputs, order, table_d, len(table), order_d)

    def _batches(self, inputs, order, table_d, n_table, order_d):
        cache, bs, n_windows = self.cache, self.batch_size, len(inputs)
        oad = not hasattr(self.dataset, "anticipation_length")
        for first in range(0, len(order), bs):
            n = min(bs, len(order) - first)
            zf = None if cache.flow is not None else self._zero_flow[:n]
            rgb, flow, target, ant = cache.gather(table_d, n_table, order_d, first, n, zf)        # one launch, fresh tensors
            if oad:
                items = [inputs[i - n_windows if i >= n_windows else i] for i in order[first:first + n]]
                yield [rgb, flow, target, [it[0] for it in items], torch.tensor([it[1] for it in items]),
                       torch.tensor([it[2] for it in items])]
            else:
                yield [rgb, flow, target, ant if ant is not None else torch.empty((n, 0, target.shape[2]), device=target.device)]


def device_loader(trainloader, device, cfg, logger=None):
    """`trainloader` with its training set in device memory (a DeviceWindowLoader) - or `trainloader` itself when the cache disables
    itself: the set is over cfg['train_cache_max_bytes'] (default: half of the free device memory), or the dataset is not one of the
    two window datasets.  The reason is logged and kept for cache_info()."""
    global _last
    from .config import TRAIN_CACHE_DEFAULTS
    cache = TrainWindowCache(trainloader.dataset, device, cfg.get("train_cache_max_bytes", TRAIN_CACHE_DEFAULTS["train_cache_max_bytes"]), logger)
    _last = cache
    return DeviceWindowLoader(trainloader, cache) if cache.state == "filled" else trainloader


def cache_info() -> dict:
    """of the latest device_loader() call of this process"""
    if _last is None:
        return dict(enabled=False, state="disabled", reason="cfg['train_cache_device'] is off", videos=0, frames=0, bytes=0, targets=None)
    return _last.cache_info()


def drop_cache():
    if _last is not None:
        _last.drop_cache()
