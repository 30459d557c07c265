"""What `Evaluate` keeps in device memory between calls (cfg['eval_cache_device'], prego_amd/evaluate.py).

`main.py` evaluates the whole test set after every epoch: the weights change between those calls, the test features do not.  The first
call with the switch on (the FILLING call) runs as ever and leaves every video's features in HBM in the form the next forward reads
them; every later call on the same loader cuts its batches from here - the loader is not iterated, nothing crosses the link.

Held per video, in the loader's order: the feature tensors (flow only where the video shipped one), the targets in the device form
`Evaluate._targets_to_device` makes, the host-side gt id array of the output JSON, and (name, frames, loader position).

Feature form: a model with `engine()` and compute_dtype 'bf16' / 'fp16' reads 16-bit operands, so that type is kept - a feeder that ships
it already (cfg['feature_dtype']) has its device tensor kept as it is, fp32 features are converted by `prego_cast_features`
(csrc/feature_cache.hip), enqueued on the compute stream behind the forward that read them.  That kernel applies the conversion the
forward's pack kernels apply to an fp32 row, so the cached operand is bit for bit what the fp32-fed forward multiplied, and a clip's
result does not depend on how a call is batched or which pass runs it: a cached call returns the bits of the filling call.  Every
other model keeps the fp32 tensors `Evaluate._features` shipped.

The cache belongs to one key - the loader's dataset OBJECT, the model's feature signature, (world, rank), the device - and is dropped
and refilled when the key differs.  Features changed IN PLACE inside the same dataset object are not seen: call
`Evaluate.drop_cache()` after such a change."""
from __future__ import annotations

import ctypes as C
import weakref
from typing import NamedTuple, Optional

import torch

_NAMES = {torch.float16: "fp16", torch.bfloat16: "bf16", torch.float32: "fp32"}


class EvalVideo(NamedTuple):
    """one video as Evaluate batches it: from the loader (host tensors) or from this cache (device tensors)"""
    features: torch.Tensor               # [T, D]
    flow: Optional[torch.Tensor]         # [T, D], or None: the flow half is all zeros and never shipped
    target: torch.Tensor                 # the loader's rows [T, C]; in the cache the device form (class ids [T] where the rows are one-hot)
    name: str
    pos: int                             # position in the loader's order
    item: int                            # the loader item it came in


class EvalFeatureCache:
    def __init__(self, max_bytes=None):
        self.max_bytes = None if max_bytes is None else int(max_bytes)     # None: half of the free device memory at the first flush
        self.logger = None
        self.drop()

    def drop(self, state: str = "empty", reason=None):
        """release everything; `state` 'disabled' keeps the key, so that calls on the same loader do not fill again"""
        self.state, self.reason = state, reason
        self.filling = False
        self.entries = []              # EvalVideo, device tensors
        self.gt_ids = {}               # name -> int array: the "gt" list of the output JSON
        self.bytes, self.frames, self.dtype, self.budget = 0, 0, None, None
        if state != "disabled":
            self._dataset, self._sig = None, None

    def info(self) -> dict:
        return dict(enabled=True, state=self.state, reason=self.reason, videos=len(self.entries), frames=self.frames, bytes=self.bytes,
                    dtype=_NAMES.get(self.dtype))

    # -- one Evaluate call ---------------------------------------------------------------------------------------------------------
    def begin(self, dataset, sig, device, keep_dtype, logger) -> bool:
        """True: this call runs from the cache.  False: from the loader - and fills the cache unless it is disabled for this key."""
        self.logger = logger
        if device.type != "cuda":
            self.drop()
            self.state, self.reason = "disabled", "cpu"
            return False
        same = self._dataset is not None and self._dataset() is dataset and self._sig == sig
        if same and self.state == "filled":
            return True
        if same and self.state == "disabled":
            return False
        self.drop()
        try:
            self._dataset = weakref.ref(dataset)
        except TypeError:              # a plain list / tuple as the loader: held strongly, which is what makes its identity a key
            self._dataset = lambda _d=dataset: _d
        self._sig, self.dtype, self.filling = sig, keep_dtype, True
        return False

    def commit(self):
        if self.filling:
            self.filling, self.state = False, "filled"
            self.logger.info(f"eval cache: {len(self.entries)} videos, {self.frames} frames, {self.bytes} bytes of {_NAMES.get(self.dtype)} "
                             f"features stay in device memory")

    def abort(self):
        """the filling call raised: a partly filled cache is no cache"""
        if self.filling:
            self.drop()

    def videos(self):
        """the cached videos as Evaluate's loop takes them: one list per loader item"""
        group = []
        for e in self.entries:
            if group and group[-1].item != e.item:
                yield group
                group = []
            group.append(e)
        if group:
            yield group

    # -- filling -------------------------------------------------------------------------------------------------------------------
    def _kept(self, x, device):
        """x in the kept dtype: itself, or - fp32 features of a 16-bit engine - its conversion, enqueued on the current stream"""
        if x.dtype == self.dtype:
            return x
        from . import _lib
        out = torch.empty(x.shape, dtype=self.dtype, device=device)
        if x.numel():
            with torch.cuda.device(device):
                _lib.check(_lib.load().prego_cast_features(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), x.numel(),
                                                           _lib.PREGO_F16 if self.dtype == torch.float16 else _lib.PREGO_BF16,
                                                           C.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
        return out

    def retain(self, items, rgb, flow, targets, device):
        """one flushed batch: `items` as Evaluate batched them, rgb / flow (None, or None per video) / targets as its forward read them on
        the device.  Bytes are counted video by video; the video that would pass the budget releases everything and disables the cache."""
        if not self.filling:
            return
        if self.budget is None:
            self.budget = self.max_bytes if self.max_bytes is not None else torch.cuda.mem_get_info(device)[0] // 2
        size = torch.empty((), dtype=self.dtype).element_size()
        for i, it in enumerate(items):
            fl = None if flow is None else flow[i]
            feats = [rgb[i]] + ([fl] if fl is not None else [])
            if any(x.dtype != self.dtype and (x.dtype != torch.float32 or x.numel() % 8 or x.data_ptr() % 16) for x in feats):
                return self._disable(f"video {it.name!r}: {rgb[i].dtype} features that prego_cast_features does not take")
            need = sum(x.numel() for x in feats) * size + targets[i].numel() * targets[i].element_size()
            if self.bytes + need > self.budget:
                return self._disable(f"budget: video {it.name!r} needs {need} bytes on top of {self.bytes}, eval_cache_max_bytes is {self.budget}")
            kept = [self._kept(x, device) for x in feats]
            self.entries.append(it._replace(features=kept[0], flow=kept[1] if fl is not None else None, target=targets[i]))
            self.bytes += need
            self.frames += int(rgb[i].shape[0])

    def _disable(self, reason):
        self.drop("disabled", reason)
        self.logger.info(f"eval cache disabled ({reason}): this and later calls run from the loader")
