"""`Evaluate` ("OAD") behind the reference's EVAL registry (step_recognition/trainer/eval.py:15-84):
the per-frame inference loop of `main.py --eval`.

Same call contract: `Evaluate(cfg)(model, dataloader, logger, device) -> mean_AP`, same side effect
(`output_miniRoad/output_miniROAD.json` = {vid: {"pred": [...], "gt": [...]}} when cfg['eval'] is set,
eval.py:51-65).  What changes is how the loop runs: the reference pushes ONE video per forward through
a batch-1 GRU and copies [T, C] probabilities back per video; here whole videos are batched (up to the
engine's clip capacity / a frame budget), advanced together by the ragged HIP path, and argmax is
taken on the device.  The FPS log line is computed correctly (the reference shadows its timer with the
loader's `start` field, eval.py:35-36,77-80)."""
from __future__ import annotations

import ctypes as C
import json
import os
import time
from collections import namedtuple
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn

from . import _lib
from .aggregate import aggregate_device
from .eval_cache import EvalFeatureCache, EvalVideo
from ._lib import PregoError, check
from .metrics import (N_STAGES, perframe_ap_raw, perframe_ap_raw_device, perframe_average_precision, perframe_average_precision_device,
                      perstage_average_precision_device, perstage_report, report_from_raw)
from .postprocessing import ThumosPostprocessing, thumos_postprocessing_device
from .registry import EVAL
from .decode import DECODE_MAX_CLASSES, uniform_transitions, viterbi_decode_device
from .segmental import segmental_scores_device


def _thumos_postprocessing(cfg, is_thumos: bool):
    """cfg['eval_thumos_postprocessing'] (not a reference key, off by default): the reference applies thumos_postprocessing in front of
    every metric of a THUMOS data set (trainer/eval.py:19-21, 92-93); here a THUMOS data set is refused without the key and evaluated
    with it.  cfg['eval_thumos_smooth'] / ['eval_thumos_switch'] default to False: the reference calls the function with its defaults."""
    on = bool(cfg.get("eval_thumos_postprocessing", False))
    if is_thumos and not on:
        raise NotImplementedError("THUMOS post-processing is outside the PREGO datasets; cfg['eval_thumos_postprocessing'] = True "
                                  "evaluates a THUMOS data set with it (prego_amd/postprocessing.py)")
    if on and not is_thumos:
        raise PregoError(f"cfg['eval_thumos_postprocessing'] is for THUMOS data sets; data_name is {cfg['data_name']!r}")
    return ThumosPostprocessing(bool(cfg.get("eval_thumos_smooth", False)), bool(cfg.get("eval_thumos_switch", False))) if on else None


def split_by_length(frames, element_size, fraction=None):
    """The parts (lists of batch indices) a batch that is copied and then forwarded goes in.  A batch runs as long as its longest video's
    recurrence and its H2D copy would sit in front of that, so a batch of 16 or more videos goes in two parts ordered by length: the few
    longest videos first (little to copy, the long critical path), then the bulk of the bytes, whose copy runs under the first part's
    recurrence.  fraction: share of the frames in the first part - its forward should last about as long as the second part's copy.
    Measured on the 60-video bench set (scripts/eval_e2e_bench.py): fp32 features 0.2: 4.23, 0.5: 4.72, 0.6: 4.41 M frames/s;
    16-bit features (half the bytes) 0.2: 5.87, 0.5: 5.62 - the defaults by element size."""
    order = list(range(len(frames)))
    if len(frames) < 16:
        return [order]
    order.sort(key=lambda i: -frames[i])
    if fraction is None:
        fraction = 0.5 if element_size >= 4 else 0.2
    budget, k, acc = float(fraction) * sum(frames), 0, 0
    while k < len(order) - 1 and acc + frames[order[k]] <= budget:
        acc += frames[order[k]]
        k += 1
    return [order[:k], order[k:]] if k >= 1 else [order]


# what each of the three enqueue paths returns, lists in the order of the videos it was given: the forward's outputs, the targets in their
# device form, the features as the forward read them on the device (flow: None, or per video a tensor or None), _targets_to_device's count
# of post-processing-kept rows, and what must stay alive until the launch has run (pinned sources of async copies, feed events)
_Enqueued = namedtuple("_Enqueued", "probs argmax targets rgb flow n_valid keep")


@dataclass
class _Launched:
    """a batch whose launch is out (_flush) and whose host half (_collect) is due one batch later"""
    videos: list                         # per video, in the loader's order: (name, probs, argmax, target)
    link_fed: bool
    n_valid: Optional[int] = 0           # the rows of this batch the THUMOS post-processing keeps, counted on the host; None: not known
    ids: Optional[torch.Tensor] = None   # [pred | gt][frame]: pinned, valid behind `ids_ready` (a CPU box: the tensor itself, no event)
    ids_ready: Optional[torch.cuda.Event] = None
    text: Optional[torch.Tensor] = None  # the ids' JSON text made on the device (prego_format_ids), pinned; text_bad[0] != 0: not usable
    text_bad: Optional[torch.Tensor] = None
    fed: list = field(default_factory=list)      # a cache-filling call: per video (rgb, flow or None) on the device, until _collect
    # alive until the record goes, behind _collect: the loader's tensors, device sources of async copies, pinned label buffers, feed events
    keep: list = field(default_factory=list)


@dataclass
class _Pass:
    """what one eval pass accumulates between its batches and hands to its ending"""
    mark: Callable                       # mark(name): phase_log entry
    t_begin: float
    json_parts: Optional[list]           # per-video JSON text, formatted batch by batch; None: written from `output` at the end
    n_valid: Optional[int]               # the THUMOS post-processing's row hint: the batches' counts summed; None: no hint
    output: dict = field(default_factory=dict)
    # the [T, C] score and target matrices of the videos, taken at launch time: they stay torch tensors on the model's device (one entry
    # per video, concatenated once at the end; the reference extends Python lists by one row object per frame, eval.py:46-49), so the
    # metric's kernels can be enqueued behind the last forward before the host waits for anything
    pred_scores: list = field(default_factory=list)
    gt_targets: list = field(default_factory=list)
    argmax_ids: list = field(default_factory=list)      # cfg['eval_segmental']: the videos' device argmax, in the order of pred_scores
    video_ids: list = field(default_factory=list)       # cfg['eval_decode']: the videos' names, in the order of pred_scores
    per_video: list = field(default_factory=list)       # (loader position, n_frames) to restore the loader's order on rank 0
    pending: Optional[_Launched] = None  # the batch whose launch is out and whose host half (_collect) is still due
    metric_inputs: Optional[tuple] = None
    finish_ap: Optional[Callable] = None
    finish_ps: Optional[Callable] = None
    finish_seg: Optional[Callable] = None
    finish_decode: Optional[Callable] = None


@EVAL.register("OAD")
class Evaluate(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        # thumos_postprocessing applies to THUMOS only (eval.py:19-21): None, or a ThumosPostprocessing under cfg['eval_thumos_postprocessing']
        self.data_processing = _thumos_postprocessing(cfg, "THUMOS" in cfg["data_name"])
        self.metric = cfg["metric"]
        if self.metric not in ("AP", "cAP"):          # known before the eval pass runs, not after it (utils/metrics.py:38-44)
            raise RuntimeError(f"Unknown metrics: {self.metric}")
        self.cfg = cfg
        self.all_class_names = json.load(open(cfg["video_list_path"]))[cfg["data_name"].split("_")[0]]["class_index"]
        # frames per forward.  The loop is pipelined one batch deep (_step: _flush / _collect): while batch k's features cross the link and
        # its forward runs, the host waits for batch k - 1's ids and formats their JSON text.  Measured on the 182-video bench set
        # (2.3 M frames, 16-bit features): ONE batch 226 ms, two batches of 1.2 M frames 238 ms - every forward pays its own fill and tail
        # (~12 ms) and the text it hides is 6 ms -, so the default keeps an eval set of this size in one forward
        self.max_frames_per_batch = int(cfg.get("eval_frames_per_batch", 4_000_000))
        if "eval_piece_frames" in cfg:
            self.PIECE_FRAMES = int(cfg["eval_piece_frames"])
        self.output_dir = cfg.get("eval_output_dir", "output_miniRoad")
        self.last_fps = None
        self._copy_stream = None             # side stream for the H2D feature copies (double buffering against the compute stream)
        self._ap_stream = None               # side stream of the metric's kernels (enqueued behind the last forward)
        # cfg['eval_cache_device'] (not a reference key): the eval set's features stay in device memory between calls (eval_cache.py)
        self._cache = EvalFeatureCache(cfg.get("eval_cache_max_bytes")) if cfg.get("eval_cache_device", False) else None
        self.last_source = None              # "loader" | "cache": where the last call took its features from
        # cfg['eval_perstage'] (not a reference key, off by default): the per-stage AP report of the pass (utils/metrics.py:64-130 with
        # metrics='AP', `prego_perstage_ap_labels`) is kept here and each stage's mean is logged; what eval returns and writes is unchanged.
        # cfg['eval_perstage_metric']: 'AP' (the default, whatever cfg['metric'] is) or 'cAP' (`prego_perstage_cap_labels`)
        self.perstage = bool(cfg.get("eval_perstage", False))
        self.perstage_metric = cfg.get("eval_perstage_metric", "AP")
        if self.perstage_metric not in ("AP", "cAP"):
            raise RuntimeError(f"Unknown eval_perstage_metric: {self.perstage_metric}")
        self.last_perstage = None
        # cfg['eval_segmental'] (not a reference key, off by default): the segmental metrics of the pass - MoF, segmental Edit, segmental
        # F1@{10,25,50} (`prego_segmental_scores`) - on the per-frame argmax ("frames") and on the sequence the anticipator reads, the
        # cfg['eval_segmental_window']-frame majority vote expanded back to frames ("vote"); kept in `last_segmental` and logged.  They
        # are computed from the argmax of the RAW scores: cfg['eval_thumos_postprocessing'] does not feed them.
        self.segmental = bool(cfg.get("eval_segmental", False))
        self.segmental_window = int(cfg.get("eval_segmental_window", 200))
        self.last_segmental = None
        # cfg['eval_decode'] (not a reference key, off by default): the pass's score matrix decoded on the device by a first-order Viterbi
        # pass (`prego_viterbi_decode`: emission cost = the quantised -log2 of the score, cfg['eval_decode_switch_cost'] per change of
        # label, cfg['eval_decode_stay_cost'] per frame that keeps it, or cfg['eval_decode_transitions'] = (trans, init), e.g.
        # ProcedureModel.transition_costs) and the segmental metrics of the decoded ids; kept in `last_decode` and logged, nothing else
        # about the pass changes.  Costs are in 1/256 bit.  The default of 2048 (8 bits per switch) is NOT tuned: there are no real
        # features here to tune it on.
        self.decode = bool(cfg.get("eval_decode", False))
        self.decode_switch_cost = int(cfg.get("eval_decode_switch_cost", 2048))
        self.decode_stay_cost = int(cfg.get("eval_decode_stay_cost", 0))
        self.decode_transitions = cfg.get("eval_decode_transitions")
        self.last_decode = None
        self.last_metric_path = None         # "device" | "host": where the last call computed cfg['metric']

    @staticmethod
    def _new_copy_stream(dev):
        """The H2D copies must run BESIDE the forward's kernels.  HIP maps streams onto a handful of hardware queues round-robin in
        creation order, and two streams that share a queue execute in submission order: in a process that had created a few streams
        before (bench.py after its main pass) the copy stream landed on the compute stream's queue and the whole transfer ran in FRONT
        of the forward (149 instead of 89 ms for the 60-video set).  A queue has one priority, so a high-priority stream never shares
        the queue of the normal-priority compute stream."""
        return torch.cuda.Stream(dev, priority=-1)

    def _zero_flow(self, model, dataloader=None) -> bool:
        """the flow half of EVERY video is identically zero - never shipped, its half of layer1's K never multiplied (exact).  Known
        from what the data IS, not from a config string: the model was told so (cfg['assume_zero_flow']), or the loader's dataset
        says it zeroes the flow stream (StepRecognitionDataset.zero_flow = the reference's dataset.py:63-69 behaviour).  A loader
        that supplies real flow under the same flow_type name has its flow used.  Single tensors are also checked, see _flow_zero."""
        known_zero = bool(getattr(model, "assume_zero_flow", False)) or bool(getattr(getattr(dataloader, "dataset", None), "zero_flow", False))
        return known_zero and bool(getattr(model, "use_rgb", True)) and bool(self.cfg.get("eval_skip_zero_flow", True))

    def _flow_zero(self, model, flow) -> bool:
        """one video's flow tensor [T, D] is provably all zeros at no cost: a stride-0 expansion of a zero row (what a dataset that
        zeroes the flow stream hands out before collation)"""
        if not (bool(getattr(model, "use_rgb", True)) and bool(self.cfg.get("eval_skip_zero_flow", True))):
            return False
        return flow.dim() == 2 and flow.shape[0] > 0 and (flow.stride(0) == 0 or flow.shape[0] == 1) and not bool(flow[0].any())

    @staticmethod
    def _features(model, x):
        """fp32 as the reference ships them (eval.py:40-45), or - when the feeder already holds the model's 16-bit operand type
        (cfg['feature_dtype']) - unchanged: half the PCIe bytes per frame, no conversion on either side"""
        keep = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(getattr(model, "compute_dtype", None))
        return x.contiguous() if (keep is not None and x.dtype == keep) else x.float().contiguous()

    @staticmethod
    def _json_int_lists(output, as_parts: bool = False):
        """the reference's output file ({vid: {"pred": [...], "gt": [...]}}, eval.py:59-65) written from the int arrays directly:
        class ids through a table of pre-formatted byte strings (json.dump walks 2 x frames Python ints one at a time: 0.25 s for
        0.8 M frames, five times the forward pass).  Same JSON value; numbers are padded with blanks, which JSON allows."""
        lut4 = np.frombuffer(b"".join(("%3d," % i).encode() for i in range(100)), dtype=np.uint32)         # one 4-byte gather per id < 100
        lut5 = np.frombuffer(b"".join(("%4d," % i).encode() for i in range(1000)), dtype=np.uint8).reshape(1000, 5)

        def arr(a):
            a = np.asarray(a)
            if a.size == 0:
                return b"[]"
            lo, hi = int(a.min()), int(a.max())
            if lo < 0 or hi >= 1000:
                return json.dumps(a.tolist()).encode()
            body = lut4[a].tobytes() if hi < 100 else np.take(lut5, a, axis=0).tobytes()
            return b"[" + body[:-1] + b"]"
        parts = [json.dumps(str(vid)).encode() + b': {"pred": ' + arr(v["pred"]) + b', "gt": ' + arr(v["gt"]) + b"}" for vid, v in output.items()]
        return parts if as_parts else b"{" + b", ".join(parts) + b"}"

    def _targets_to_device(self, targets, dev):
        """The loader's target rows [T, C] of a batch's videos -> device tensors, enqueued on the current (copy) stream.  Host fp32
        one-hot targets (what the reference's dataset yields) travel as ONE class id per frame: `prego_onehot_labels` reduces them in the
        loader's memory (a few host threads, while the GPU is busy with the features) and says per video whether the ids tell everything
        the rows do - 4 bytes per frame over the link instead of 4 x classes (0.79 GB for the 182-video eval set: 14 ms of a 200 ms
        pass).  Such a video's entry is an int32 vector [T]; any other video's rows are copied as they are ([T, C]).  Returns the entries,
        what must stay alive until the copies have run, and the rows the THUMOS post-processing keeps of them (None: not counted)."""
        out, keep, n_valid = [None] * len(targets), [], None
        if self.data_processing is not None and all(t.device.type == "cpu" and t.dim() == 2 for t in targets):
            # the frames the THUMOS post-processing keeps, counted while the rows are in host memory: with this hint the device
            # post-processing and the metric behind it are enqueued without a wait for the count (a device target: no hint)
            n_valid = sum(self.data_processing.count_valid(t.numpy()) for t in targets)
        host = [i for i, t in enumerate(targets) if t.device.type == "cpu" and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()
                and t.shape[1] == len(self.all_class_names)]
        if host and self.cfg.get("eval_label_targets", True):
            nv = len(host)
            ptrs = (C.c_void_p * nv)(*[targets[i].data_ptr() for i in host])
            rows = (C.c_int64 * nv)(*[int(targets[i].shape[0]) for i in host])
            total = sum(int(targets[i].shape[0]) for i in host)
            labels = torch.empty(max(total, 1), dtype=torch.int32, pin_memory=dev.type == "cuda")
            flags = (C.c_int32 * nv)()
            check(_lib.load().prego_onehot_labels(nv, ptrs, rows, len(self.all_class_names), C.c_void_p(labels.data_ptr()), flags))
            labels_dev = labels.to(dev, non_blocking=True)
            keep.append(labels)                              # the pinned source of an async copy
            o = 0
            for k, i in enumerate(host):
                n = int(targets[i].shape[0])
                if flags[k]:
                    out[i] = labels_dev[o:o + n]
                o += n
        for i, t in enumerate(targets):
            if out[i] is None:
                out[i] = t.to(dev, non_blocking=True)
        return out, keep, n_valid

    def _gt_matrix(self, t):
        """a video's ground truth as the [T, C] matrix the loader gave (class-id vectors of _targets_to_device expanded again)"""
        if t.dim() == 2:
            return t
        m = torch.zeros((t.shape[0], len(self.all_class_names)), dtype=torch.float32, device=t.device)
        m[torch.arange(t.shape[0], device=t.device), t.long()] = 1
        return m

    def _enqueue(self, model, sub, device):
        """H2D of one sub-batch on the copy stream + its forward on the compute stream; nothing here waits for the GPU"""
        dev = torch.device(device)
        flows = [b.flow for b in sub]
        if all(f is None for f in flows):
            flows = None
        if dev.type == "cuda":
            # H2D on a side stream: these copies run while whatever was enqueued before is still computing (the loader's
            # pin_memory=True makes them true async DMA); the compute stream waits on one event per sub-batch
            if self._copy_stream is None:
                self._copy_stream = self._new_copy_stream(dev)
            cur = torch.cuda.current_stream(dev)
            with torch.cuda.stream(self._copy_stream):
                rgb = [b.features.to(dev, non_blocking=True) for b in sub]
                flow = None if flows is None else [None if f is None else f.to(dev, non_blocking=True) for f in flows]
                tgt, keep, n_valid = self._targets_to_device([b.target for b in sub], dev)
                ready = torch.cuda.Event()
                ready.record(self._copy_stream)
            cur.wait_event(ready)
            for t in rgb + [f for f in (flow or []) if f is not None] + tgt:
                t.record_stream(cur)         # allocated on the copy stream, consumed on the compute stream
        else:
            rgb = [b.features.to(device) for b in sub]
            flow = None if flows is None else [None if f is None else f.to(device) for f in flows]
            tgt, keep, n_valid = self._targets_to_device([b.target for b in sub], dev)
        probs, args, _ = model.forward_clips(rgb, flow, want_probs=True, want_argmax=True)
        return _Enqueued(probs, args, tgt, rgb, flow, n_valid, keep)

    @staticmethod
    def _enqueue_resident(model, batch, device=None):
        """a batch cut from the feature cache: ONE forward on the resident tensors, whatever the batch's size - nothing to copy, so nothing
        to hide behind a first part (forward_ragged provides the resident buffer and the library picks the pass, as for any
        device-resident call); the targets are in their device form already, and were never counted on the host"""
        rgb, flow = [b.features for b in batch], [b.flow for b in batch]
        flow = None if all(f is None for f in flow) else flow
        probs, args, _ = model.forward_clips(rgb, flow, want_probs=True, want_argmax=True)
        return _Enqueued(probs, args, [b.target for b in batch], rgb, flow, None, [])

    # link-fed eval: frames per H2D piece; one feed event per ~EVENT_BYTES copied.  A copy costs ~10 us of fixed time whatever its size, so
    # large pieces keep the link busier (182-video set, 16-bit features: 2 048 frames 226 ms to the last id, 4 096: 220, 8 192: 215.5) -
    # but the recurrence cannot pass a piece's first step before the piece has landed, so whatever a slot's LAST piece covers is run after
    # the link has gone idle: the tail of every video goes in TAIL_PIECE_FRAMES pieces
    PIECE_FRAMES = 8192
    TAIL_PIECE_FRAMES = 2048
    EVENT_BYTES = 64 << 20

    def _pieces_of(self, T):
        """frame ranges [a, b) one video's features are copied in"""
        P, Q = self.PIECE_FRAMES, min(self.TAIL_PIECE_FRAMES, self.PIECE_FRAMES)
        out, a = [], 0
        while T - a > P + Q:
            out.append((a, a + P))
            a += P
        while a < T:
            out.append((a, min(a + Q, T)))
            a += Q
        return out

    def _enqueue_link_fed(self, model, batch, device):
        """ONE forward over the whole batch while its features are still arriving (MROAD.link_fed_eval; pinned host features).
        The engine says at which step every video starts in its recurrence slot (plan_starts: a schedule costed for a link-bound
        feed - about frames / longest-video slots, every slot alive to the end, so rows are needed at the rate the link delivers
        them); the features are cut into pieces of PIECE_FRAMES frames, copied in the order the packed pipeline needs them
        (piece (video, a) at step start[video] + a), and a feed event is recorded every EVENT_BYTES; the library's packing stream waits
        for the events a chunk needs (set_feed_events).  The recurrence's critical path - the longest video - is paid once, with the
        copy under it, instead of copy + forward one after the other (round 3: 46 % of the PCIe floor)."""
        dev = torch.device(device)
        eng = model.engine()
        if self._copy_stream is None:
            self._copy_stream = self._new_copy_stream(dev)
        cur = torch.cuda.current_stream(dev)
        lens = [int(b.features.shape[0]) for b in batch]
        any_flow = any(b.flow is not None for b in batch)
        row_bytes = sum(int(t.shape[1]) * t.element_size() for t in (batch[0].features,) + ((next(b.flow for b in batch if b.flow is not None),) if any_flow else ()))
        start, n_steps = eng.plan_starts(lens, row_bytes)
        pieces = sorted((start[i] + a, i, a, b_) for i, T in enumerate(lens) for a, b_ in self._pieces_of(T))
        upto, events, acc = [], [], 0
        with torch.cuda.stream(self._copy_stream):
            # the destination tensors belong to the COPY stream (allocated inside its context): the copies of this batch follow the
            # previous batch's copies at once - they do not wait for the compute stream, which is still running the previous forward
            rgb = [torch.empty(b.features.shape, dtype=b.features.dtype, device=dev) for b in batch]
            flow = [None if b.flow is None else torch.empty(b.flow.shape, dtype=b.flow.dtype, device=dev) for b in batch] if any_flow else None
            for k, (need, i, a, b) in enumerate(pieces):
                rgb[i][a:b].copy_(batch[i].features[a:b], non_blocking=True)
                acc += (b - a) * int(rgb[i].shape[1]) * rgb[i].element_size()
                if flow is not None and flow[i] is not None:
                    flow[i][a:b].copy_(batch[i].flow[a:b], non_blocking=True)
                    acc += (b - a) * int(flow[i].shape[1]) * flow[i].element_size()
                last = k + 1 == len(pieces)
                if acc >= self.EVENT_BYTES or last:
                    ev = torch.cuda.Event()
                    ev.record(self._copy_stream)
                    events.append(ev)
                    upto.append(2 ** 31 - 1 if last else pieces[k + 1][0])      # every piece needed before that step has been copied
                    acc = 0
        for t in rgb + [f for f in (flow or []) if f is not None]:
            t.record_stream(cur)                               # allocated on the copy stream (inside its context), read on `cur`
        eng.set_feed_events(upto, events, row_bytes)
        try:
            probs, args, _ = model.forward_clips(rgb, flow, want_probs=True, want_argmax=True)
        except BaseException:
            eng.set_feed_events([], [], 0)                     # a forward that never reached the library must not leave its feed events armed for the next one
            raise
        # the targets are only needed behind the forward: reduced / copied now that everything else is enqueued, behind the features
        with torch.cuda.stream(self._copy_stream):
            tgt, keep, n_valid = self._targets_to_device([b.target for b in batch], dev)
            ready = torch.cuda.Event()
            ready.record(self._copy_stream)
        for t in tgt:
            t.record_stream(cur)
        cur.wait_event(ready)
        return _Enqueued(probs, args, tgt, rgb, flow, n_valid, keep + events)      # the hipEvent_t objects stay alive until the stream has used them

    def _flush(self, model, batch, device, resident=False):
        """enqueue one batch (H2D + forward + argmax ids D2H): nothing here waits for the GPU.  Returns the record _collect finishes.
        resident: the batch comes from the feature cache (device tensors, targets in their device form)."""
        if not batch:
            return None
        # Pinned host features + a model that can be fed while it runs: ONE link-fed forward (_enqueue_link_fed).  Otherwise the batch is
        # copied and then forwarded (_enqueue), a large one in two parts (split_by_length).  Results return to the loader's order below.
        on_gpu = torch.device(device).type == "cuda"
        link_fed = on_gpu and bool(getattr(model, "link_fed_eval", False)) and bool(self.cfg.get("eval_link_fed", True)) and len(batch) >= 2 and \
            all(b.features.device.type == "cpu" and b.features.is_pinned() and
                (b.flow is None or (b.flow.device.type == "cpu" and b.flow.is_pinned())) for b in batch)
        enqueue = self._enqueue_resident if resident else self._enqueue_link_fed if link_fed else self._enqueue
        if on_gpu and not resident and not link_fed and self.cfg.get("eval_split_by_length", True):
            parts = split_by_length([int(b.features.shape[0]) for b in batch], batch[0].features.element_size(), self.cfg.get("eval_split_fraction"))
        else:
            parts = [list(range(len(batch)))]
        rec = _Launched([None] * len(batch), link_fed, keep=list(batch))
        fed = [None] * len(batch)            # (rgb, flow or None) as the forward read them on the device: what the cache keeps
        for part in parts:
            r = enqueue(model, [batch[i] for i in part], device)
            for k, i in enumerate(part):
                rec.videos[i] = (batch[i].name, r.probs[k], r.argmax[k], r.targets[k])
                fed[i] = (r.rgb[k], None if r.flow is None else r.flow[k])
            rec.keep += r.keep
            rec.n_valid = None if (rec.n_valid is None or r.n_valid is None) else rec.n_valid + r.n_valid
        if self.cfg["eval"] is not None:
            self._enqueue_ids(rec)
        if self._cache is not None and self._cache.filling:
            # behind everything this batch's ids wait for: the features (fp32 ones of a 16-bit engine converted by prego_cast_features, on
            # this stream, behind the forward that read them) and the device targets stay; an fp32 source lives until _collect drops it
            self._cache.retain(batch, [rgb for rgb, _fl in fed], [fl for _rgb, fl in fed], [t for _vid, _p, _a, t in rec.videos], torch.device(device))
            rec.fed = fed
        batch.clear()
        return rec

    def _enqueue_ids(self, rec):
        """enqueue the batch's ids to the host.  np.argmax of the one-hot targets (eval.py:55) on the device, where they are anyway for the
        AP kernel (on the host it reads frames x classes floats through one core: 25 ms for the bench set); ONE device -> host copy of the
        whole batch's pred and gt ids is ENQUEUED here (into pinned memory, behind the forward) and waited for in _collect - one batch
        later, so that the next batch's copies and forward are already running while the host waits for these ids and formats their text"""
        pred_ids = torch.cat([a for _vid, _p, a, _t in rec.videos])
        gt_ids = torch.cat([t if t.dim() == 1 else torch.argmax(t, dim=1) for _vid, _p, _a, t in rec.videos]).to(pred_ids.dtype)
        ids_dev = torch.stack([pred_ids, gt_ids])
        if not ids_dev.is_cuda:                    # a stand-in model on a CPU box (the gloo tests of the sharding logic)
            rec.ids = ids_dev
            return
        rec.ids = torch.empty(ids_dev.shape, dtype=ids_dev.dtype, pin_memory=True)
        rec.ids.copy_(ids_dev, non_blocking=True)
        rec.keep.append(ids_dev)
        if ids_dev.dtype == torch.int32 and len(self.all_class_names) <= 1000:
            # the JSON text of the ids as well (prego_format_ids: four bytes "%3d," per id), so that behind the last frame
            # the host only cuts it per video: formatting 2 x 2.3 M numbers through a numpy table took 10-15 ms there
            text_dev = torch.empty(ids_dev.shape, dtype=torch.int32, device=ids_dev.device)
            bad_dev = torch.zeros(1, dtype=torch.int32, device=ids_dev.device)
            with torch.cuda.device(ids_dev.device):
                check(_lib.load().prego_format_ids(C.c_void_p(ids_dev.data_ptr()), ids_dev.numel(), C.c_void_p(text_dev.data_ptr()),
                                                   C.c_void_p(bad_dev.data_ptr()),
                                                   C.c_void_p(torch.cuda.current_stream(ids_dev.device).cuda_stream)))
            rec.text = torch.empty(ids_dev.shape, dtype=torch.int32, pin_memory=True)
            rec.text_bad = torch.empty(1, dtype=torch.int32, pin_memory=True)
            rec.text.copy_(text_dev, non_blocking=True)
            rec.text_bad.copy_(bad_dev, non_blocking=True)
            rec.keep += [text_dev, bad_dev]
        rec.ids_ready = torch.cuda.Event()
        rec.ids_ready.record()

    def _collect(self, rec, output, json_parts):
        """the host half of a batch, one batch behind its launch: wait for its ids, cut them per video, format the videos' JSON text"""
        if rec is None:
            return
        ids = None
        if rec.ids is not None:
            if rec.ids_ready is not None:
                rec.ids_ready.synchronize()
            ids = rec.ids.numpy()
        elif rec.link_fed:
            self._copy_stream.synchronize()      # the copies read the loader's pinned tensors: keep them alive until then
        text = None
        if ids is not None and rec.text is not None and int(rec.text_bad[0]) == 0:
            text = rec.text.numpy().view(np.uint8).reshape(2, -1, 4)      # [pred | gt][frame] = b"%3d," (prego_format_ids)
        o = 0
        for vid, _p, a, _t in rec.videos:
            if ids is not None:
                n = int(a.shape[0])
                output[vid] = {"pred": ids[0, o:o + n], "gt": ids[1, o:o + n]}      # int arrays; text below
                if json_parts is not None:
                    if json_parts:
                        json_parts.append(b", ")
                    if text is not None and n > 0:
                        # the video's slice of the device-made text, in place: every list's last comma becomes its bracket
                        tp, tg = text[0, o:o + n], text[1, o:o + n]
                        tp[-1, 3] = tg[-1, 3] = 0x5D
                        json_parts += [json.dumps(str(vid)).encode() + b': {"pred": [', tp, b', "gt": [', tg, b"}"]
                    else:
                        json_parts += self._json_int_lists({vid: output[vid]}, as_parts=True)
                if self._cache is not None and self._cache.filling:
                    self._cache.gt_ids[vid] = output[vid]["gt"].copy()
                o += n
                self.last_device_argmax[vid] = a          # int32 on the device: input of aggregate_device (utils/aggregate.py)
        rec.fed = []                         # a filling call's device features: what the cache does not keep (fp32 sources of its 16-bit copies) goes now

    def _cat_targets(self, gt_targets, matrix=False):
        """the eval set's ground truth: one class-id vector [frames] when every video came as class ids (and the caller takes them), else
        the [frames, C] matrix"""
        if not matrix and all(t.dim() == 1 for t in gt_targets):
            return torch.cat(gt_targets, 0)
        return torch.cat([self._gt_matrix(t) for t in gt_targets], 0)

    def _postprocessed(self, pred, gt, n_valid):
        """the eval set's device scores and targets as the metrics see them: unchanged, or - cfg['eval_thumos_postprocessing'] -
        post-processed ONCE on the device (prego_thumos_postprocess, enqueued on the current stream) for the per-frame and the per-stage
        metric; the third value compares the device's row count with the host's when the metric is collected (None: nothing to
        compare).  The output file, the logged frame count and the FPS keep every frame: the reference post-processes inside the metric."""
        if self.data_processing is None:
            return pred, gt, None
        res = thumos_postprocessing_device(pred, gt, self.data_processing, n_valid)
        return res[1], res[0], (res.check if n_valid is not None else None)

    def _enqueue_segmental(self, argmax_ids, gt_targets, dev):
        """cfg['eval_segmental']: prego_segmental_scores twice on the current stream - over the per-video device argmax and the device
        class ids as they are, and over the cfg['eval_segmental_window']-frame vote of every video (prego_window_vote) expanded back to
        frames and cut to the video's length.  Returns the function that collects {"frames": report, "vote": report}; a vote marker of
        -1 (a window with an id outside the classes) raises there, as in aggregate_device.  cfg['eval_thumos_postprocessing'] does not
        feed this metric: it works on the argmax of the raw scores, every frame kept."""
        lib, w, ncls = _lib.load(), self.segmental_window, len(self.all_class_names)
        if w < 1 or ncls > 128:
            raise PregoError(f"cfg['eval_segmental']: eval_segmental_window {w} (>= 1), {ncls} classes (prego_window_vote takes up to 128)")
        lens = [int(a.shape[0]) for a in argmax_ids]
        offsets = torch.tensor(np.concatenate(([0], np.cumsum(lens, dtype=np.int64))), dtype=torch.int32).to(dev)
        pred = torch.cat([a.to(device=dev, dtype=torch.int32) for a in argmax_ids]).contiguous()
        gt = torch.cat([t.to(device=dev, dtype=torch.int32) for t in gt_targets]).contiguous()
        votes = torch.empty(sum((n + w - 1) // w for n in lens), dtype=torch.int32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        voted, o, f = [], 0, 0
        with torch.cuda.device(dev):
            for n in lens:
                k = (n + w - 1) // w
                if n > 0:
                    check(lib.prego_window_vote(C.c_void_p(pred[f:f + n].data_ptr()), n, w, ncls, C.c_void_p(votes[o:o + k].data_ptr()), stream))
                    voted.append(torch.repeat_interleave(votes[o:o + k], w)[:n])
                o, f = o + k, f + n
        pred_vote = torch.cat(voted).contiguous() if voted else pred
        fn_frames = segmental_scores_device(pred, gt, offsets, defer=True)
        fn_vote = segmental_scores_device(pred_vote, gt, offsets, defer=True)

        def finish():
            if bool((votes.cpu() < 0).any()):
                raise PregoError(f"cfg['eval_segmental']: a vote window holds a class id outside [0, {ncls}) (np.bincount of "
                                 "utils/aggregate.py:60 would raise / count a class the model does not have)")
            return {"frames": fn_frames(), "vote": fn_vote()}
        return finish

    def _enqueue_decode(self, ps, dev):
        """cfg['eval_decode']: prego_viterbi_decode over the pass's concatenated scores and the per-video offsets, then
        prego_segmental_scores over the decoded ids, both on the current stream.  Returns the function that collects
        {"labels": {video: int32 tensor}, "records": int64 tensor [videos, 2] (total cost | end state), "segmental": report}.
        The RAW scores are decoded: cfg['eval_thumos_postprocessing'] does not feed this."""
        ncls = len(self.all_class_names)
        lens = [int(p.shape[0]) for p in ps.pred_scores]
        offsets = torch.tensor(np.concatenate(([0], np.cumsum(lens, dtype=np.int64))), dtype=torch.int32).to(dev)
        # the concatenation the AP kernels read is the same matrix unless the THUMOS post-processing has changed it
        scores = self._metric_inputs(ps, dev)[0] if self.data_processing is None else torch.cat(ps.pred_scores, 0).to(dev)
        if scores.dim() != 2 or int(scores.shape[1]) != ncls:
            raise PregoError(f"cfg['eval_decode']: the pass's scores have shape {tuple(scores.shape)}, the data set has {ncls} classes")
        # fp32 contiguous scores (what the engines' eval forward returns) pass through; anything else is copied once, at full size
        scores = scores.to(dtype=torch.float32).contiguous()
        gt = torch.cat([t.to(device=dev, dtype=torch.int32) for t in ps.gt_targets]).contiguous()
        if self.decode_transitions is not None:
            trans, init = self.decode_transitions
        else:
            trans, init = uniform_transitions(ncls, self.decode_switch_cost, self.decode_stay_cost), None
        labels, records = viterbi_decode_device(scores, offsets, trans, init)
        fn_seg = segmental_scores_device(labels, gt, offsets, defer=True)
        names = list(ps.video_ids)

        def finish():
            lab = labels.cpu()
            cuts = np.concatenate(([0], np.cumsum(lens, dtype=np.int64))).tolist()
            return {"labels": {vid: lab[cuts[i]:cuts[i + 1]] for i, vid in enumerate(names)}, "records": records.cpu(), "segmental": fn_seg()}
        return finish

    def _loader_videos(self, model, dataloader, world, rank, skip_flow):
        """this rank's videos (EvalVideo) as the loop below batches them, one list per loader item"""
        pos = 0
        for item, (rgb_input, flow_input, target, vid, start, end) in enumerate(dataloader):
            group = []
            # loader items carry a leading batch dim of test_batch_size == 1 (dataset_builder.py:19)
            for b in range(rgb_input.shape[0]):
                mine = (pos % world) == rank
                pos += 1
                if not mine:
                    continue
                name = vid[b] if isinstance(vid, (list, tuple)) else vid
                fl = None if (skip_flow or self._flow_zero(model, flow_input[b])) else self._features(model, flow_input[b])
                group.append(EvalVideo(self._features(model, rgb_input[b]), fl, target[b], name, pos - 1, item))
            yield group

    def eval(self, model, dataloader, logger, device):
        """One pass over the eval set.  With cfg['eval_cache_device'] (off by default; eval_cache.py) the first call on a loader also
        leaves its features in device memory - at most cfg['eval_cache_max_bytes'], by default half of what is free at the first batch;
        a set that does not fit is not cached, which is no error - and later calls on the same dataset object, feature signature and
        (world, rank) take them from there: the loader is not iterated, the results are bit for bit the first call's for the same
        weights.  Features changed IN PLACE inside the same dataset object are not detected: call drop_cache().  `last_source` says
        where a call's features came from ("loader" | "cache"), `cache_info()` what is held."""
        model.eval()
        # data-parallel eval: videos are independent, so under torch.distributed rank r takes every world-th video of
        # the loader's order (no data-path collective); rank 0 gathers the per-video results once at the end
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        rank = dist.get_rank() if world > 1 else 0
        if self.perstage and world > 1:
            raise PregoError("cfg['eval_perstage']: per-stage AP depends on the order of the frames (action instances are runs over the "
                             f"concatenated videos) and is computed by a single process only; this eval runs on {world} ranks")
        if self.data_processing is not None and world > 1:
            raise PregoError("cfg['eval_thumos_postprocessing']: the temporal smoothing runs over the concatenated frames of the whole eval "
                             f"set, across the boundaries of the ranks' frame ranges, and is computed by a single process only; this eval "
                             f"runs on {world} ranks")
        if self.segmental and world > 1:
            raise PregoError("cfg['eval_segmental']: the segmental metrics are computed by a single process only (the per-video records "
                             f"of the ranks are not gathered); this eval runs on {world} ranks")
        if self.segmental and torch.device(device).type != "cuda":
            raise PregoError("cfg['eval_segmental']: the segmental metrics of an eval pass run on the device (prego_segmental_scores); host "
                             "arrays: prego_amd.segmental.segmental_scores")
        if self.decode:
            if world > 1:
                raise PregoError("cfg['eval_decode']: the decode of an eval pass is computed by a single process only (the ranks' score "
                                 f"matrices are not gathered); this eval runs on {world} ranks")
            if torch.device(device).type != "cuda":
                raise PregoError("cfg['eval_decode']: the decode of an eval pass runs on the device (prego_viterbi_decode); host arrays: "
                                 "prego_amd.decode.viterbi_decode")
            if self.cfg.get("model") == "Transformer":
                raise PregoError("cfg['eval_decode']: model 'Transformer' returns raw logits from its eval forward (ViT.py:140-143), not "
                                 "probabilities; the decoder's emission cost is defined on probabilities")
            if len(self.all_class_names) > DECODE_MAX_CLASSES:
                raise PregoError(f"cfg['eval_decode']: {len(self.all_class_names)} classes (prego_viterbi_decode takes up to {DECODE_MAX_CLASSES})")
        if self.perstage and torch.device(device).type != "cuda":
            raise PregoError("cfg['eval_perstage']: the per-stage AP of an eval pass runs on the device (prego_perstage_ap_labels); host "
                             "arrays: prego_amd.metrics.perstage_average_precision")
        skip_flow = self._zero_flow(model, dataloader)
        cache = self._cache
        self.last_source = "loader"
        if cache is None:
            return self._eval_pass(model, self._loader_videos(model, dataloader, world, rank, skip_flow), logger, device, world, rank)
        op16 = {"fp16": torch.float16, "bf16": torch.bfloat16}.get(getattr(model, "compute_dtype", None)) if hasattr(model, "engine") else None
        keep = op16 or torch.float32         # a 16-bit engine reads 16-bit operands; every other model what _features ships
        sig = (getattr(model, "d_rgb", None), getattr(model, "d_flow", None), keep, skip_flow, world, rank, str(torch.device(device)))
        if cache.begin(getattr(dataloader, "dataset", dataloader), sig, torch.device(device), keep, logger):
            self.last_source = "cache"
            videos = cache.videos()
        else:
            videos = self._loader_videos(model, dataloader, world, rank, skip_flow)
        try:
            result = self._eval_pass(model, videos, logger, device, world, rank)
        except BaseException:
            cache.abort()
            raise
        cache.commit()
        return result

    def drop_cache(self):
        """release the cached eval set (cfg['eval_cache_device']); the next call iterates the loader and fills the cache again"""
        if self._cache is not None:
            self._cache.drop()

    def cache_info(self) -> dict:
        """enabled, state ("empty" | "filled" | "disabled"), reason (why disabled), videos, frames, bytes (device memory), dtype"""
        if self._cache is None:
            return dict(enabled=False, state="disabled", reason="cfg['eval_cache_device'] is off", videos=0, frames=0, bytes=0, dtype=None)
        return self._cache.info()

    def _eval_pass(self, model, videos, logger, device, world, rank):
        """`videos`: _loader_videos, or the feature cache's record of them (device tensors: every batch is one resident forward)"""
        self.last_device_argmax = {}
        max_clips = model.max_clips          # MROAD: the engine's clip capacity; ViTEnc (`model: 'Transformer'`): its own bound
        resident = self.last_source == "cache"
        t0_ = time.perf_counter()
        self.phase_log = []                  # (phase, host seconds since the start of this eval): where an end-to-end eval spends its time
        # the THUMOS post-processing's row count: summed over the batches' host targets; a cached set's targets are on the device, so
        # its count is read back from there (8 bytes, behind the last forward)
        ps = _Pass(mark=lambda name: self.phase_log.append((name, time.perf_counter() - t0_)), t_begin=time.time(),
                   json_parts=[] if (self.cfg["eval"] is not None and world == 1) else None,
                   n_valid=0 if (self.data_processing is not None and not resident) else None)
        with torch.no_grad():
            batch, frames = [], 0
            for group in videos:
                for v in group:
                    batch.append(v)
                    ps.per_video.append((v.pos, int(v.features.shape[0])))
                    frames += int(v.features.shape[0])
                if len(batch) >= max_clips or frames >= self.max_frames_per_batch:
                    self._step(ps, model, batch, device, resident)
                    frames = 0
            self._step(ps, model, batch, device, resident, behind=lambda: self._enqueue_metrics(ps, device, world))
            self._collect(ps.pending, ps.output, ps.json_parts)
            ps.mark("collect_last")
            model.check()
            ps.mark("check")
            if world > 1:
                return self._end_multi_rank(ps, logger, device, world, rank)
            return self._end_single_process(ps, logger, device)

    def _step(self, ps, model, batch, device, resident, behind=None):
        """one step of the pass loop, in the loop and behind it: batch k is enqueued, then the host finishes batch k - 1.
        behind: enqueues what follows the last forward (the metrics), before the host waits for anything"""
        ps.mark("loader")
        rec = self._flush(model, batch, device, resident)       # batch k: enqueued ...
        if rec is not None:
            for _vid, p, a, t in rec.videos:
                ps.video_ids.append(_vid)
                ps.pred_scores.append(p)
                ps.gt_targets.append(t)
                ps.argmax_ids.append(a)
            if ps.n_valid is not None:       # one batch whose rows were not counted: no hint for the pass
                ps.n_valid = None if rec.n_valid is None else ps.n_valid + rec.n_valid
        if behind is not None:
            behind()
        ps.mark("launch")
        self._collect(ps.pending, ps.output, ps.json_parts)      # ... while the host finishes batch k - 1
        ps.mark("collect")
        ps.pending = rec

    def _on_metric_stream(self, dev, enqueue):
        """The metric queue: `enqueue()` runs on a stream of its own behind an event on the forward's stream, so that model.check() (which
        drains the forward's stream to read its timeout word) does not wait for the metric as well.  enqueue returns the function that
        collects the metric; what is returned here calls it under the same stream: the result's device -> host copy follows the kernels
        on THEIR stream."""
        if self._ap_stream is None:
            self._ap_stream = torch.cuda.Stream(dev)
        fwd_done = torch.cuda.Event()
        fwd_done.record(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self._ap_stream):
            self._ap_stream.wait_event(fwd_done)
            fn = enqueue()

        def finish(_s=self._ap_stream):
            with torch.cuda.stream(_s):
                return fn()
        return finish

    def _metric_inputs(self, ps, dev):
        """(pred, gt, check) of _postprocessed for the pass's concatenated scores and targets, made once (on the current stream)"""
        if ps.metric_inputs is None:
            pred_all = torch.cat(ps.pred_scores, 0)
            gt_all = self._cat_targets(ps.gt_targets).to(pred_all.device)
            ps.metric_inputs = self._postprocessed(pred_all.to(dev), gt_all.to(dev), ps.n_valid)
        return ps.metric_inputs

    def _need_class_ids(self, key, gt_targets):
        if not all(t.dim() == 1 for t in gt_targets):
            raise PregoError(f"cfg['{key}'] needs targets that are one class id per frame (one-hot rows, cfg['eval_label_targets'] on); this "
                             "eval set has rows that are not (dense multi-label targets: no runs of one action, no transcript)")

    def _enqueue_metrics(self, ps, device, world):
        """behind the last forward: per-frame AP, per-stage AP, the segmental metrics and the decode, each enqueued on the metric stream in
        this order"""
        dev = torch.device(device)
        self.last_perstage = self.last_segmental = self.last_decode = None
        if not ps.pred_scores:
            return
        if world == 1 and dev.type == "cuda":
            # the metric in libprego_amd.so (prego_perframe_ap, or prego_perframe_cap for metric 'cAP'), ENQUEUED here behind the last
            # forward and collected behind the output file: the GPU ranks the positives while the host waits for the ids and writes the JSON
            def enqueue_ap():
                pred, gt, post_check = self._metric_inputs(ps, dev)
                ap_fn = perframe_average_precision_device(pred, gt, self.all_class_names, None, self.metric, defer=True)
                return ap_fn if post_check is None else lambda: (ap_fn(), post_check())[0]      # the report, behind it the row count's check
            ps.finish_ap = self._on_metric_stream(dev, enqueue_ap)
        if self.perstage:
            # the per-stage report on the same device-resident scores and class ids, enqueued behind the per-frame metric and
            # collected behind everything eval writes and logs today
            self._need_class_ids("eval_perstage", ps.gt_targets)
            ps.finish_ps = self._on_metric_stream(dev, lambda: perstage_average_precision_device(
                *self._metric_inputs(ps, dev)[:2], self.all_class_names, defer=True, metrics=self.perstage_metric))
        if self.segmental:
            # the segmental records of the same device-resident ids, enqueued behind the other metrics on their stream
            self._need_class_ids("eval_segmental", ps.gt_targets)
            ps.finish_seg = self._on_metric_stream(dev, lambda: self._enqueue_segmental(ps.argmax_ids, ps.gt_targets, dev))
        if self.decode:
            # the decode of the same device-resident scores and the segmental records of its ids, behind everything above on that stream
            self._need_class_ids("eval_decode", ps.gt_targets)
            ps.finish_decode = self._on_metric_stream(dev, lambda: self._enqueue_decode(ps, dev))

    def _write_output(self, chunks):
        os.makedirs(self.output_dir, exist_ok=True)
        with open(os.path.join(self.output_dir, "output_miniROAD.json"), "wb") as file:
            file.writelines(chunks)

    def _end_multi_rank(self, ps, logger, device, world, rank):
        """the ending of a pass on several ranks: gather, class-sharded AP, rank 0 writes the file, FPS"""
        # the small things go to rank 0 as objects: per-video frame counts and the pred / gt id arrays of the output file
        # (8 bytes per frame).  The [frames x classes] score and target matrices do NOT travel whole (round 3 pickled 0.8 GB of
        # them through gather_object): the metric is computed class-sharded, see _sharded_ap
        output = ps.output
        gathered = [None] * world if rank == 0 else None
        dist.gather_object((ps.per_video, output), gathered, dst=0)
        if rank == 0:                       # back into the loader's order (a rank's dict is in the order of its per_video list)
            entries = []
            for pv, out in gathered:
                entries += [(p_idx, vid, ent) for (p_idx, _n), (vid, ent) in zip(pv, out.items())]
            output = {vid: ent for _p, vid, ent in sorted(entries, key=lambda e: e[0])}
        pred_local = torch.cat(ps.pred_scores, 0) if ps.pred_scores else torch.zeros((0, len(self.all_class_names)), device=device)
        gt_local = self._cat_targets(ps.gt_targets).to(pred_local.device) if ps.gt_targets else torch.zeros_like(pred_local)
        result = self._sharded_ap(pred_local, gt_local, world, rank)
        if rank == 0 and self.cfg["eval"] is not None:
            self._write_output([self._json_int_lists(output)])
        t_end = time.time()
        nf = torch.tensor([int(pred_local.shape[0])], dtype=torch.int64, device=pred_local.device)
        dist.all_reduce(nf)
        num_frames = int(nf.item())
        self.last_fps = num_frames / max(t_end - ps.t_begin, 1e-9)
        if rank == 0:
            logger.info(f"Processed {num_frames} frames in {t_end - ps.t_begin:.1f} seconds ({self.last_fps:.1f} FPS)")
        return result["mean_AP"]

    def _end_single_process(self, ps, logger, device):
        """the ending of a single-process pass: write the file, collect the metrics behind it, log"""
        finish_ap = ps.finish_ap
        if finish_ap is None:
            pred_all = torch.cat(ps.pred_scores, 0) if ps.pred_scores else torch.zeros((0, len(self.all_class_names)))
            gt_all = self._cat_targets(ps.gt_targets, matrix=True).to(pred_all.device) if ps.gt_targets else torch.zeros_like(pred_all)
            if torch.device(device).type == "cuda":        # an empty eval set: the empty report
                finish_ap = perframe_average_precision_device(pred_all.to(device), gt_all.to(device), self.all_class_names,
                                                              self.data_processing, self.metric, defer=True)
        num_frames = sum(n for _pos, n in ps.per_video)
        if self.cfg["eval"] is not None:      # per-video pieces (bytes and slices of the device-made text), ", " between videos
            self._write_output([self._json_int_lists(ps.output)] if ps.json_parts is None else [b"{", *ps.json_parts, b"}"])
        ps.mark("json_written")
        self.last_metric_path = "device" if finish_ap is not None else "host"
        if finish_ap is not None:
            result = finish_ap()
            ps.mark("ap_done")
        else:       # a stand-in model on a CPU box (the gloo tests of the sharding logic)
            result = perframe_average_precision(pred_all.cpu().numpy(), gt_all.cpu().numpy(), self.all_class_names, self.data_processing, self.metric)
        t_end = time.time()
        time_taken = max(t_end - ps.t_begin, 1e-9)
        self.last_fps = num_frames / time_taken
        logger.info(f"Processed {num_frames} frames in {time_taken:.1f} seconds ({self.last_fps:.1f} FPS)")
        if self.perstage:
            self.last_perstage = ps.finish_ps() if ps.finish_ps is not None else \
                perstage_report(np.zeros((N_STAGES, len(self.all_class_names))), self.all_class_names)
            ps.mark("perstage_done")
            for stage, rep_ in self.last_perstage.items():
                logger.info(f"per-stage mAP {stage}: {rep_['mean_AP'] * 100:.2f}")
        if ps.finish_seg is not None:
            self.last_segmental = ps.finish_seg()
            ps.mark("segmental_done")
            for key in [k for k in self.last_segmental["frames"] if k not in ("videos", "per_video")]:      # MoF, Edit, three F1
                logger.info(f"segmental {key}: frames {self.last_segmental['frames'][key]:.2f}, "
                            f"vote({self.segmental_window}) {self.last_segmental['vote'][key]:.2f}")
        if ps.finish_decode is not None:
            self.last_decode = ps.finish_decode()
            ps.mark("decode_done")
            how = "given transitions" if self.decode_transitions is not None else f"switch {self.decode_switch_cost}, stay {self.decode_stay_cost}"
            for key in [k for k in self.last_decode["segmental"] if k not in ("videos", "per_video")]:      # MoF, Edit, three F1
                logger.info(f"decoded ({how}) {key}: {self.last_decode['segmental'][key]:.2f}")
        return result["mean_AP"]

    def _sharded_ap(self, pred, gt, world, rank):
        """per-frame AP over the frames of ALL ranks without gathering the [frames x classes] matrices anywhere: rank q owns the classes
        [C q / world, C (q + 1) / world) of every frame - one all_to_all_single per matrix brings it those columns from every rank
        (each rank sends (world - 1) / world of its matrix once, RCCL over xGMI on a GPU node) -, runs the AP kernel on them, and only
        the three per-class vectors (AP, positives, score mass) are all-gathered: 24 bytes per class.  AP per class does not depend
        on the order of the frames (exact integer ranks, ties share a threshold), so the result equals the single-process one."""
        C_ = len(self.all_class_names)
        cb = [C_ * q // world for q in range(world + 1)]
        n_local = torch.tensor([int(pred.shape[0])], dtype=torch.int64, device=pred.device)
        ns = [torch.zeros_like(n_local) for _ in range(world)]
        dist.all_gather(ns, n_local)
        ns = [int(x.item()) for x in ns]
        mine = cb[rank + 1] - cb[rank]

        def exchange(m):
            m = m.to(torch.float32)
            send = torch.cat([m[:, cb[q]:cb[q + 1]].contiguous().reshape(-1) for q in range(world)]) if m.numel() else m.reshape(-1)
            recv = torch.empty(sum(ns) * mine, dtype=torch.float32, device=m.device)
            dist.all_to_all_single(recv, send, output_split_sizes=[n * mine for n in ns],
                                   input_split_sizes=[int(m.shape[0]) * (cb[q + 1] - cb[q]) for q in range(world)])
            return recv.reshape(sum(ns), mine) if mine else recv.reshape(sum(ns), 0)
        p_cols = exchange(pred)
        by_id = torch.tensor([int(gt.dim() == 1)], dtype=torch.int64, device=pred.device)
        dist.all_reduce(by_id, op=dist.ReduceOp.MIN)                 # class ids only if EVERY rank holds ids (a rank without videos: a matrix of no rows)
        if int(by_id.item()):
            # one-hot ground truth held as one class id per frame (_targets_to_device): every rank gets every frame's id (4 bytes per
            # frame, padded to the longest rank) instead of its columns of the target matrix; an id outside my columns = no positive there
            width_n = max(ns) if ns else 0
            buf = torch.full((max(width_n, 1),), -1, dtype=torch.int32, device=pred.device)
            buf[:gt.shape[0]] = gt.to(torch.int32)
            bufs = [torch.empty_like(buf) for _ in range(world)]
            dist.all_gather(bufs, buf)
            ids = torch.cat([bufs[q][:ns[q]] for q in range(world)]) - cb[rank]
            g_cols = ids
            if not (p_cols.is_cuda and self.metric == "AP"):
                g_cols = torch.zeros((sum(ns), mine), dtype=torch.float32, device=pred.device)
                ok = (ids >= 0) & (ids < mine)
                g_cols[torch.arange(sum(ns), device=pred.device)[ok], ids[ok].long()] = 1
        else:
            g_cols = exchange(self._gt_matrix(gt))
        if mine == 0:
            raw = (np.zeros(0), np.zeros(0, np.int64), np.zeros(0))
        elif p_cols.is_cuda and self.metric == "AP":
            self.last_metric_path = "device"
            raw = perframe_ap_raw_device(p_cols, g_cols)
        else:                                # a CPU box, or metric 'cAP' (its class-sharded form keeps the host path)
            self.last_metric_path = "host"
            raw = perframe_ap_raw(p_cols.cpu().numpy(), g_cols.cpu().numpy(), self.metric)
        width = max(cb[q + 1] - cb[q] for q in range(world))
        pack = torch.zeros((3, width), dtype=torch.float64, device=pred.device)
        pack[0, :mine] = torch.from_numpy(np.asarray(raw[0], dtype=np.float64))
        pack[1, :mine] = torch.from_numpy(np.asarray(raw[1], dtype=np.float64))          # counts < 2^53: exact in fp64
        pack[2, :mine] = torch.from_numpy(np.asarray(raw[2], dtype=np.float64))
        parts = [torch.zeros_like(pack) for _ in range(world)]
        dist.all_gather(parts, pack)
        ap = np.concatenate([parts[q][0, :cb[q + 1] - cb[q]].cpu().numpy() for q in range(world)])
        npos = np.concatenate([parts[q][1, :cb[q + 1] - cb[q]].cpu().numpy() for q in range(world)]).astype(np.int64)
        ssum = np.concatenate([parts[q][2, :cb[q + 1] - cb[q]].cpu().numpy() for q in range(world)])
        return report_from_raw(ap, npos, ssum, self.all_class_names)

    def aggregate_last(self, output_path=None, window_size: int = 200):
        """utils/aggregate.py:46-90 on the per-frame argmax the last eval left in HBM (`last_device_argmax`), with this config's
        number of classes; ground truth from the output JSON's "gt" lists"""
        js = json.load(open(os.path.join(self.output_dir, "output_miniROAD.json")))
        return aggregate_device(self.last_device_argmax, {k: v["gt"] for k, v in js.items()}, output_path, window_size,
                                n_classes=len(self.all_class_names))

    def forward(self, model, dataloader, logger, device):
        return self.eval(model, dataloader, logger, device)


@EVAL.register("ANTICIPATION")
class AntEvaluate(nn.Module):
    """`ANT_Evaluate` (trainer/eval.py:87-161): `AntEvaluate(cfg)(model, dataloader, logger[, device])` runs the anticipation eval set
    (items (rgb, flow, target [T, C], ant_target [T, L, C]) of the *_ANTICIPATION data layers) and returns the mean over the L steps of
    the per-step mAP.  `self.result` holds what the reference's `result` holds: the OAD report (`mean_AP`, per class) and
    `anticipation_{l+1}` = the report of step l.
    A model with `forward_clips` on a GPU (MiniROADA) is fed whole videos in batches (one ragged forward per batch, anticipation head
    included); on a CUDA device metric 'AP' (`prego_perframe_ap`) and metric 'cAP' (`prego_perframe_cap`) are computed there, for the
    OAD scores and every anticipation step.  A stand-in model on the CPU (called per loader batch, as the reference does) uses the
    host path.  `last_metric_path` ('device' or 'host') says what ran.
    A THUMOS data set (the name in front of the first '_') is refused unless cfg['eval_thumos_postprocessing'] is set; with it every
    report is computed on post-processed arrays (`ThumosPostprocessing`; on the device `prego_thumos_postprocess`, step l read in
    place through its row stride)."""

    def __init__(self, cfg):
        super().__init__()
        data_name =cfg["data_name"].split("_")[0]
        # eval.py:92-93: the OAD report is post-processed with target[:, 21], step l with ant_target[:, l, 21]
        self.data_processing = _thumos_postprocessing(cfg, data_name == "THUMOS")
        self.metric = cfg["metric"]
        if self.metric not in ("AP", "cAP"):
            raise RuntimeError(f"Unknown metrics: {self.metric}")
        self.all_class_names = json.load(open(cfg["video_list_path"]))[data_name]["class_index"]
        self.max_frames_per_batch = int(cfg.get("eval_frames_per_batch", 4_000_000))
        self.result = None
        self.last_fps = None
        self.last_metric_path = None

    def _metric(self, pred, gt, n_valid=None):
        """pred / gt [frames, C], possibly [:, l, :] views of the [frames, L, C] tensors: with the THUMOS post-processing they go to the C
        entry as they are (ld_scores / ld_target), n_valid = the rows it keeps when they were counted on the host"""
        post = self.data_processing
        if pred.is_cuda:
            self.last_metric_path = "device"
            if post is None:
                pred, gt = pred.contiguous(), gt.contiguous()
                return perframe_average_precision_device(pred, gt.to(pred.device, torch.float32), self.all_class_names, None, self.metric)
            return perframe_average_precision_device(pred, gt.to(pred.device, torch.float32), self.all_class_names, post, self.metric,
                                                     n_valid=n_valid)
        self.last_metric_path = "host"
        return perframe_average_precision(pred.contiguous().cpu().numpy(), gt.contiguous().cpu().numpy(), self.all_class_names, post, self.metric)

    def eval(self, model, dataloader, logger, device=None):
        dev = torch.device(device) if device is not None else (torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu"))
        model.eval()
        batched = hasattr(model, "forward_clips") and dev.type == "cuda"
        preds, gts, apreds, agts = [], [], [], []
        pend, pend_frames = [], 0

        def flush():
            nonlocal pend, pend_frames
            if not pend:
                return
            rgb = [p[0] for p in pend] if model.use_rgb else None
            flow = [p[1] for p in pend] if model.use_flow else None
            outs, _, _, ants, _ = model.forward_clips(rgb, flow, want_argmax=False, want_ant=True)
            for (_, _, t, a), o, x in zip(pend, outs, ants):
                preds.append(o); gts.append(t); apreds.append(x); agts.append(a)
            pend, pend_frames = [], 0

        post = self.data_processing
        counts = {0: 0} if (post is not None and batched) else None      # [0]: the OAD targets, [l + 1]: step l
        t0 = time.perf_counter()
        with torch.no_grad():
            for rgb_input, flow_input, target, ant_target in dataloader:
                C = target.shape[-1]
                if batched:
                    for b in range(rgb_input.shape[0]):
                        T = int(target.shape[1])
                        if T == 0:
                            continue
                        if post is not None and counts is not None:      # the rows the post-processing keeps, while the targets are host rows
                            if target.device.type == "cpu" and ant_target.device.type == "cpu":
                                counts[0] += post.count_valid(target[b].numpy())
                                for l in range(ant_target.shape[2]):
                                    counts[l + 1] = counts.get(l + 1, 0) + post.count_valid(ant_target[b][:, l].numpy())
                            else:
                                counts = None
                        pend.append((rgb_input[b].to(dev, torch.float32).contiguous(), flow_input[b].to(dev, torch.float32).contiguous(),
                                     target[b].to(dev), ant_target[b].to(dev)))
                        pend_frames += T
                        if pend_frames >= self.max_frames_per_batch or len(pend) >= model.max_clips:
                            flush()
                else:
                    out = model(rgb_input.to(dev), flow_input.to(dev))
                    preds.append(out["logits"].reshape(-1, C)); gts.append(target.to(dev).reshape(-1, C))
                    L = out["anticipation_logits"].shape[-2]
                    apreds.append(out["anticipation_logits"].reshape(-1, L, C)); agts.append(ant_target.to(dev).reshape(-1, L, C))
            if batched:
                flush()
        n_frames = sum(int(p.shape[0]) for p in preds)
        pred, gt = torch.cat(preds).to(torch.float32), torch.cat(gts).to(torch.float32)
        apred, agt = torch.cat(apreds).to(torch.float32), torch.cat(agts).to(torch.float32)
        hint = (lambda k: counts.get(k)) if counts is not None else (lambda k: None)
        result = self._metric(pred, gt, hint(0))
        logger.info(f'OAD mAP: {result["mean_AP"] * 100:.2f}')
        maps = []
        for step in range(agt.shape[1]):
            result[f"anticipation_{step + 1}"] = self._metric(apred[:, step, :], agt[:, step, :], hint(step + 1))
            maps.append(result[f"anticipation_{step + 1}"]["mean_AP"])
            logger.info(f"Anticipation at step {step + 1}: {maps[-1] * 100:.2f}")
        logger.info(f"Mean Anticipation mAP: {np.mean(maps) * 100:.2f}")
        dt = time.perf_counter() - t0
        self.last_fps = n_frames / dt if dt > 0 else None
        logger.info(f"Processed {n_frames} frames in {dt:.1f} seconds ({(self.last_fps or 0):.1f} FPS)")
        self.result = result
        return np.mean(maps)

    def forward(self, model, dataloader, logger, device=None):
        return self.eval(model, dataloader, logger, device)
