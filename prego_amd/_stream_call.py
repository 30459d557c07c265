"""The steps the nine streaming entries share between their signature and their C call: MiniRoadEngine.step / step_wide / step_frames /
step_ragged, StreamPool.push / push_frames / push_ragged, TransformerStreamPool.push / push_bursts.  Each entry calls them in its own
order - the order decides which message wins when a call is wrong in two ways.  `who` is the entry's name as its messages spell it.
Nothing here loads the library.  Where the entries' policies have drifted apart a flag keeps each one's behaviour and says whose it is
(tests/golden/stream_refusals.json pins the texts)."""
from __future__ import annotations

import ctypes as C

import torch

from ._lib import PregoError

F32, I32 = torch.float32, torch.int32


def refuse_general(who: str, compute_dtype: str, hid: int, num_layers: int, advice: str):
    """the entries without a general-forward route, on an engine the streaming kernels are not built for; advice: what to do instead"""
    if compute_dtype in ("fp32", "fp16x2") or hid != 1024 or num_layers != 1:
        raise PregoError(f"{who}: the streaming kernels are built for bf16 / fp16 operands, hidden_dim 1024, one GRU layer (this engine: "
                         f"{compute_dtype}, hidden_dim {hid}, {num_layers} layers); {advice}")


def resolve_ant(who: str, want_ant, ant_len: int) -> bool:
    """want_ant None: whether the model has an anticipation head (ant_len: 0 before set_anticipation)"""
    if want_ant is None:
        want_ant = bool(ant_len)
    if want_ant and not ant_len:
        raise PregoError(f"{who}(want_ant=True) before set_anticipation")
    return want_ant


def frame_source(who: str, d_rgb: int, rgb, flow, frames: str = "frame"):
    """the tensor that tells the call's shape: rgb, or flow for a --no_rgb model.  frames: "frame" / "frames", as the entry says it"""
    src = rgb if d_rgb > 0 else flow
    if src is None:
        raise PregoError(f"{who}: a --no_rgb model needs the flow {frames}" if d_rgb == 0 else f"{who}: rgb is None")
    return src


def counts_list(who: str, counts, n=None, refuse_cuda: bool = False, one_int: bool = False) -> list:
    """a call's frame counts as ints; n: the length they must have, where the entry knows it from its slots.
    refuse_cuda: step_ragged refuses a CUDA, floating-point or non-1-d tensor; the pools' entries take whatever .tolist() gives.
    one_int: push_bursts takes one number as the count of every slot; the others let the TypeError out."""
    if isinstance(counts, torch.Tensor):
        if refuse_cuda and (counts.is_cuda or counts.is_floating_point() or counts.dim() != 1):
            raise PregoError(f"{who}: counts is a sequence of ints or a 1-d CPU int tensor, got {tuple(counts.shape)} {counts.dtype} on {counts.device}")
        counts = counts.tolist()
    try:
        counts = [int(k) for k in counts]
    except TypeError:
        if not one_int:
            raise
        counts = [int(counts)] * n
    if n is not None and len(counts) != n:
        raise PregoError(f"{who}: {n} slots, {len(counts)} counts")
    return counts


def clamp_i32(counts) -> list:
    """step_ragged saturates the counts it hands the library as int32; the pools' entries do not (ctypes wraps)"""
    return [min(max(k, -(2 ** 31)), 2 ** 31 - 1) for k in counts]


def in_specs(rows: tuple, d_rgb: int, d_flow: int, rgb, flow) -> list:
    """check() specs of the feature tensors of a call whose outputs have the leading shape `rows`; a --no_rgb model's rgb is not looked at"""
    return [(rgb if d_rgb > 0 else None, rows + (d_rgb,), F32, "rgb"), (flow, rows + (d_flow,), F32, "flow")]


def outputs(device, rows: tuple, ncls: int, ant_len: int, out, argmax, ant_out=None, ant_argmax=None):
    """(the tuple the entry returns, its check() specs): out and argmax and, with ant_len > 0, the anticipation pair, each allocated where
    the caller passed none.  rows: (n,), (n, K) or (R,)"""
    specs = [(out, rows + (ncls,), F32, "out"), (argmax, rows, I32, "argmax")]
    if ant_len:
        specs += [(ant_out, rows + (ant_len, ncls), F32, "anticipation out"), (ant_argmax, rows + (ant_len,), I32, "anticipation argmax")]
    specs = [(torch.empty(shape, dtype=dt, device=device) if t is None else t, shape, dt, what) for t, shape, dt, what in specs]
    return tuple(s[0] for s in specs), specs


def check(who: str, specs, expected: str = "{what} as contiguous {dt} cuda {shape}"):
    """every (tensor or None, shape, dtype, what) of specs: a contiguous cuda tensor of that dtype and shape.  expected: how the entry
    words what it wanted (`step` has three wordings of its own, push_bursts a note on the packed rows)"""
    for t, shape, dt, what in specs:
        if t is not None and (not t.is_cuda or t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != shape):
            raise PregoError(f"{who}: expected {expected.format(what=what, dt=dt, shape=list(shape))}, got {tuple(t.shape)} {t.dtype} on {t.device}")


class Workspace:
    """a byte tensor that grows to the largest size asked for: allocated outside the C call, by torch's allocator"""
    t = None

    def fit(self, need: int, device, none_if_zero: bool = False):
        """none_if_zero: the engine's entries pass no workspace for a size of 0 (a shape the library refuses, or step_wide up to 16
        streams); the pools' entries pass the tensor they hold.  Either way the C call is made and the refusal is the library's"""
        if none_if_zero and not need:
            return None
        if self.t is None or self.t.numel() < need:
            self.t = torch.empty(need, dtype=torch.uint8, device=device)
        return self.t


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None
