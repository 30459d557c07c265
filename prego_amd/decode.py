"""Viterbi decoding: the cheapest label sequence of a video under per-frame emission costs and a first-order transition matrix - the
smoother step-recognition results on Assembly101 are reported with (Edit / F1 of the decoded transcript instead of the per-frame
argmax).  Unlike the 200-frame block vote (`aggregate`, prego_window_vote) it reads the scores, can put a boundary anywhere, and weighs
one more switch against the evidence for it.

Definitions (include/prego_amd.h, prego_viterbi_decode, carries them word for word).  Everything is integer: costs are in 1/256 bit
(256 units = a factor 2 in probability), DECODE_CAP = 32767 is the largest cost word, DECODE_FORBIDDEN = -1 (any negative word) a
transition or a start that cannot be taken.  The emission cost of a probability is read off its fp32 WORD (`emission_costs`): CAP for a
set sign bit, a NaN or an exponent field E of 0; 0 for p >= 1; else 256 * (127 - E) - DECODE_LUT[mantissa >> 15] with
DECODE_LUT[k] = rint(256 * log2(1 + (k + 0.5) / 256)) - no logarithm is taken at run time, so host and device cannot differ.
Per video, with e_t(j) the emission cost of frame t and class j:  d_0(j) = init[j] + e_0(j);  d_t(j) = e_t(j) + min over the allowed i
with a finite d_{t-1}(i) of d_{t-1}(i) + trans[i][j], back-pointer = the LOWEST such i;  end state = the lowest j with the smallest
finite d_{T-1}(j);  labels = the back-pointer chain.  A frame at which no state is finite makes the video INFEASIBLE: labels all -1,
record (-1, -1).  An empty video has the record (0, -1).  Record = (total cost, end state), int64.

  * `DECODE_LUT`, `emission_costs`          - the quantiser in numpy, bit for bit the kernel's.
  * `viterbi_decode`                        - the host model of one video (integer numpy): the oracle of the kernel.
  * `path_cost`                             - what a given label sequence costs under the model (None: it takes a forbidden step).
  * `uniform_transitions`                   - stay_cost on the diagonal, switch_cost elsewhere.
  * `viterbi_decode_device`                 - the HIP path, `prego_viterbi_decode` / `prego_viterbi_decode_costs` (csrc/decode.hip): one
                                              launch, one workgroup per video.  No CPU fallback.
  * `emission_costs_device`                 - `prego_emission_costs`, the kernel's quantiser alone.
  * `OnlineDecoder`                         - the host model of one slot of a decode pool (online fixed-lag decoding, below): the oracle
                                              of csrc/decode_pool.hip.
  * `online_decode_device`                  - whole videos through a `stream_pool.DecodePool`: what a lag costs against the offline decode.

Online, fixed lag (include/prego_amd.h, prego_decode_pool_*, carries this word for word).  The model and the quantiser are the ones above.
  - trans[i][j] and init[j] are int32.
  - A negative word is forbidden.  A word above DECODE_CAP is read as CAP.  init None means zeros.
  - At most 128 classes.
  - Emission costs come from the fp32 word by DECODE_LUT, or from int32 cost words clamped into [0, CAP].
  - d_0, d_t and the back-pointer (lowest i on a tie) are as in viterbi_decode.
  - e_t is the lowest j with the smallest finite d_t(j).
Fixed lag L (0..256).
  - After frame t of a stream has been ingested and t >= L, frame f = t - L is committed.  label(f) is the state at frame f on the
    back-pointer chain that starts at e_t.
  - flush commits the remaining frames [max(0, T - L), T) from the chain that starts at e_{T-1}.
  - Dead streams: a frame at which no state is finite makes the stream dead.  Every label committed from then on is -1, at flush too.
    Labels already committed stay.
Equivalently, and this is the oracle identity:  label(f) = viterbi_decode(x[: min(f + L, T - 1) + 1])[0][f].
After T frames, (cost, end state) equals viterbi_decode(x[:T])'s record.  With L >= T - 1 the labels equal the offline decode.
Consecutive labels come from different chains, so the committed sequence need not be an allowed path.
The result depends on the frames only.  It does not depend on how they were cut into calls, on slot numbers, on the order of `slots`,
or on the other slots.
`ProcedureModel.transition_costs` (procedure.py) turns a corpus of correct transcripts into (trans, init)."""
from __future__ import annotations

import numpy as np

DECODE_CAP = 32767                 # PREGO_DECODE_CAP
DECODE_FORBIDDEN = -1              # PREGO_DECODE_FORBIDDEN
DECODE_MAX_CLASSES = 128           # PREGO_DECODE_MAX_CLASSES
DECODE_BLOCK = 64                  # PREGO_DECODE_BLOCK: frames per block of the kernel's backtrace
DECODE_PREFETCH = 8                # PREGO_DECODE_PREFETCH: frames ahead of the step the kernel requests its emission rows
DECODE_POOL_MAX_LAG = 256          # PREGO_DECODE_POOL_MAX_LAG
DECODE_PENDING = -2                # PREGO_DECODE_PENDING: the filler behind the labels a push or a flush committed
DECODE_POOL_BURST = 32             # frames a slot takes per push at most
STATUS_DEAD, STATUS_FLUSHED, STATUS_PUSHED_AFTER_FLUSH = 1, 2, 4      # the status word of a slot's header
_INF = 1 << 62                     # the oracle's "no path": above every finite cost (below 2^31 frames x 65534)

DECODE_LUT = np.array([
      1,   2,   4,   5,   6,   8,   9,  11,  12,  13,  15,  16,  18,  19,  20,  22,
     23,  24,  26,  27,  28,  30,  31,  32,  34,  35,  36,  38,  39,  40,  42,  43,
     44,  45,  47,  48,  49,  50,  52,  53,  54,  55,  57,  58,  59,  60,  62,  63,
     64,  65,  66,  68,  69,  70,  71,  72,  74,  75,  76,  77,  78,  80,  81,  82,
     83,  84,  85,  86,  88,  89,  90,  91,  92,  93,  94,  95,  97,  98,  99, 100,
    101, 102, 103, 104, 105, 106, 108, 109, 110, 111, 112, 113, 114, 115, 116, 117,
    118, 119, 120, 121, 122, 123, 124, 125, 126, 127, 128, 129, 131, 132, 133, 134,
    135, 136, 137, 138, 139, 140, 140, 141, 142, 143, 144, 145, 146, 147, 148, 149,
    150, 151, 152, 153, 154, 155, 156, 157, 158, 159, 160, 161, 162, 163, 163, 164,
    165, 166, 167, 168, 169, 170, 171, 172, 173, 173, 174, 175, 176, 177, 178, 179,
    180, 181, 182, 182, 183, 184, 185, 186, 187, 188, 189, 189, 190, 191, 192, 193,
    194, 195, 195, 196, 197, 198, 199, 200, 200, 201, 202, 203, 204, 205, 205, 206,
    207, 208, 209, 210, 210, 211, 212, 213, 214, 214, 215, 216, 217, 218, 218, 219,
    220, 221, 222, 222, 223, 224, 225, 226, 226, 227, 228, 229, 229, 230, 231, 232,
    233, 233, 234, 235, 236, 236, 237, 238, 239, 239, 240, 241, 242, 242, 243, 244,
    245, 245, 246, 247, 248, 248, 249, 250, 251, 251, 252, 253, 253, 254, 255, 256], dtype=np.int32)


def emission_costs(p) -> np.ndarray:
    """probabilities (any shape, read as fp32) -> int32 emission costs of the same shape, from the fp32 words alone"""
    w = np.ascontiguousarray(np.asarray(p, dtype=np.float32)).view(np.uint32)
    e = ((w >> 23) & 0xFF).astype(np.int32)
    k = ((w >> 15) & 0xFF).astype(np.intp)
    cost = 256 * (127 - e) - DECODE_LUT[k]
    cost = np.where(e >= 127, 0, cost)                                       # p >= 1.0, +inf included (NaN: below)
    bad = ((w >> 31) != 0) | (e == 0) | ((e == 255) & ((w & 0x7FFFFF) != 0))
    return np.where(bad, DECODE_CAP, cost).astype(np.int32)


def _clamp_model(trans, init, C):
    """(trans [C, C], init [C]) as int64 with -1 for forbidden words and words above CAP read as CAP"""
    tr = np.asarray(trans, dtype=np.int64)
    if tr.shape != (C, C):
        raise ValueError(f"decode: trans has shape {tr.shape}, the scores have {C} classes")
    ini = np.zeros(C, np.int64) if init is None else np.asarray(init, dtype=np.int64).reshape(-1)
    if ini.shape != (C,):
        raise ValueError(f"decode: init has {ini.size} words, the scores have {C} classes")
    clamp = lambda x: np.where(x < 0, -1, np.minimum(x, DECODE_CAP))
    return clamp(tr), clamp(ini)


def uniform_transitions(C: int, switch_cost: int, stay_cost: int = 0) -> np.ndarray:
    """int32 [C, C]: stay_cost on the diagonal, switch_cost everywhere else (either may be DECODE_FORBIDDEN)"""
    C = int(C)
    if not 1 <= C <= DECODE_MAX_CLASSES:
        raise ValueError(f"decode: {C} classes (1..{DECODE_MAX_CLASSES})")
    tr = np.full((C, C), int(switch_cost), np.int32)
    np.fill_diagonal(tr, int(stay_cost))
    return tr


def viterbi_decode(costs_or_probs, trans, init=None):
    """The host model of ONE video.  costs_or_probs [T, C]: a floating array is probabilities (quantised by `emission_costs`), an
    integer array emission costs (clamped into [0, CAP]).  trans int [C, C], init int [C] or None (zeros); negative words are
    forbidden, words above CAP are CAP.  Returns (labels int32 [T], (total cost, end state)); an infeasible video: labels all -1 and
    (-1, -1); T == 0: no labels and (0, -1)."""
    x = np.asarray(costs_or_probs)
    if x.ndim != 2:
        raise ValueError(f"decode: scores of shape {x.shape} ([frames, classes])")
    T, C = x.shape
    if not 1 <= C <= DECODE_MAX_CLASSES:
        raise ValueError(f"decode: {C} classes (1..{DECODE_MAX_CLASSES})")
    e = emission_costs(x).astype(np.int64) if x.dtype.kind == "f" else np.clip(x.astype(np.int64), 0, DECODE_CAP)
    tr, ini = _clamp_model(trans, init, C)
    if T == 0:
        return np.zeros(0, np.int32), (0, -1)
    step = np.where(tr < 0, _INF, tr)                        # [i, j]
    d = np.where(ini < 0, _INF, ini + e[0])
    back = np.zeros((T, C), np.int64)
    for t in range(1, T):
        cand = np.where((d[:, None] >= _INF) | (step >= _INF), _INF, d[:, None] + step)
        back[t] = np.argmin(cand, axis=0)                    # the first minimum: the lowest i
        best = cand[back[t], np.arange(C)]
        d = np.where(best >= _INF, _INF, best + e[t])
        if (d >= _INF).all():
            break
    if (d >= _INF).all():
        return np.full(T, -1, np.int32), (-1, -1)
    end = int(np.argmin(d))
    labels = np.empty(T, np.int32)
    s = end
    for t in range(T - 1, -1, -1):
        labels[t] = s
        s = int(back[t, s])
    return labels, (int(d[end]), end)


def path_cost(costs_or_probs, trans, init, labels):
    """what the label sequence `labels` costs under the model, or None when it takes a forbidden start or transition"""
    x = np.asarray(costs_or_probs)
    e = emission_costs(x).astype(np.int64) if x.dtype.kind == "f" else np.clip(x.astype(np.int64), 0, DECODE_CAP)
    tr, ini = _clamp_model(trans, init, x.shape[1])
    lab = np.asarray(labels, dtype=np.int64)
    if lab.size == 0:
        return 0
    steps = tr[lab[:-1], lab[1:]]
    if ini[lab[0]] < 0 or (steps < 0).any():
        return None
    return int(ini[lab[0]] + steps.sum() + e[np.arange(lab.size), lab].sum())


def _device_args(what, scores, C):
    import torch

    from ._lib import PregoError
    if not (isinstance(scores, torch.Tensor) and scores.is_cuda):
        raise PregoError(f"{what} needs CUDA tensors; there is no CPU fallback (host arrays: prego_amd.decode.viterbi_decode)")
    if scores.dim() != 2 or scores.stride(1) != 1 and scores.shape[0] > 0:
        raise PregoError(f"{what}: scores must be [frames, classes] with contiguous rows")
    if not 1 <= C <= DECODE_MAX_CLASSES:
        raise PregoError(f"{what}: {C} classes (1..{DECODE_MAX_CLASSES})")


def viterbi_decode_device(scores, offsets, trans, init=None, costs=False, defer=False):
    """Device path: scores a CUDA tensor [frames, classes] (rows contiguous, any row stride >= classes) - fp32 probabilities, or int32
    emission costs with costs=True -, the videos one after the other; offsets an int32 CUDA tensor [videos + 1]; trans [C, C] and init
    [C] (or None) integer arrays or tensors.  `prego_viterbi_decode` / `prego_viterbi_decode_costs` on the current stream.  Returns
    (labels int32 CUDA tensor [frames], records int64 CUDA tensor [videos, 2]); nothing waits.  defer=True: a function is returned that
    waits for the kernel and gives (labels, records) on the host as numpy arrays.  No CPU fallback."""
    import ctypes as C_

    import torch

    from . import _lib
    from ._lib import PregoError, check
    what = "viterbi_decode_device"
    C = int(scores.shape[1]) if hasattr(scores, "shape") and len(scores.shape) == 2 else 0
    _device_args(what, scores, C)
    if scores.dtype != (torch.int32 if costs else torch.float32):
        raise PregoError(f"{what}: scores are {scores.dtype}; costs={costs} takes {'int32' if costs else 'float32'}")
    if not (isinstance(offsets, torch.Tensor) and offsets.is_cuda) or offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 2:
        raise PregoError(f"{what}: offsets must be a one-dimensional int32 CUDA tensor of videos + 1 words (at least 2)")
    dev = scores.device
    as_dev = lambda a, n: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))).to(
        device=dev, dtype=torch.int32).reshape(n).contiguous()
    tr = as_dev(trans, C * C)
    ini = None if init is None else as_dev(init, C)
    offsets = offsets.contiguous()
    n, nv = int(scores.shape[0]), int(offsets.numel()) - 1
    ld = int(scores.stride(0)) if n > 1 else C
    lib = _lib.load()
    src = scores if n > 0 else torch.zeros((1, C), dtype=scores.dtype, device=dev)     # an empty tensor has no address
    ws = torch.empty(lib.prego_viterbi_workspace_bytes(n, nv, C), dtype=torch.uint8, device=dev)
    labels = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    records = torch.empty((nv, 2), dtype=torch.int64, device=dev)
    p = lambda t: C_.c_void_p(t.data_ptr())
    entry = lib.prego_viterbi_decode_costs if costs else lib.prego_viterbi_decode
    with torch.cuda.device(dev):
        check(entry(p(src), ld, p(offsets), nv, n, C, p(tr), p(ini) if ini is not None else None, p(labels), p(records),
                    p(ws) if n > 0 else None, ws.numel(), C_.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    labels = labels[:n]
    if not defer:                                          # the allocator hands the workspace out again only behind the kernel, on its stream
        return labels, records

    def finish(_keep=(src, offsets, tr, ini, ws)):
        return labels.cpu().numpy(), records.cpu().numpy()
    return finish


def emission_costs_device(probs):
    """fp32 CUDA tensor [frames, classes] (rows contiguous) -> int32 CUDA tensor [frames, classes]: `prego_emission_costs` on the
    current stream, the quantiser of the decode kernel alone"""
    import ctypes as C_

    import torch

    from . import _lib
    from ._lib import PregoError, check
    what = "emission_costs_device"
    if not (isinstance(probs, torch.Tensor) and probs.is_cuda) or probs.dtype != torch.float32 or probs.dim() != 2 or \
            (probs.stride(1) != 1 and probs.shape[0] > 0):
        raise PregoError(f"{what} needs an fp32 CUDA tensor [frames, classes] with contiguous rows; host arrays: emission_costs")
    n, C = int(probs.shape[0]), int(probs.shape[1])
    out = torch.empty((n, C), dtype=torch.int32, device=probs.device)
    if n == 0 or C == 0:
        return out
    with torch.cuda.device(probs.device):
        check(_lib.load().prego_emission_costs(C_.c_void_p(probs.data_ptr()), int(probs.stride(0)) if n > 1 else C, n, C,
                                               C_.c_void_p(out.data_ptr()), C_.c_void_p(torch.cuda.current_stream(probs.device).cuda_stream)))
    return out


class OnlineDecoder:
    """OnlineDecoder(trans, init=None, lag=64, n_classes=None, vote_window=1, max_events=1024): the host model of ONE slot of a decode
    pool, in integer numpy (the definitions are the module's).  `push(rows)` - rows [K, C], floating = probabilities, integer = costs -
    returns (labels, now): the labels the rows committed, in frame order, and e_t of every row (-1 once dead).  `flush()` commits the
    tail and returns its labels; afterwards a push ingests nothing and returns DECODE_PENDING fillers.  `frames`, `committed`, `dead`,
    `flushed`, `cost`, `end` are the header; `record` is the `aggregate.OnlineRecord` the committed labels went through, one by one;
    `state_words()` is the slot's header and keys as the device keeps them."""

    def __init__(self, trans, init=None, lag: int = 64, n_classes=None, vote_window: int = 1, max_events: int = 1024):
        from .aggregate import OnlineRecord
        C = int(np.asarray(trans).shape[0]) if n_classes is None else int(n_classes)
        if not 1 <= C <= DECODE_MAX_CLASSES:
            raise ValueError(f"decode: {C} classes (1..{DECODE_MAX_CLASSES})")
        if not 0 <= int(lag) <= DECODE_POOL_MAX_LAG:
            raise ValueError(f"decode: lag {lag} (0..{DECODE_POOL_MAX_LAG})")
        tr, self._ini = _clamp_model(trans, init, C)
        self._step = np.where(tr < 0, _INF, tr)
        self.n_classes, self.lag = C, int(lag)
        self.record = OnlineRecord(int(vote_window), C, int(max_events))
        self.frames, self.committed, self.dead, self.flushed, self.pushed_after_flush = 0, 0, False, False, False
        self._d, self._back = None, {}                       # the keys' costs; frame -> back-pointer row, the last `lag` frames

    def _costs(self, rows):
        x = np.asarray(rows)
        if x.ndim == 1:
            x = x[None]
        if x.ndim != 2 or x.shape[1] != self.n_classes:
            raise ValueError(f"decode: rows of shape {x.shape} ([frames, {self.n_classes}])")
        return emission_costs(x).astype(np.int64) if x.dtype.kind == "f" else np.clip(x.astype(np.int64), 0, DECODE_CAP)

    def _finite(self):
        return self._d is not None and bool((self._d < _INF).any())

    @property
    def end(self) -> int:
        """e of the last frame: -1 for a dead or an empty stream"""
        return int(np.argmin(self._d)) if self._finite() else -1

    @property
    def cost(self) -> int:
        """the total cost so far: 0 for an empty stream, -1 for a dead one"""
        return 0 if self.frames == 0 else (int(self._d.min()) if self._finite() else -1)

    def _walk(self, s: int, t: int, f: int) -> int:
        for u in range(t, f, -1):
            s = int(self._back[u][s])
        return s

    def _commit(self, label: int):
        self.record.push(label)
        self.committed += 1

    def push(self, rows):
        e = self._costs(rows)
        if self.flushed:
            self.pushed_after_flush = True
            fill = np.full(e.shape[0], DECODE_PENDING, np.int32)
            return fill, fill.copy()
        labels, now, C = [], [], self.n_classes
        for row in e:
            t = self.frames
            if t == 0:
                self._d = np.where(self._ini < 0, _INF, self._ini + row)
            else:
                cand = np.where((self._d[:, None] >= _INF) | (self._step >= _INF), _INF, self._d[:, None] + self._step)
                back = np.argmin(cand, axis=0)
                best = cand[back, np.arange(C)]
                self._back[t] = np.where(best >= _INF, 0, back)
                self._back.pop(t - self.lag - 1, None)
                self._d = np.where(best >= _INF, _INF, best + row)
            self.frames += 1
            en = self.end
            self.dead = self.dead or en < 0
            now.append(en)
            if t >= self.lag:
                labels.append(-1 if en < 0 else self._walk(en, t, t - self.lag))
                self._commit(labels[-1])
        return np.asarray(labels, np.int32), np.asarray(now, np.int32)

    def flush(self):
        """commits the frames [committed, frames) from the chain of the last frame, votes the record's unfinished window, marks the
        stream flushed; returns the labels (a second flush: none)"""
        labels = []
        if not self.flushed:
            en, T = self.end, self.frames
            labels = [-1 if en < 0 else self._walk(en, T - 1, f) for f in range(self.committed, T)]
            for lab in labels:
                self._commit(lab)
            self.flushed = True
        self.record.flush()
        return np.asarray(labels, np.int32)

    @property
    def status(self) -> int:
        return (STATUS_DEAD if self.dead else 0) | (STATUS_FLUSHED if self.flushed else 0) | (STATUS_PUSHED_AFTER_FLUSH if self.pushed_after_flush else 0)

    def keys(self) -> np.ndarray:
        """int64 [n_classes rounded up to 4]: d << 7 | state, 2^62 for "no path"; zeros while the stream is empty, and in the padding"""
        k = np.zeros((self.n_classes + 3) // 4 * 4, np.int64)
        if self.frames:
            k[:self.n_classes] = np.where(self._d >= _INF, _INF, (self._d << 7) | np.arange(self.n_classes))
        return k

    def state_words(self) -> np.ndarray:
        """the slot's header and keys as int32 words (prego_decode_pool_state): frames | committed | status | end state (0 while empty) |
        cost (int64) | 0 | 0, then the keys"""
        head = np.array([self.frames, self.committed, self.status, self.end if self.frames else 0], np.int32)
        return np.concatenate((head, np.array([self.cost], np.int64).view(np.int32), np.zeros(2, np.int32), self.keys().view(np.int32)))


def online_decode_device(scores, offsets, trans, init=None, lag: int = 64, costs: bool = False):
    """Whole videos through a `stream_pool.DecodePool`, as live streams would pass: scores a CUDA tensor [frames, classes] (fp32
    probabilities, or int32 costs with costs=True), the videos one after the other; offsets [videos + 1] (host ints or a tensor).  Up
    to 256 videos at a time, each fed 32 frames per call (at most 256 rows a call, gathered by `index_select`), then flushed.  Returns
    (labels int32 CUDA tensor [frames] - label(f) of the module's definition -, records int64 CUDA tensor [videos, 2] - total cost |
    end state as `viterbi_decode_device` gives them).  Host glue over the pool: it measures what a lag costs against the offline
    decode.  No CPU fallback."""
    import torch

    from .stream_pool import MAX_ACTIVE, DecodePool
    what = "online_decode_device"
    C = int(scores.shape[1]) if hasattr(scores, "shape") and len(scores.shape) == 2 else 0
    _device_args(what, scores, C)
    off = [int(v) for v in (offsets.cpu().tolist() if isinstance(offsets, torch.Tensor) else offsets)]
    n, nv, dev = int(scores.shape[0]), len(off) - 1, scores.device
    if nv < 1 or off[0] < 0 or off[-1] > n or any(b < a for a, b in zip(off, off[1:])):
        from ._lib import PregoError
        raise PregoError(f"{what}: offsets must ascend within [0, {n}] and name at least one video")
    lag = int(lag)
    labels = torch.full((max(n, 1),), DECODE_PENDING, dtype=torch.int32, device=dev)
    records = torch.empty((nv, 2), dtype=torch.int64, device=dev)
    for g0 in range(0, nv, MAX_ACTIVE):
        vids = list(range(g0, min(g0 + MAX_ACTIVE, nv)))
        pool = DecodePool(C, trans, init, lag=lag, capacity=len(vids), device=dev)
        slot_of = {v: pool.open() for v in vids}
        done = {v: 0 for v in vids}                          # frames of video v pushed so far
        while True:
            call, rows = [], 0
            for v in vids:
                k = min(DECODE_POOL_BURST, off[v + 1] - off[v] - done[v], MAX_ACTIVE - rows)
                if k > 0:
                    call.append((v, k))
                    rows += k
            if not call:
                break
            src, dst_from, dst_to, at = [], [], [], 0
            for v, k in call:
                F = done[v]
                src.extend(range(off[v] + F, off[v] + F + k))
                first, m = max(0, F - lag), max(0, F + k - lag) - max(0, F - lag)       # what this call commits: known without asking
                dst_from.extend(range(at, at + m))
                dst_to.extend(range(off[v] + first, off[v] + first + m))
                done[v] += k
                at += k
            x = scores.index_select(0, torch.tensor(src, dtype=torch.int64).to(dev))
            lab, _, _ = pool.push([slot_of[v] for v, _ in call], x, counts=[k for _, k in call], costs=costs)
            if dst_to:
                labels.index_copy_(0, torch.tensor(dst_to, dtype=torch.int64).to(dev), lab.index_select(0, torch.tensor(dst_from, dtype=torch.int64).to(dev)))
        tail, _ = pool.flush([slot_of[v] for v in vids])
        dst_from, dst_to = [], []
        for i, v in enumerate(vids):
            T = off[v + 1] - off[v]
            first = max(0, T - lag)
            dst_from.extend(range(i * lag, i * lag + T - first))
            dst_to.extend(range(off[v] + first, off[v] + T))
        if dst_to:
            labels.index_copy_(0, torch.tensor(dst_to, dtype=torch.int64).to(dev),
                               tail.reshape(-1).index_select(0, torch.tensor(dst_from, dtype=torch.int64).to(dev)))
        head = pool.headers()                                # int32 [capacity, 8] on the device
        h = head[torch.tensor([slot_of[v] for v in vids], dtype=torch.int64).to(dev)]
        cost = h[:, 4:6].contiguous().view(torch.int64).reshape(-1)
        empty = h[:, 0] == 0
        records[g0:g0 + len(vids), 0] = cost
        records[g0:g0 + len(vids), 1] = torch.where(empty, torch.full_like(cost, -1), h[:, 3].to(torch.int64))
    return labels[:n], records
