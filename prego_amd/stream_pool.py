"""Stream pool: the online detector as one object.  Every live video owns a SLOT of one device block - its GRU state row and its running
aggregation record (utils/aggregate.py:46-90, one id at a time) - and `push` advances any subset of the slots by one frame with the wide
step's bits (prego_miniroad_step_pool: gather, the unchanged prego_miniroad_step_wide, commit + vote; csrc/stream_pool.hip).  `close`
returns what `aggregate` would return for the stream's per-frame predictions ('pred', 'changes_pred'); no argmax crosses to the host on
the way.  `SlotTable` is the host bookkeeping (which slots are open), usable without a device.  `EventFeed` (`pool.event_feed()`,
csrc/stream_feed.hip) tells a live consumer which slots gained an event since it last asked, in one asynchronous report per tick;
`FeedModel` is its host model; `MistakeMonitor` (`pool.mistake_monitor(model)`, csrc/procedure.hip) judges every drained event against a
procedure model on the device, `MonitorModel` is its host model; `DecodePool` is the online fixed-lag Viterbi decoder beside a pool (csrc/decode_pool.hip): the scores a
push returns go into it, and its record - the decoded transcript - serves the same feed and monitors.  `pool.snapshot` / `restore` / `detach` (csrc/stream_image.hip) take live slots out of a pool as a
`PoolSnapshot` of canonical images and put them into a pool again - another pool, other slot numbers, another device or process -,
validated on the device before a slot is written; `image_fault`, `image_layout` and `model_image` are their host model."""
from __future__ import annotations

import ctypes as C
import heapq
import weakref
from typing import NamedTuple

import torch

from . import _stream_call as SC
from ._lib import PregoError
from .aggregate import OVERFLOW_BAD_ID, OVERFLOW_FULL

REC_HEADER = 4               # frames, last vote + 1, n_events, overflow (csrc/stream_pool.hip)
MAX_ACTIVE = 256             # slots per call


def pack_bursts(bursts):
    """[K_s, d] tensors, one per stream in the caller's order -> (packed [sum K_s, d], counts): the rows `step_ragged` / `push_ragged`
    take, stream s at rows off[s] .. off[s] + K_s) with off the prefix sum of counts.  Device-free; the inverse is
    `torch.split(packed, counts)` (`unpack_bursts`)."""
    bursts = list(bursts)
    if not bursts:
        raise PregoError("pack_bursts: no streams")
    for s, b in enumerate(bursts):
        if b.dim() != 2 or b.shape[0] < 1 or b.shape[1] != bursts[0].shape[1] or b.dtype != bursts[0].dtype or b.device != bursts[0].device:
            raise PregoError(f"pack_bursts: stream {s}: expected [K >= 1, {bursts[0].shape[1]}] {bursts[0].dtype} on {bursts[0].device}, got "
                             f"{tuple(b.shape)} {b.dtype} on {b.device}")
    return torch.cat(bursts, dim=0).contiguous(), [int(b.shape[0]) for b in bursts]


def unpack_bursts(packed, counts):
    """the inverse of `pack_bursts`, for packed outputs as well: one [K_s, ...] view per stream"""
    counts = [int(k) for k in counts]
    if packed.shape[0] != sum(counts):
        raise PregoError(f"unpack_bursts: {packed.shape[0]} rows, counts sum to {sum(counts)}")
    return list(torch.split(packed, counts, dim=0))


def burst_offsets(counts):
    """off[s]: the first packed row of stream s"""
    off, at = [], 0
    for k in counts:
        off.append(at)
        at += int(k)
    return off


class SlotTable:
    """Which slots of a pool are open.  open() hands out the lowest free slot."""

    def __init__(self, capacity: int):
        if capacity < 1:
            raise PregoError(f"stream pool: capacity {capacity} (>= 1)")
        self.capacity = int(capacity)
        self._free = list(range(self.capacity))          # a heap: range() is one already
        self._open = set()

    @property
    def free(self) -> int:
        return len(self._free)

    def is_open(self, slot: int) -> bool:
        return slot in self._open

    def open(self, slot=None) -> int:
        """the lowest free slot, or exactly `slot` when a number is given (a pool that mirrors another pool's numbering)"""
        if slot is not None:
            slot = int(slot)
            if not 0 <= slot < self.capacity or slot in self._open:
                raise PregoError(f"stream pool: slot {slot} is " + ("already open" if slot in self._open else f"outside the pool (capacity {self.capacity})"))
            self._free.remove(slot)
            heapq.heapify(self._free)
            self._open.add(slot)
            return slot
        if not self._free:
            raise PregoError(f"stream pool: all {self.capacity} slots are open")
        slot = heapq.heappop(self._free)
        self._open.add(slot)
        return slot

    def release(self, slot: int):
        self.check([slot], "close")
        self._open.remove(slot)
        heapq.heappush(self._free, slot)

    def check(self, slots, who: str) -> list:
        """the slot list of one call as ints: 1..min(256, capacity) open slots, each named once"""
        slots = [int(s) for s in slots]
        n_max = min(MAX_ACTIVE, self.capacity)
        if not 1 <= len(slots) <= n_max:
            raise PregoError(f"stream pool {who}: {len(slots)} slots (1..{n_max} per call)")
        seen = set()
        for s in slots:
            if s not in self._open:
                raise PregoError(f"stream pool {who}: slot {s} is not open" + ("" if 0 <= s < self.capacity else f" (capacity {self.capacity})"))
            if s in seen:
                raise PregoError(f"stream pool {who}: slot {s} is named twice")
            seen.add(s)
        return slots


class _RecordPool:
    """What the two pools share: the slot bookkeeping and the reading of a slot's vote record (csrc/stream_pool.hip).  A subclass sets
    lib, device, p, slots (SlotTable), _block, _vote_window, max_events, _ncls, _ncls_pad and names its C entry points in `_C`."""
    _C = {}                      # 'destroy', 'flush', 'reset', 'record', 'feed_create', 'image_bytes', 'snapshot', 'restore' -> symbol
    _feeds = ()                  # the event feeds attached (a WeakSet once there is one): close() has them forget the slot

    def __del__(self):
        try:
            if getattr(self, "p", None):
                getattr(self.lib, self._C["destroy"])(self.p)
                self.p = None
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise PregoError(f"prego_amd error {rc}: {self.lib.prego_last_error().decode()}")

    # -- bookkeeping ---------------------------------------------------------------------------
    @property
    def capacity(self) -> int:
        return self.slots.capacity

    @property
    def free(self) -> int:
        return self.slots.free

    def open(self) -> int:
        """the lowest free slot; it is zero (after create, after close), so nothing is launched"""
        return self.slots.open()

    @staticmethod
    def _slot_array(slots):
        return (C.c_int32 * len(slots))(*slots)

    def _step_call(self, who, sym, handle, rows, ws_bytes, lead, slots, rgb, flow, bufs, flags, ant_len=None, note=""):
        """What a push entry of either pool does once it knows the row shape of its outputs (the shared steps are prego_amd/_stream_call.py's):
        outputs, checks, workspace and the C call `sym`(handle, pool, n, *lead, slots, rgb, flow, *outs, flags, workspace, bytes, stream).
        ant_len None: the Transformer pool, whose symbols take no anticipation outputs; 0: NULL for them.  note: push_bursts' on its
        packed rows.  A subclass sets _dims = (d_rgb, d_flow, n_classes)."""
        d_rgb, d_flow, ncls = self._dims
        outs, specs = SC.outputs(self.device, rows, ncls, ant_len or 0, *bufs)
        SC.check(who, SC.in_specs(rows, d_rgb, d_flow, rgb, flow) + specs, "{what} as contiguous {dt} cuda {shape}" + note)
        ws = self._ws.fit(ws_bytes, self.device)                 # 0 bytes: the C call refuses the shape with its message
        c_outs = outs if ant_len is None else (outs + (None, None))[:4]
        with torch.cuda.device(self.device):
            self._check(getattr(self.lib, sym)(handle, self.p, len(slots), *lead, self._slot_array(slots), SC.ptr(rgb if d_rgb > 0 else None),
                                               SC.ptr(flow), *[SC.ptr(t) for t in c_outs], flags, SC.ptr(ws), ws.numel(),
                                               C.c_void_p(self._stream_ptr(self.device))))
        return outs

    # -- reading a slot ------------------------------------------------------------------------
    def _record(self, slot: int):
        """one D2H copy of the slot's record (it waits for the stream): (frames, overflow, event ids, event starts)"""
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        self._check(getattr(self.lib, self._C["record"])(self.p, slot, C.byref(ptr), C.byref(nbytes)))
        off = ptr.value - self._block.data_ptr()
        w = self._block[off:off + nbytes.value].view(torch.int32).cpu().numpy()
        n_ev = int(w[2])
        e0 = REC_HEADER + self._ncls_pad
        return int(w[0]), int(w[3]), [int(v) for v in w[e0:e0 + n_ev]], [int(v) for v in w[e0 + self.max_events:e0 + self.max_events + n_ev]]

    def events(self, slot: int) -> dict:
        """{'pred', 'changes_pred', 'frames'}: the step sequence of the slot's finished windows so far ('changes_pred' ends where the last
        finished window ends) and the frames it has taken.  One small D2H copy; it waits."""
        slot = self.slots.check([slot], "events")[0]
        frames, overflow, ev_id, ev_start = self._record(slot)
        self._raise_overflow(slot, overflow)
        return {"pred": ev_id, "changes_pred": ev_start[1:] + [frames - frames % self._vote_window], "frames": frames}

    def _raise_overflow(self, slot: int, overflow: int):
        if overflow & OVERFLOW_BAD_ID:
            raise PregoError(f"stream pool: slot {slot} was fed a step id outside [0, {self._ncls}) (np.bincount of utils/aggregate.py:60 would raise)")
        if overflow & OVERFLOW_FULL:
            raise PregoError(f"stream pool: slot {slot} produced more than max_events = {self.max_events} events; the record dropped the rest")

    def close(self, slot: int) -> dict:
        """Ends the stream: votes its unfinished window, reads the record (one D2H copy), zeroes the slot and frees it.  Returns
        {'pred', 'changes_pred'} as utils/aggregate.py:46-90 gives them for the stream's per-frame predictions; a stream closed before its
        first frame returns {'pred': [], 'changes_pred': [0]}.  Raises PregoError, the slot freed all the same, if the record overflowed
        or met an id outside the classes."""
        slot = self.slots.check([slot], "close")[0]
        arr, s = self._slot_array([slot]), C.c_void_p(self._stream_ptr(self.device))
        with torch.cuda.device(self.device):
            self._check(getattr(self.lib, self._C["flush"])(self.p, 1, arr, s))
            frames, overflow, ev_id, ev_start = self._record(slot)
            self._check(getattr(self.lib, self._C["reset"])(self.p, 1, arr, s))
            for feed in self._feeds:                         # a reopened slot starts at index 0
                feed.forget([slot])
        self.slots.release(slot)
        self._raise_overflow(slot, overflow)
        return {"pred": ev_id, "changes_pred": ev_start[1:] + [frames]}

    def event_feed(self, max_out: int = 1024, depth: int = 2) -> "EventFeed":
        """An `EventFeed` over this pool: `feed.drain()` reports every event that any slot's record gained since the previous drain,
        whatever push variant produced it, in one asynchronous copy of at most `max_out` entries; `depth` reports may be in flight."""
        return EventFeed(self, max_out, depth)

    def mistake_monitor(self, model, max_out: int = 1024, depth: int = 2) -> "MistakeMonitor":
        """A `MistakeMonitor` over this pool: an event feed of its own whose every drained event is judged on the device against the
        procedure model `model` (a `ProcedureModel` or its `.to(device)`; prego_amd/procedure.py) before the report leaves it."""
        return MistakeMonitor(self, model, max_out, depth)

    def forecast_monitor(self, model, max_out: int = 1024, depth: int = 2) -> "ForecastMonitor":
        """A `ForecastMonitor` over this pool: a mistake monitor whose drain also reports, per event, the steps the procedure model
        expects next, and whose `forecast_slots(slots)` asks the same of open slots by name."""
        return ForecastMonitor(self, model, max_out, depth)

    # -- slot images: a live slot as data (csrc/stream_image.hip) ----------------------------------
    def image_geometry(self) -> dict:
        """what an image of this pool's slots must match to be restored here (csrc/pool_image.h: tag words 2..7), as plain ints"""
        kind, dim, window_size, _ = self._image_desc()
        return {"kind": kind, "dim": dim, "window_size": window_size, "n_classes": self._ncls, "vote_window": self._vote_window,
                "max_events": self.max_events}

    def _image_bytes(self) -> int:
        nb = getattr(self.lib, self._C["image_bytes"])(self.p)
        if nb == 0:
            raise PregoError("stream pool: a slot of this pool is too large for an image")
        return nb

    def _open_slots(self, slots, who: str) -> list:
        """any number of open slots, each named once (a C call takes at most 256 of them: the callers go in groups)"""
        slots = [int(s) for s in slots]
        for a in range(0, len(slots), MAX_ACTIVE):
            self.slots.check(slots[a:a + MAX_ACTIVE], who)
        if len(set(slots)) != len(slots):
            raise PregoError(f"stream pool {who}: a slot is named twice")
        return slots

    def _own_feed(self, feed, who: str):
        if feed is not None and getattr(feed, "pool", None) is not self:
            raise PregoError(f"stream pool {who}: the feed belongs to another pool")
        return feed.f if feed is not None else None

    def snapshot(self, slots=None, feed=None) -> "PoolSnapshot":
        """The open slots named (default: all of them, ascending) as a `PoolSnapshot`: one canonical image per slot - state or ring,
        vote record with the unfinished window's counters, and with `feed=` the slot's position in that feed - in one device tensor.
        The pool is only read; nothing waits.  An image is only meaningful for the weights that made it."""
        slots = sorted(self.slots._open) if slots is None else self._open_slots(slots, "snapshot")
        f = self._own_feed(feed, "snapshot")
        _, _, _, dtype = self._image_desc()
        nb = self._image_bytes()
        images = torch.empty((len(slots), nb), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            for a in range(0, len(slots), MAX_ACTIVE):
                grp = slots[a:a + MAX_ACTIVE]
                self._check(getattr(self.lib, self._C["snapshot"])(self.p, f, len(grp), self._slot_array(grp), C.c_void_p(images[a].data_ptr()),
                                                                   len(grp) * nb, C.c_void_p(self._stream_ptr(self.device))))
        return PoolSnapshot(images, self.image_geometry(), dtype)

    def restore(self, snap, feed=None, slots=None) -> list:
        """Puts the streams of `snap` into this pool and returns their slots, image i in slots[i]: `snap.n` slots opened here, lowest
        free first, or `slots` the caller opened and has not pushed to.  With `feed=` every stream goes on in that feed where the
        snapshot's feed stood; every other feed attached to the pool forgets the slots, as `close` has it.  Refused before anything is
        launched: a snapshot of the other pool kind, of another geometry or compute_dtype, too few free slots.  Every image is checked
        on the device before its slot is written (csrc/pool_image.h); if one is refused, the slots opened here are emptied and freed and
        PregoError names image and clause.  One small D2H copy; it waits."""
        if not isinstance(snap, PoolSnapshot):
            raise PregoError(f"stream pool restore: expected a PoolSnapshot, got {type(snap).__name__}")
        f = self._own_feed(feed, "restore")
        geom, (_, _, _, dtype) = self.image_geometry(), self._image_desc()
        if snap.geometry.get("kind") != geom["kind"]:
            raise PregoError(f"stream pool restore: the snapshot is of pool kind {snap.geometry.get('kind')} (1 GRU, 2 Transformer), this pool "
                             f"is kind {geom['kind']}")
        if snap.geometry != geom:
            raise PregoError(f"stream pool restore: the snapshot's geometry {snap.geometry} is not this pool's {geom}")
        if snap.compute_dtype != dtype:
            raise PregoError(f"stream pool restore: the snapshot was taken under compute_dtype {snap.compute_dtype!r}, this pool runs {dtype!r}")
        nb, n = self._image_bytes(), snap.n
        if snap.images.dtype != torch.uint8 or snap.images.dim() != 2 or snap.images.shape[1] != nb:
            raise PregoError(f"stream pool restore: expected images as uint8 [n, {nb}], got {tuple(snap.images.shape)} {snap.images.dtype}")
        opened = slots is None
        if opened:
            if self.free < n:
                raise PregoError(f"stream pool restore: {n} streams, {self.free} free slots")
        else:
            slots = self._open_slots(slots, "restore")
            if len(slots) != n:
                raise PregoError(f"stream pool restore: {n} images, {len(slots)} slots")
        if n == 0:
            return []
        images = snap.images.to(self.device).contiguous()
        if images.data_ptr() % 256:
            images = images.clone()
        if opened:
            slots = [self.slots.open() for _ in range(n)]
        status = torch.empty((n,), dtype=torch.int32, device=self.device)
        s = C.c_void_p(self._stream_ptr(self.device))
        try:
            with torch.cuda.device(self.device):
                for a in range(0, n, MAX_ACTIVE):
                    grp = slots[a:a + MAX_ACTIVE]
                    self._check(getattr(self.lib, self._C["restore"])(self.p, f, len(grp), self._slot_array(grp), C.c_void_p(images[a].data_ptr()),
                                                                      len(grp) * nb, C.c_void_p(status[a:].data_ptr()), s))
                for other in self._feeds:                        # as close(): a feed that was not named starts the slots at index 0
                    if other is not feed:
                        for a in range(0, n, MAX_ACTIVE):
                            other.forget(slots[a:a + MAX_ACTIVE])
                faults = status.cpu().tolist()
        except Exception:
            if opened:
                self._drop(slots)
            raise
        bad = [(i, v) for i, v in enumerate(faults) if v]
        if bad:
            if opened:
                self._drop(slots)
            raise PregoError("stream pool restore: " + "; ".join(f"image {i} refused ({', '.join(image_fault_names(v))})" for i, v in bad[:8]) +
                             (f" and {len(bad) - 8} more" if len(bad) > 8 else ""))
        return slots

    def _drop(self, slots):
        """empties the slots, has every feed forget them and frees them: no flush, nothing read"""
        with torch.cuda.device(self.device):
            for a in range(0, len(slots), MAX_ACTIVE):
                grp = slots[a:a + MAX_ACTIVE]
                self._check(getattr(self.lib, self._C["reset"])(self.p, len(grp), self._slot_array(grp), C.c_void_p(self._stream_ptr(self.device))))
                for feed in self._feeds:
                    feed.forget(grp)
        for slot in slots:
            self.slots.release(slot)

    def detach(self, slots, feed=None) -> "PoolSnapshot":
        """`snapshot(slots, feed)`, then the slots are emptied and freed and every feed forgets them.  Nothing is flushed: the unfinished
        window travels in the image.  Nothing waits."""
        slots = self._open_slots(slots, "detach")
        snap = self.snapshot(slots, feed)
        self._drop(slots)
        return snap


FEED_COUNT_MASK, FEED_REP_SHIFT = (1 << 30) - 1, 30          # a feed's cursor word (csrc/stream_feed.hip)


class FeedModel:
    """Host model of an event feed (csrc/stream_feed.hip) over `OnlineRecord`s, usable without a device: `records[slot]` is the slot's
    record (the list is the caller's: putting a fresh OnlineRecord in place is a reset behind the feed's back).  `drain()` returns
    {'count', 'pending', 'seq', 'entries'} with entries (slot, index, step id, first frame) in ascending slot order, then ascending
    index; a slot's newly set overflow bits are the entry (slot, -1, bits, frames) in front of its events.  At most `max_out` entries
    per drain: the cursors move only past what was written and the next drain goes on from there."""

    def __init__(self, records, max_out: int = 1024):
        if max_out < 1:
            raise ValueError(f"FeedModel: max_out {max_out} (>= 1)")
        self.records, self.max_out = records, int(max_out)
        self.delivered, self.reported, self.seq = [0] * len(records), [0] * len(records), 0

    def drain(self) -> dict:
        entries, due = [], 0
        for slot, rec in enumerate(self.records):
            n = min(len(rec.event_id), rec.max_events)
            if n < self.delivered[slot] or self.reported[slot] & ~rec.overflow:      # the record was reset behind the feed's back
                self.delivered[slot], self.reported[slot] = 0, 0
            fresh = rec.overflow & ~self.reported[slot]
            if fresh:
                due += 1
                if len(entries) < self.max_out:
                    entries.append((slot, -1, fresh, rec.frames))
                    self.reported[slot] |= fresh
            for i in range(self.delivered[slot], n):
                due += 1
                if len(entries) < self.max_out:
                    entries.append((slot, i, rec.event_id[i], rec.event_start[i]))
                    self.delivered[slot] = i + 1
        self.seq += 1
        return {"count": len(entries), "pending": due - len(entries), "seq": self.seq, "entries": entries}

    def forget(self, slots):
        for s in slots:
            self.delivered[s], self.reported[s] = 0, 0

    def cursor(self, slot: int) -> int:
        """the slot's cursor word as the device keeps it"""
        return self.delivered[slot] | self.reported[slot] << FEED_REP_SHIFT

    cursor_word = cursor                                         # the word a slot image carries in its tag

    def seek(self, slot: int, cursor_word: int):
        """the slot's cursor set from a cursor word: what `restore(snap, feed=...)` does with the word in an image's tag"""
        word = int(cursor_word) & 0xFFFFFFFF
        self.delivered[slot], self.reported[slot] = word & FEED_COUNT_MASK, word >> FEED_REP_SHIFT


# ---- slot images: the host model (csrc/pool_image.h) ---------------------------------------------------------------------------
IMAGE_MAGIC, IMAGE_VERSION, IMAGE_TAG_WORDS = 0x474D4950, 1, 16
IMAGE_GRU, IMAGE_VIT = 1, 2
TAG_FRAMES, TAG_HEAD, TAG_FILL, TAG_CURSOR = 8, 9, 10, 11
IMAGE_FAULTS = {1: "geometry", 2: "frames", 4: "n_events", 8: "last vote", 16: "overflow word", 32: "counter", 64: "ring head / fill",
                128: "feed cursor"}
FAULT_GEOMETRY, FAULT_FRAMES, FAULT_EVENTS, FAULT_VOTE, FAULT_OVERFLOW, FAULT_COUNTER, FAULT_RING, FAULT_CURSOR = IMAGE_FAULTS


def image_fault_names(fault: int) -> list:
    """the clauses a status word of `restore` names"""
    return [name for bit, name in IMAGE_FAULTS.items() if fault & bit]


def image_layout(geometry: dict) -> dict:
    """word counts of a slot image of this geometry: {'state_words', 'rec_words', 'image_words', 'ncls_pad'}; the tag is words
    [0, 16), the state [16, 16 + state_words), the record the rec_words behind it, zeros up to image_words (a multiple of 64)"""
    g = geometry
    pad = (g["n_classes"] + 3) // 4 * 4
    rec = (REC_HEADER + pad + 2 * g["max_events"] + 3) // 4 * 4
    state = g["window_size"] * g["dim"] if g["kind"] == IMAGE_VIT else g["dim"]
    return {"state_words": state, "rec_words": rec, "image_words": (IMAGE_TAG_WORDS + state + rec + 63) // 64 * 64, "ncls_pad": pad}


def image_geometry_words(geometry: dict) -> list:
    """tag words 0..7 of every image a pool of this geometry writes and accepts"""
    g = geometry
    return [IMAGE_MAGIC, IMAGE_VERSION, g["kind"], g["dim"], g["window_size"] if g["kind"] == IMAGE_VIT else 0, g["n_classes"],
            g["vote_window"], g["max_events"]]


def image_fault(words, geometry: dict) -> int:
    """The validity rule of `restore` (csrc/pool_image.h: pool_image_fault) on an image's int32 words: 0 = a pool of `geometry` restores
    it, else the clause bits the device writes into `status` (IMAGE_FAULTS)."""
    lay, g = image_layout(geometry), geometry
    r0 = IMAGE_TAG_WORDS + lay["state_words"]
    tag = [int(v) for v in words[:IMAGE_TAG_WORDS]]
    rec = [int(v) for v in words[r0:r0 + REC_HEADER + lay["ncls_pad"]]]
    f = 0
    if tag[:8] != image_geometry_words(g):
        f |= FAULT_GEOMETRY
    frames, n_events = tag[TAG_FRAMES], rec[2]
    if frames < 0 or rec[0] != frames:
        f |= FAULT_FRAMES
    if not 0 <= n_events <= g["max_events"]:
        f |= FAULT_EVENTS
    if not 0 <= rec[1] <= g["n_classes"]:
        f |= FAULT_VOTE
    if not 0 <= rec[3] <= 3:
        f |= FAULT_OVERFLOW
    if any(not 0 <= c <= g["vote_window"] for c in rec[REC_HEADER:]):
        f |= FAULT_COUNTER
    if g["kind"] == IMAGE_VIT and frames >= 0:
        T = g["window_size"]
        if tag[TAG_HEAD] != frames % T or tag[TAG_FILL] != min(frames, T):
            f |= FAULT_RING
    if (tag[TAG_CURSOR] & 0xFFFFFFFF) & FEED_COUNT_MASK > max(n_events, 0):
        f |= FAULT_CURSOR
    return f


def model_image(geometry: dict, record, state=None, cursor_word: int = 0) -> list:
    """The int32 words of the image `snapshot` writes for a slot whose record is `record` (an OnlineRecord): the tag, `state` (the
    state_words 32-bit patterns as ints; default zeros - for the Transformer pool the rows [0, fill) are the caller's to fill, the rest
    must stay zero), `record.to_words`, zeros.  head and fill follow from the record's frames."""
    lay, g = image_layout(geometry), geometry
    frames = record.frames
    T = g["window_size"] if g["kind"] == IMAGE_VIT else 0
    cur = int(cursor_word) & 0xFFFFFFFF
    tag = image_geometry_words(g) + [frames, frames % T if T else 0, min(frames, T) if T else 0, cur - (1 << 32) if cur >> 31 else cur, 0, 0, 0, 0]
    state = [0] * lay["state_words"] if state is None else [int(v) for v in state]
    if len(state) != lay["state_words"]:
        raise ValueError(f"model_image: {len(state)} state words, the geometry has {lay['state_words']}")
    w = tag + state + record.to_words(g["n_classes"], g["max_events"])
    return w + [0] * (lay["image_words"] - len(w))


class PoolSnapshot:
    """Slots of a stream pool as data (`pool.snapshot` / `pool.detach`): `images` uint8 [n, image_bytes], one canonical image per slot
    (csrc/pool_image.h), `geometry` - the plain dict `pool.image_geometry()` gave -, `compute_dtype` and `n`.  It lives where `images`
    lives: `.cpu()` / `.to(device)` move it, `.save(path)` / `PoolSnapshot.load(path)` put it through a file (`torch.save` of a plain
    dict, loadable with weights_only=True).  An image is only meaningful for the weights that made it: `restore` checks geometry and
    compute_dtype, the weights are the caller's business."""
    FORMAT = "prego_amd.PoolSnapshot/1"

    def __init__(self, images, geometry: dict, compute_dtype: str):
        if images.dtype != torch.uint8 or images.dim() != 2:
            raise PregoError(f"PoolSnapshot: expected images as uint8 [n, image_bytes], got {tuple(images.shape)} {images.dtype}")
        self.images, self.geometry, self.compute_dtype = images, {k: int(v) for k, v in geometry.items()}, str(compute_dtype)
        if images.shape[1] != 4 * image_layout(self.geometry)["image_words"]:
            raise PregoError(f"PoolSnapshot: images of {images.shape[1]} bytes, the geometry {self.geometry} has "
                             f"{4 * image_layout(self.geometry)['image_words']}")

    @property
    def n(self) -> int:
        return int(self.images.shape[0])

    @property
    def device(self):
        return self.images.device

    def to(self, device) -> "PoolSnapshot":
        return PoolSnapshot(self.images.to(device), self.geometry, self.compute_dtype)

    def cpu(self) -> "PoolSnapshot":
        return self.to("cpu")

    def words(self):
        """the images as int32 [n, image_words] (a view)"""
        return self.images.view(torch.int32)

    def frames(self) -> list:
        """frames each stream has taken, from the tags; it waits for the device"""
        return self.words()[:, TAG_FRAMES].tolist()

    def save(self, path):
        torch.save({"format": self.FORMAT, "images": self.images.cpu().contiguous(), "geometry": dict(self.geometry),
                    "compute_dtype": self.compute_dtype, "n": self.n}, path)

    @classmethod
    def load(cls, path) -> "PoolSnapshot":
        d = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(d, dict) or d.get("format") != cls.FORMAT:
            raise PregoError(f"PoolSnapshot.load: {path} is not a saved PoolSnapshot ({cls.FORMAT})")
        snap = cls(d["images"], d["geometry"], d["compute_dtype"])
        if snap.n != d["n"]:
            raise PregoError(f"PoolSnapshot.load: {path} says n = {d['n']}, its images hold {snap.n}")
        return snap


class FeedTicket:
    """One drain in flight: `ready()` - has the report landed in host memory; `events()` - waits if it must, returns the entries as
    (slot, index, step, start) and hands the buffer back to the feed; `pending` - entries the report had no room for (the next drain
    brings them); `count`, `seq` - the header; `entries` - the report as it is, overflow entries (index -1) included, and like
    `events()` it hands the buffer back."""

    def __init__(self, feed, k: int):
        self._feed, self._k, self._report, self._read = feed, k, None, False

    def ready(self) -> bool:
        return self._report is not None or self._feed._done[self._k].query()

    def _wait(self):
        if self._report is None:
            self._feed._done[self._k].synchronize()
            w = self._feed._host[self._k]
            count = int(w[0])
            if not 0 <= count <= self._feed.max_out:
                raise PregoError(f"event feed: a report with count {count} (max_out {self._feed.max_out})")
            self._report = (count, int(w[1]), int(w[2]), [tuple(r) for r in w[4:4 + 4 * count].view(count, 4).tolist()])
        return self._report

    @property
    def count(self) -> int:
        return self._wait()[0]

    @property
    def pending(self) -> int:
        return self._wait()[1]

    @property
    def seq(self) -> int:
        return self._wait()[2]

    @property
    def entries(self) -> list:
        ent = self._wait()[3]
        self._read = True                                        # as events(): the report has reached the caller
        return list(ent)

    def events(self) -> list:
        """[(slot, index, step, start)]; raises PregoError, in `events(slot)`'s words, if a slot's record overflowed or met an id
        outside the classes (the ticket counts as read all the same; `entries` still holds the whole report)"""
        ent = self._wait()[3]
        self._read = True                                        # the host buffer is the feed's again
        for slot, index, bits, _ in ent:
            if index < 0:
                self._feed.pool._raise_overflow(slot, bits)
        return list(ent)


class EventFeed:
    """EventFeed(pool, max_out=1024, depth=2) - `pool.event_feed(...)`: a live consumer's view of either pool (csrc/stream_feed.hip).
    `drain()` enqueues, on the current stream, one scan of every slot's record and one non-blocking copy of the report (at most
    `max_out` entries, 16 bytes each) into one of `depth` pinned host buffers, and returns a `FeedTicket` without waiting.  The
    cursors advance on the device when the drain runs, so an unread ticket holds events nobody else will be handed: `drain()` raises,
    before it launches anything, when all `depth` buffers hold unread tickets.  The pool's `close` has the feed forget the slot."""

    def __init__(self, pool, max_out: int = 1024, depth: int = 2):
        self.pool, self.lib, self.device = pool, pool.lib, pool.device
        self.max_out, self.depth = int(max_out), int(depth)
        if self.depth < 1:
            raise PregoError(f"event feed: depth {depth} (>= 1)")
        need = self.lib.prego_stream_pool_feed_bytes(pool.capacity, self.max_out)
        self._report_bytes = self.lib.prego_stream_pool_feed_report_bytes(self.max_out)
        if need == 0 or self._report_bytes == 0:
            raise PregoError(f"event feed: max_out {max_out} (1..{1 << 24} entries per report)")
        self._block = torch.empty(need, dtype=torch.uint8, device=self.device)
        self._dev = [torch.empty(self._report_bytes, dtype=torch.uint8, device=self.device) for _ in range(self.depth)]
        self._host = [torch.empty(self._report_bytes // 4, dtype=torch.int32).pin_memory() for _ in range(self.depth)]
        self._done = [torch.cuda.Event() for _ in range(self.depth)]
        self._tickets = [None] * self.depth
        self._next = 0
        self.f = None
        f = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = getattr(self.lib, pool._C["feed_create"])(C.byref(f), pool.p, self.max_out, C.c_void_p(self._block.data_ptr()), need,
                                                           C.c_void_p(pool._stream_ptr(self.device)))
        pool._check(rc)
        self.f = f
        if not isinstance(pool._feeds, weakref.WeakSet):
            pool._feeds = weakref.WeakSet()
        pool._feeds.add(self)

    def __del__(self):
        try:
            if getattr(self, "f", None):
                self.lib.prego_stream_pool_feed_destroy(self.f)
                self.f = None
        except Exception:
            pass

    def drain(self) -> FeedTicket:
        k = self._next
        held = self._tickets[k]
        if held is not None and not held._read:                  # the oldest buffer: if it is unread, all of them are
            raise PregoError(f"event feed drain: all {self.depth} report buffers hold unread tickets (read one with events(); the "
                             "cursors advance when a drain runs, so its events would reach nobody)")
        with torch.cuda.device(self.device):
            self.pool._check(self.lib.prego_stream_pool_feed_drain(self.f, C.c_void_p(self._dev[k].data_ptr()), self._report_bytes,
                                                                   C.c_void_p(self.pool._stream_ptr(self.device))))
            self._host[k].copy_(self._dev[k].view(torch.int32), non_blocking=True)
            self._done[k].record()
        ticket = FeedTicket(self, k)
        self._tickets[k] = ticket
        self._next = (k + 1) % self.depth
        return ticket

    def forget(self, slots):
        """zeroes the cursors of `slots` (any slots of the pool, each named once): what `close` does for the slot it frees"""
        slots = [int(s) for s in slots]
        with torch.cuda.device(self.device):
            self.pool._check(self.lib.prego_stream_pool_feed_forget(self.f, len(slots), self.pool._slot_array(slots),
                                                                    C.c_void_p(self.pool._stream_ptr(self.device))))


class MonitorModel:
    """Host model of a `MistakeMonitor`, usable without a device and the counterpart of `FeedModel`: a FeedModel over `records`, a group
    per slot (-1 until `set_group`; `forget` - what the pool's close does - puts it back) and the `ProcedureModel` that judges.
    `drain()` returns FeedModel's dict with 'verdicts', one `Verdict` per entry: the entry's step after the slot's events in front of
    it, in the slot's group; an overflow entry, or an event the record no longer holds, is SKIPPED."""

    def __init__(self, records, model, max_out: int = 1024):
        self.feed, self.model, self.records = FeedModel(records, max_out), model, records
        self.groups = [-1] * len(records)

    def set_group(self, slots, groups):
        for s, g in zip(slots, groups):
            self.groups[s] = int(g)

    def forget(self, slots):
        self.feed.forget(slots)
        for s in slots:
            self.groups[s] = -1

    def judge_entry(self, entry):
        from .procedure import SKIPPED_VERDICT
        slot, index, step, _ = entry
        rec = self.records[slot]
        if index < 0 or index >= min(len(rec.event_id), rec.max_events):
            return SKIPPED_VERDICT
        return self.model.judge(rec.event_id[:index], step, self.groups[slot])

    def drain(self) -> dict:
        r = self.feed.drain()
        r["verdicts"] = [self.judge_entry(e) for e in r["entries"]]
        return r

    def forecast_entry(self, entry):
        """what a `ForecastMonitor` reports beside the entry's verdict: the forecast after the slot's events in front of it and its own
        step; SKIPPED where the verdict is"""
        from .procedure import SKIPPED_FORECAST
        slot, index, step, _ = entry
        rec = self.records[slot]
        if index < 0 or index >= min(len(rec.event_id), rec.max_events):
            return SKIPPED_FORECAST
        return self.model.forecast(list(rec.event_id[:index]) + [step], self.groups[slot])

    def forecast_slots(self, slots) -> list:
        """`ForecastMonitor.forecast_slots`: the forecast after every event a slot's record holds; a slot outside the records is SKIPPED"""
        from .procedure import SKIPPED_FORECAST
        out = []
        for s in slots:
            if not 0 <= s < len(self.records):
                out.append(SKIPPED_FORECAST)
                continue
            rec = self.records[s]
            out.append(self.model.forecast(rec.event_id[:min(len(rec.event_id), rec.max_events)], self.groups[s]))
        return out


class _MonitorFeed(EventFeed):
    """the feed a monitor owns: a slot the pool has it forget (close, detach, a restore that does not name it) loses its group too"""
    _monitor = None

    def forget(self, slots):
        super().forget(slots)
        mon = self._monitor() if self._monitor is not None else None
        if mon is not None:
            mon._ungroup([int(s) for s in slots])


class MonitorTicket:
    """One monitor drain in flight: `events()` - the report's entries (slot, index, step, start), overflow entries (index -1) included -
    and `verdicts()` - one `Verdict` per entry, index-aligned; both wait if they must and hand the buffers back to the monitor.
    `count`, `pending`, `seq`, `ready()` as `FeedTicket` has them."""

    def __init__(self, monitor, feed_ticket, k: int):
        self._mon, self._ft, self._k, self._got = monitor, feed_ticket, k, None

    def ready(self) -> bool:
        return self._got is not None or self._mon._done[self._k].query()

    def _wait(self):
        if self._got is None:
            from .procedure import VERDICT_WORDS, Verdict
            self._mon._done[self._k].synchronize()               # recorded behind the verdict copy: the report has landed as well
            entries = self._ft.entries                           # hands the report buffer back
            rows = self._mon._host[self._k][:VERDICT_WORDS * len(entries)].view(len(entries), VERDICT_WORDS).tolist()
            self._got = (entries, [Verdict.from_words(w) for w in rows])
        return self._got

    count = property(lambda self: self._ft.count)
    pending = property(lambda self: self._ft.pending)
    seq = property(lambda self: self._ft.seq)

    def events(self) -> list:
        return list(self._wait()[0])

    def verdicts(self) -> list:
        return list(self._wait()[1])


class MistakeMonitor:
    """MistakeMonitor(pool, model, max_out=1024, depth=2) - `pool.mistake_monitor(model)`: online mistake detection behind the drain
    (csrc/procedure.hip).  It owns an `EventFeed` (`.feed`), a group per slot on the device (-1: judged against every group) and
    `depth` pinned verdict buffers.  `drain()` enqueues, on the current stream, the feed's drain, one judging launch over the report
    where it lies and both copies, and returns a `MonitorTicket` without waiting.  `set_group(slots, groups)` is stream-ordered: it
    holds for the drains enqueued after it.  When the pool closes a slot its group goes back to -1; slot images carry no group, so a
    restored slot has -1 until `set_group`."""

    def __init__(self, pool, model, max_out: int = 1024, depth: int = 2):
        from .procedure import VERDICT_WORDS, ProcedureModel
        self.pool, self.lib, self.device = pool, pool.lib, pool.device
        self.model = model.to(self.device, lib=self.lib) if isinstance(model, ProcedureModel) else model
        if getattr(self.model, "m", None) is None or torch.device(self.model.device) != torch.device(self.device):
            raise PregoError(f"mistake monitor: expected a ProcedureModel or its .to({self.device}), got {type(model).__name__}")
        self.feed = _MonitorFeed(pool, max_out, depth)
        self.feed._monitor = weakref.ref(self)
        self.max_out, self.depth = self.feed.max_out, self.feed.depth
        self._judge = getattr(self.lib, pool._C["feed_create"].replace("_feed_create", "_feed_judge"))
        self._groups = torch.full((pool.capacity,), -1, dtype=torch.int32, device=self.device)
        self._dev = [torch.empty(self.max_out * VERDICT_WORDS, dtype=torch.int32, device=self.device) for _ in range(self.depth)]
        self._host = [torch.empty(self.max_out * VERDICT_WORDS, dtype=torch.int32).pin_memory() for _ in range(self.depth)]
        self._done = [torch.cuda.Event() for _ in range(self.depth)]

    def set_group(self, slots, groups):
        """group groups[i] (>= -1) for open slot slots[i], from the next drain on"""
        slots = self.pool._open_slots(slots, "mistake monitor set_group")
        groups = [int(g) for g in groups]
        if len(groups) != len(slots) or any(g < -1 for g in groups):
            raise PregoError(f"mistake monitor set_group: {len(slots)} slots, groups {groups} (one per slot, each >= -1)")
        self._put(slots, groups)

    def _put(self, slots, groups):
        with torch.cuda.device(self.device):
            self._groups.index_copy_(0, torch.tensor(slots, dtype=torch.int64).to(self.device), torch.tensor(groups, dtype=torch.int32).to(self.device))

    def _ungroup(self, slots):
        self._put(slots, [-1] * len(slots))

    def groups(self) -> list:
        """the group of every slot; it waits for the stream"""
        return self._groups.cpu().tolist()

    def drain(self) -> MonitorTicket:
        k = self.feed._next
        ft = self.feed.drain()                                   # raises, before anything is launched, when buffer k is unread
        with torch.cuda.device(self.device):
            self.pool._check(self._judge(self.feed.f, self.model.m, C.c_void_p(self.feed._dev[k].data_ptr()), self.feed._report_bytes,
                                         C.c_void_p(self._groups.data_ptr()), C.c_void_p(self._dev[k].data_ptr()), self._dev[k].numel() * 4,
                                         C.c_void_p(self.pool._stream_ptr(self.device))))
            self._host[k].copy_(self._dev[k], non_blocking=True)
            self._done[k].record()
        return MonitorTicket(self, ft, k)


class ForecastTicket(MonitorTicket):
    """One forecast-monitor drain in flight: a `MonitorTicket` that adds `forecasts()`, one `Forecast` per entry, index-aligned with
    `events()` and `verdicts()`: what the model expects after that event.  The first read waits for all three copies."""

    def _wait(self):
        if self._got is None:
            from .procedure import FORECAST_WORDS, Forecast
            self._mon._fdone[self._k].synchronize()              # recorded behind the forecast copy: report and verdicts have landed
            entries, verdicts = super()._wait()
            rows = self._mon._fhost[self._k][:FORECAST_WORDS * len(entries)].view(len(entries), FORECAST_WORDS).tolist()
            self._got = (entries, verdicts, [Forecast.from_words(w) for w in rows])
        return self._got

    def ready(self) -> bool:
        return self._got is not None or self._mon._fdone[self._k].query()

    def forecasts(self) -> list:
        return list(self._wait()[2])


class SlotForecastTicket:
    """One `forecast_slots` call in flight: `forecasts()` - one `Forecast` per slot named, in the caller's order; it waits if it must and
    hands the buffer back to the monitor.  `ready()` as `FeedTicket` has it."""

    def __init__(self, monitor, k: int, n: int):
        self._mon, self._k, self._n, self._got = monitor, k, n, None

    def ready(self) -> bool:
        return self._got is not None or self._mon._sdone[self._k].query()

    def forecasts(self) -> list:
        if self._got is None:
            from .procedure import FORECAST_WORDS, Forecast
            self._mon._sdone[self._k].synchronize()
            rows = self._mon._shost[self._k][:FORECAST_WORDS * self._n].view(self._n, FORECAST_WORDS).tolist()
            self._got = [Forecast.from_words(w) for w in rows]
        return list(self._got)


class ForecastMonitor(MistakeMonitor):
    """ForecastMonitor(pool, model, max_out=1024, depth=2) - `pool.forecast_monitor(model)`: a `MistakeMonitor` that also says what should
    come next (csrc/procedure.hip).  `drain()` enqueues the feed's drain, the judge, one forecasting launch over the
    same report and the three copies, and returns a `ForecastTicket` without waiting.  `forecast_slots(slots)` asks for open slots by
    name - whatever their records hold now, drained or not - in one launch and one copy into one of `depth` pinned buffers of its own;
    it raises, before it launches anything, when all of them hold unread tickets."""

    def __init__(self, pool, model, max_out: int = 1024, depth: int = 2):
        from .procedure import FORECAST_WORDS
        super().__init__(pool, model, max_out, depth)
        self._fw = FORECAST_WORDS
        stem = pool._C["feed_create"].replace("_feed_create", "")
        self._forecast, self._slot_forecast = getattr(self.lib, stem + "_feed_forecast"), getattr(self.lib, stem + "_forecast")
        words = lambda n: torch.empty(n * FORECAST_WORDS, dtype=torch.int32, device=self.device)
        pinned = lambda n: torch.empty(n * FORECAST_WORDS, dtype=torch.int32).pin_memory()
        self._fdev, self._fhost = [words(self.max_out) for _ in range(self.depth)], [pinned(self.max_out) for _ in range(self.depth)]
        self._fdone = [torch.cuda.Event() for _ in range(self.depth)]
        cap = pool.capacity
        self._sdev, self._shost = [words(cap) for _ in range(self.depth)], [pinned(cap) for _ in range(self.depth)]
        self._slots_host = [torch.empty(cap, dtype=torch.int32).pin_memory() for _ in range(self.depth)]
        self._slots_dev = [torch.empty(cap, dtype=torch.int32, device=self.device) for _ in range(self.depth)]
        self._sdone = [torch.cuda.Event() for _ in range(self.depth)]
        self._stickets, self._snext = [None] * self.depth, 0

    def drain(self) -> ForecastTicket:
        t = super().drain()                                      # raises, before anything is launched, when buffer k is unread
        k = t._k
        with torch.cuda.device(self.device):
            self.pool._check(self._forecast(self.feed.f, self.model.m, C.c_void_p(self.feed._dev[k].data_ptr()), self.feed._report_bytes,
                                            C.c_void_p(self._groups.data_ptr()), C.c_void_p(self._fdev[k].data_ptr()), self._fdev[k].numel() * 4,
                                            C.c_void_p(self.pool._stream_ptr(self.device))))
            self._fhost[k].copy_(self._fdev[k], non_blocking=True)
            self._fdone[k].record()
        return ForecastTicket(self, t._ft, k)

    def forecast_slots(self, slots) -> SlotForecastTicket:
        """what comes next for each of `slots` (open slots, 1..capacity of them, a slot may repeat), in the group `set_group` gave it"""
        slots = [int(s) for s in slots]
        if not 1 <= len(slots) <= self.pool.capacity:
            raise PregoError(f"forecast monitor forecast_slots: {len(slots)} slots (1..{self.pool.capacity}, the pool's capacity)")
        for s in slots:
            if not self.pool.slots.is_open(s):
                raise PregoError(f"forecast monitor forecast_slots: slot {s} is not open")
        k = self._snext
        held = self._stickets[k]
        if held is not None and held._got is None:               # the oldest buffer: if it is unread, all of them are
            raise PregoError(f"forecast monitor forecast_slots: all {self.depth} forecast buffers hold unread tickets (read one with forecasts())")
        n = len(slots)
        self._slots_host[k][:n] = torch.tensor(slots, dtype=torch.int32)
        with torch.cuda.device(self.device):
            self._slots_dev[k][:n].copy_(self._slots_host[k][:n], non_blocking=True)
            self.pool._check(self._slot_forecast(self.pool.p, self.model.m, C.c_void_p(self._slots_dev[k].data_ptr()), n,
                                                 C.c_void_p(self._groups.data_ptr()), C.c_void_p(self._sdev[k].data_ptr()), self._sdev[k].numel() * 4,
                                                 C.c_void_p(self.pool._stream_ptr(self.device))))
            self._shost[k][:n * self._fw].copy_(self._sdev[k][:n * self._fw], non_blocking=True)
            self._sdone[k].record()
        ticket = SlotForecastTicket(self, k, n)
        self._stickets[k] = ticket
        self._snext = (k + 1) % self.depth
        return ticket


class StreamPool(_RecordPool):
    """StreamPool(model_or_engine, capacity=256, window=200, max_events=1024): `capacity` slots of GRU state + vote record in one device
    block; a record holds up to `max_events` (step id, first frame) events of `window`-frame majority votes.
    `push` needs an engine the streaming kernels are built for (bf16 / fp16 operands, hidden_dim 1024, one GRU layer); `vote`, `events`
    and `close` serve every engine (ids from the Transformer path or a general forward); live Transformer streams have a pool of their
    own, `TransformerStreamPool` below (`ViTEnc.stream_pool`)."""
    _C = {"destroy": "prego_stream_pool_destroy", "flush": "prego_stream_pool_flush", "reset": "prego_stream_pool_reset",
          "record": "prego_stream_pool_record", "feed_create": "prego_stream_pool_feed_create",
          "image_bytes": "prego_stream_pool_image_bytes", "snapshot": "prego_stream_pool_snapshot", "restore": "prego_stream_pool_restore"}

    def _image_desc(self):
        return IMAGE_GRU, self._hid, 0, self.engine.compute_dtype

    def __init__(self, model_or_engine, capacity: int = 256, window: int = 200, max_events: int = 1024):
        from .engine import _stream_ptr
        eng = model_or_engine.engine() if hasattr(model_or_engine, "engine") else model_or_engine
        self.engine, self.lib, self.device = eng, eng.lib, eng.device
        self.window, self.max_events = int(window), int(max_events)
        self._vote_window = self.window
        self.slots = SlotTable(capacity)
        self._stream_ptr = _stream_ptr
        d_rgb, d_flow, emb, hid, ncls = eng.dims
        self._hid, self._ncls, self._ncls_pad, self._dims = hid, ncls, (ncls + 3) // 4 * 4, (d_rgb, d_flow, ncls)
        need = self.lib.prego_stream_pool_bytes(eng.h, int(capacity), self.max_events)
        if need == 0:
            raise PregoError(f"stream pool: capacity {capacity}, max_events {max_events} (each 1..{1 << 20})")
        self._block = torch.empty(need, dtype=torch.uint8, device=self.device)
        self._ws = SC.Workspace()
        p = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.prego_stream_pool_create(C.byref(p), eng.h, int(capacity), self.window, self.max_events, C.c_void_p(self._block.data_ptr()),
                                                   need, C.c_void_p(_stream_ptr(self.device)))
        self._check(rc)
        self.p = p

    # -- frames for a subset of the streams ---------------------------------------------------------
    _ADVICE = "run the general forward and feed its ids to vote()"

    def push(self, slots, rgb, flow=None, softmax: bool = True, want_ant=None, out=None, argmax=None, ant_out=None, ant_argmax=None):
        """One new frame for each open slot of `slots`: rgb [n, d_rgb] / flow [n, d_flow] (None = zero flow) fp32 cuda contiguous, rows in
        `slots` order.  Returns step_wide's tuple - (out [n, C], argmax int32 [n]) and, with want_ant (default: the model has an
        anticipation head), (ant_out [n, L, C], ant_argmax int32 [n, L]) - bit for bit what step_wide returns for a dense call of these
        streams; each slot's state is advanced and its record takes the frame's argmax.  Pass buffers to reuse them."""
        eng, who = self.engine, "stream pool push"
        SC.refuse_general(who, eng.compute_dtype, self._hid, eng.num_layers, self._ADVICE)
        slots = self.slots.check(slots, "push")
        n = len(slots)
        want_ant = SC.resolve_ant(who, want_ant, getattr(eng, "ant_len", 0))
        SC.frame_source(who, eng.dims[0], rgb, flow)
        return self._step_call(who, "prego_miniroad_step_pool", eng.h, (n,), self.lib.prego_miniroad_step_pool_workspace_bytes(eng.h, n), (), slots,
                               rgb, flow, (out, argmax, ant_out, ant_argmax), 1 if softmax else 0, eng.ant_len if want_ant else 0)

    def push_frames(self, slots, rgb, flow=None, softmax: bool = True, want_ant=None, out=None, argmax=None, ant_out=None, ant_argmax=None):
        """K new frames for each open slot of `slots` in one call (prego_miniroad_step_pool_frames): rgb [n, K, d_rgb] / flow [n, K, d_flow]
        (None = zero flow) fp32 cuda contiguous, 1 <= K <= 32 the same for every slot, n K <= 256 - slots with different backlogs: `push_ragged`;
        a backlog longer than 32 frames is forward()'s work (h0 / h_last).  Returns `push`'s tuple with a K axis: (out [n, K, C],
        argmax int32 [n, K]) and, with want_ant, (ant_out [n, K, L, C], ant_argmax int32 [n, K, L]); every frame's bits are `push`'s for a
        call of 5..256 slots.  Each slot's state is advanced by K frames and its record is word for word the record after K `push`
        calls: the K ids are voted in frame order, window boundaries inside the burst included."""
        eng, who = self.engine, "stream pool push_frames"
        SC.refuse_general(who, eng.compute_dtype, self._hid, eng.num_layers, self._ADVICE)
        slots = self.slots.check(slots, "push_frames")
        n = len(slots)
        want_ant = SC.resolve_ant(who, want_ant, getattr(eng, "ant_len", 0))
        src = SC.frame_source(who, eng.dims[0], rgb, flow, "frames")
        if src.dim() != 3 or src.shape[0] != n:
            raise PregoError(f"stream pool push_frames: expected frames as [{n}, K, d], got {tuple(src.shape)}")
        K = int(src.shape[1])
        return self._step_call(who, "prego_miniroad_step_pool_frames", eng.h, (n, K), self.lib.prego_miniroad_step_pool_frames_workspace_bytes(eng.h, n, K),
                               (K,), slots, rgb, flow, (out, argmax, ant_out, ant_argmax), 1 if softmax else 0, eng.ant_len if want_ant else 0)

    def push_ragged(self, slots, counts, rgb, flow=None, softmax: bool = True, want_ant=None, out=None, argmax=None, ant_out=None, ant_argmax=None):
        """counts[i] new frames (1..32, R = sum(counts) <= 256) for open slot slots[i] in one call (prego_miniroad_step_pool_ragged): rgb
        [R, d_rgb] / flow [R, d_flow] (None = zero flow) fp32 cuda contiguous, packed in `slots` order (`pack_bursts`).  Returns `push`'s
        tuple over the packed rows: (out [R, C], argmax int32 [R]) and, with want_ant, (ant_out [R, L, C], ant_argmax int32 [R, L]); every
        row's bits are `push_frames`'s.  Slot i's state is advanced by counts[i] frames and its record is word for word the record after
        counts[i] `push` calls."""
        eng, who = self.engine, "stream pool push_ragged"
        SC.refuse_general(who, eng.compute_dtype, self._hid, eng.num_layers, self._ADVICE)
        slots = self.slots.check(slots, "push_ragged")
        n = len(slots)
        counts = SC.counts_list(who, counts, n)
        R = sum(counts)
        want_ant = SC.resolve_ant(who, want_ant, getattr(eng, "ant_len", 0))
        src = SC.frame_source(who, eng.dims[0], rgb, flow, "frames")
        if src.dim() != 2 or src.shape[0] != R:
            raise PregoError(f"stream pool push_ragged: expected packed frames as [sum(counts) = {R}, d], got {tuple(src.shape)}")
        return self._step_call(who, "prego_miniroad_step_pool_ragged", eng.h, (R,), self.lib.prego_miniroad_step_pool_ragged_workspace_bytes(eng.h, n, R),
                               (self._slot_array(counts),), slots, rgb, flow, (out, argmax, ant_out, ant_argmax), 1 if softmax else 0,
                               eng.ant_len if want_ant else 0)


    def vote(self, slots, ids):
        """Aggregation alone: ids (int32 cuda [n], or a host sequence) are the new frame's step ids of `slots`, from whatever produced them."""
        slots = self.slots.check(slots, "vote")
        if not isinstance(ids, torch.Tensor):
            ids = torch.tensor([int(i) for i in ids], dtype=torch.int32).to(self.device)
        if not ids.is_cuda or ids.dtype != torch.int32 or not ids.is_contiguous() or tuple(ids.shape) != (len(slots),):
            raise PregoError(f"stream pool vote: expected ids as contiguous int32 cuda [{len(slots)}], got {tuple(ids.shape)} {ids.dtype} on {ids.device}")
        with torch.cuda.device(self.device):
            rc = self.lib.prego_stream_pool_vote(self.p, len(slots), self._slot_array(slots), C.c_void_p(ids.data_ptr()),
                                                 C.c_void_p(self._stream_ptr(self.device)))
        self._check(rc)

    def state(self, slot: int):
        """a clone of the slot's GRU state [hid]"""
        slot = self.slots.check([slot], "state")[0]
        return self._block[:self.capacity * self._hid * 4].view(torch.float32).view(self.capacity, self._hid)[slot].clone()


RING_CLS, RING_BIAS = -2, -1


def ring_source(head: int, fill: int, T: int, j: int) -> int:
    """Where token j of a slot's window comes from (csrc/vit_stream.hip, vit_ring_tokens): RING_CLS for j == T (cls + pe[T]), RING_BIAS
    for j < T - fill (a zero feature row in front of the stream encodes to the bias alone), else the ring row (head - (T - j)) mod T.
    head = frames mod T is the next row to write, fill = min(frames, T); the newest frame is token T - 1."""
    if not (0 <= j <= T and 0 <= head < T and 0 <= fill <= T):
        raise ValueError(f"ring_source: head {head}, fill {fill}, T {T}, j {j}")
    if j == T:
        return RING_CLS
    if j < T - fill:
        return RING_BIAS
    return (head - (T - j)) % T


class BurstRow(NamedTuple):
    """`burst_source`'s answer for a token that comes from the call itself: burst row k of the same slot (packed row off + k).  Not an
    int, so that it never compares equal to a ring row."""
    k: int


def burst_source(head: int, fill: int, T: int, k: int, j: int):
    """Where token j of the window of burst frame k comes from (csrc/vit_stream.hip, vit_burst_tokens), head / fill being the slot's ring
    words BEFORE the call.  d = T - 1 - j frames back from the window's newest: RING_CLS for j == T; BurstRow(k - d) where d <= k (a
    row of this call); RING_BIAS where d - k > fill (a zero feature row in front of the stream); else the ring row
    (head - (d - k)) mod T as it was before the call.  0 <= k < min(32, T)."""
    if not (0 <= j <= T and 0 <= head < T and 0 <= fill <= T and 0 <= k < min(32, T)):
        raise ValueError(f"burst_source: head {head}, fill {fill}, T {T}, k {k}, j {j}")
    if j == T:
        return RING_CLS
    d = T - 1 - j
    if d <= k:
        return BurstRow(k - d)
    if d - k > fill:
        return RING_BIAS
    return (head - (d - k)) % T


def ring_after_burst(head: int, fill: int, T: int, count: int):
    """(head, fill, rows) after a burst of `count` frames: the ring words vit_ring_commit_burst leaves and the ring rows it wrote, burst
    frame k into rows[k] - what `count` one-frame commits leave"""
    if not (0 <= head < T and 0 <= fill <= T and 1 <= count <= min(32, T)):
        raise ValueError(f"ring_after_burst: head {head}, fill {fill}, T {T}, count {count}")
    return (head + count) % T, min(fill + count, T), [(head + k) % T for k in range(count)]


class TransformerStreamPool(_RecordPool):
    """TransformerStreamPool(vit, capacity=256, vote_window=200, max_events=1024) - `ViTEnc.stream_pool(...)`: live streams through the
    `Transformer` entry.  Every slot of one device block holds a ring of the stream's last `window_size` encoded frames
    (linear_encoding runs once per frame, as in `forward_frames`) and the vote record `StreamPool` keeps; `push` gives any subset of the
    slots one new frame and returns one ViTEnc window per slot - the window ending at that frame, zero feature rows in front of the
    stream (prego_vit_step_pool; csrc/vit_stream.hip).  window_size * embedding_dim * 4 bytes per slot.  bf16 / fp16 operands.
    `push_bursts` gives every slot named a frame count of its own (1..min(32, window_size), at most 256 frames per call) and returns one
    window per frame: a backlog costs one encoding GEMM and one encoder batch, not one call per frame (prego_vit_step_pool_bursts)."""
    _C = {"destroy": "prego_vit_stream_pool_destroy", "flush": "prego_vit_stream_pool_flush", "reset": "prego_vit_stream_pool_reset",
          "record": "prego_vit_stream_pool_record", "feed_create": "prego_vit_stream_pool_feed_create",
          "image_bytes": "prego_vit_stream_pool_image_bytes", "snapshot": "prego_vit_stream_pool_snapshot",
          "restore": "prego_vit_stream_pool_restore"}

    def _image_desc(self):
        return IMAGE_VIT, self._E, self._T, self.model.compute_dtype

    def __init__(self, vit, capacity: int = 256, vote_window: int = 200, max_events: int = 1024):
        from .engine import _stream_ptr
        self.model = vit
        self._refuse_fp32("stream_pool")
        lib, dev, hnd = vit._eval_handle()
        self.lib, self.device, self._h = lib, dev, hnd
        self.vote_window, self.max_events = int(vote_window), int(max_events)      # `window` is a method here: the slot's ring
        self._vote_window = self.vote_window
        self.slots = SlotTable(capacity)
        self._stream_ptr = _stream_ptr
        self._T, self._E = int(vit.img_dim), int(vit.embedding_dim)
        self._ncls, self._ncls_pad = int(vit.out_dim), (int(vit.out_dim) + 3) // 4 * 4
        self._dims = (vit.d_rgb, vit.d_flow, self._ncls)
        need = lib.prego_vit_stream_pool_bytes(hnd, int(capacity), self.max_events)
        if need == 0:
            raise PregoError(f"transformer stream pool: capacity {capacity} (>= 1), max_events {max_events} (1..{1 << 20}), or a block "
                             "beyond size_t")
        self._block = torch.empty(need, dtype=torch.uint8, device=dev)
        self._ws = SC.Workspace()
        p = C.c_void_p()
        with torch.cuda.device(dev):
            rc = lib.prego_vit_stream_pool_create(C.byref(p), hnd, int(capacity), self.vote_window, self.max_events,
                                                  C.c_void_p(self._block.data_ptr()), need, C.c_void_p(_stream_ptr(dev)))
        self._check(rc)
        self.p = p

    def _refuse_fp32(self, who: str):
        if self.model.compute_dtype == "fp32":
            raise PregoError(f"ViTEnc {who}: compute_dtype 'fp32' is the parity mode of the window forward; the stream pool runs on bf16 / "
                             "fp16 operands (prego_vit_step_pool refuses an fp32-operand handle)")

    def _handle(self, who: str):
        """the model's inference handle with its current weights (changed weights are ingested here, as for forward_frames)"""
        self._refuse_fp32(who)
        lib, dev, hnd = self.model._eval_handle()
        if hnd is not self._h:
            raise PregoError(f"ViTEnc {who}: the model's inference handle changed since the pool was created (compute_dtype switched); "
                             "create a new pool")
        return hnd

    def push(self, slots, rgb, flow=None, out=None, argmax=None):
        """One new frame for each open slot of `slots`: rgb [n, d_rgb] / flow [n, d_flow] (None = zero flow) fp32 cuda contiguous, rows in
        `slots` order.  Returns (logits [n, C] fp32 - raw, ViTEnc applies no softmax -, argmax int32 [n]): row i is the model's forward on
        the window_size frames of slot slots[i] ending at this frame.  Each slot's ring takes the frame and its record the argmax.
        Pass buffers to reuse them."""
        hnd = self._handle("push")
        slots = self.slots.check(slots, "push")
        n = len(slots)
        SC.frame_source("transformer stream pool push", self.model.d_rgb, rgb, flow)
        return self._step_call("transformer stream pool push", "prego_vit_step_pool", hnd, (n,), self.lib.prego_vit_step_pool_workspace_bytes(hnd, n),
                               (), slots, rgb, flow if self._dims[1] else None, (out, argmax), 1 if self.model.causal else 0)

    def push_bursts(self, slots, counts, rgb, flow=None, out=None, argmax=None):
        """counts[i] new frames (1..min(32, window_size); one int = the same for every slot; R = sum(counts) <= 256) for open slot
        slots[i] in one call: rgb [R, d_rgb] / flow [R, d_flow] (None = zero flow) fp32 cuda contiguous, packed in `slots` order
        (`pack_bursts`).  Returns (logits [R, C] fp32, argmax int32 [R]): packed row off[i] + k is the model's forward on the
        window_size frames of slot slots[i] ending at its burst frame k.  Afterwards each slot's ring and record are what counts[i]
        `push` calls leave; the logits agree with those calls at the tolerance that holds `push` against `forward_frames` (the GEMM
        kernels are chosen by row count), bit for bit when every count is 1.  A longer backlog is the caller's to split."""
        who = "transformer stream pool push_bursts"
        hnd = self._handle("push_bursts")
        slots = self.slots.check(slots, "push_bursts")
        counts = SC.counts_list(who, counts, len(slots), one_int=True)
        k_max = min(32, self._T)
        for i, k in enumerate(counts):
            if not 1 <= k <= k_max:
                raise PregoError(f"transformer stream pool push_bursts: counts[{i}] = {k} (1..{k_max} frames per slot per call: at most 32, "
                                 f"window_size {self._T}; split a longer backlog)")
        R = sum(counts)
        if R > MAX_ACTIVE:
            raise PregoError(f"transformer stream pool push_bursts: the counts sum to {R} rows (at most {MAX_ACTIVE} windows per call)")
        SC.frame_source(who, self.model.d_rgb, rgb, flow, "frames")
        return self._step_call(who, "prego_vit_step_pool_bursts", hnd, (R,), self.lib.prego_vit_step_pool_bursts_workspace_bytes(hnd, len(slots), R),
                               (self._slot_array(counts),), slots, rgb, flow if self._dims[1] else None, (out, argmax),
                               1 if self.model.causal else 0, note=f" (sum(counts) = {R} packed rows)")


    def window(self, slot: int):
        """([window_size, E] fp32 tensor, fill): the slot's encoded frames, oldest first - linear_encoding's rows, its bias where the
        stream has no frame yet - and how many of them are frames.  For inspection; it waits for the stream."""
        slot = self.slots.check([slot], "window")[0]
        self._handle("window")
        rows = torch.empty((self._T, self._E), dtype=torch.float32, device=self.device)
        fill = torch.empty((1,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            self._check(self.lib.prego_vit_stream_pool_window(self.p, slot, C.c_void_p(rows.data_ptr()), C.c_void_p(fill.data_ptr()),
                                                              C.c_void_p(self._stream_ptr(self.device))))
        return rows, int(fill.item())


class DecodePool(_RecordPool):
    """DecodePool(n_classes, trans, init=None, lag=64, capacity=256, vote_window=1, max_events=1024, device="cuda"): online fixed-lag
    Viterbi per live stream (prego_decode_pool_*, csrc/decode_pool.hip; definitions: prego_amd/decode.py).  Every slot of one device block
    holds a stream's Viterbi state; `push` gives any subset of the slots 1..32 rows of scores each - what `StreamPool.push` /
    `push_frames` / `push_ragged` return with softmax=True - and every frame's label is committed `lag` frames after it arrived, into a
    record of the stream pools' layout: `events`, `close`, `event_feed`, `mistake_monitor` and `forecast_monitor` work on the decoded
    transcript.  With vote_window 1 every change of the committed label is an event.  `decode.OnlineDecoder` is the host model of a
    slot.  Consecutive labels come from different back-pointer chains, so the committed sequence need not be an allowed path."""
    _C = {"destroy": "prego_decode_pool_destroy", "flush": "prego_decode_pool_flush", "reset": "prego_decode_pool_reset",
          "record": "prego_decode_pool_record", "feed_create": "prego_decode_pool_feed_create"}

    def __init__(self, n_classes: int, trans, init=None, lag: int = 64, capacity: int = 256, vote_window: int = 1, max_events: int = 1024,
                 device="cuda"):
        import numpy as np

        from . import _lib
        from .engine import _stream_ptr
        self.lib, self._stream_ptr = _lib.load(), _stream_ptr
        dev = torch.device(device)
        self.device = torch.device("cuda", torch.cuda.current_device()) if dev.type == "cuda" and dev.index is None else dev
        if self.device.type != "cuda":
            raise PregoError("decode pool needs a CUDA device; there is no CPU fallback (host model: prego_amd.decode.OnlineDecoder)")
        self.lag, self.vote_window, self.max_events = int(lag), int(vote_window), int(max_events)
        self._vote_window, self._ncls, self._ncls_pad = self.vote_window, int(n_classes), (int(n_classes) + 3) // 4 * 4
        self.slots = SlotTable(capacity)
        need = self.lib.prego_decode_pool_bytes(int(capacity), self._ncls, self.lag, self.max_events)
        if need == 0:
            raise PregoError(f"decode pool: capacity {capacity}, max_events {max_events} (each 1..{1 << 20}), n_classes {n_classes} (1..128), "
                             f"lag {lag} (0..256)")
        as_dev = lambda a, n: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))).to(
            device=self.device, dtype=torch.int32).reshape(n).contiguous()
        tr = as_dev(trans, self._ncls * self._ncls)
        ini = None if init is None else as_dev(init, self._ncls)
        self._block = torch.empty(need, dtype=torch.uint8, device=self.device)
        self.p = None
        p = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.prego_decode_pool_create(C.byref(p), int(capacity), self._ncls, self.lag, self.vote_window, self.max_events,
                                                   C.c_void_p(tr.data_ptr()), C.c_void_p(ini.data_ptr()) if ini is not None else None,
                                                   C.c_void_p(self._block.data_ptr()), need, C.c_void_p(_stream_ptr(self.device)))
        self._check(rc)                                          # trans / init go back to the allocator behind the clamp, on its stream
        self.p = p

    def open(self, slot=None) -> int:
        """the lowest free slot, or exactly `slot`: a decoder beside a `StreamPool` mirrors its numbering.  Nothing is launched"""
        return self.slots.open(slot)

    def _out(self, buf, shape, name):
        if buf is None:
            return torch.empty(shape, dtype=torch.int32, device=self.device)
        if not buf.is_cuda or buf.dtype != torch.int32 or not buf.is_contiguous() or tuple(buf.shape) != tuple(shape):
            raise PregoError(f"decode pool: expected {name} as contiguous int32 cuda {tuple(shape)}, got {tuple(buf.shape)} {buf.dtype}")
        return buf

    def push(self, slots, scores, counts=None, costs: bool = False, labels=None, commit=None, now=None):
        """Rows of scores for the open slots named: [n, C] (one frame each), [n, K, C] (K <= 32 each) or packed [R, C] with
        counts[i] rows (1..32, R <= 256) for slots[i] - fp32 probabilities, or int32 emission costs with costs=True; cuda, rows
        contiguous.  Returns (labels int32 [R], commit int32 [n, 2], now int32 [R]) on the device: in slot i's row block the labels this
        call committed, in frame order, then DECODE_PENDING; (first frame committed or next due, how many); e_t of every row, the
        zero-lag provisional label (-1 once the stream is dead).  Nothing waits.  Pass buffers to reuse them."""
        who = "decode pool push"
        slots = self.slots.check(slots, "push")
        n, Cn = len(slots), self._ncls
        if not (isinstance(scores, torch.Tensor) and scores.is_cuda) or scores.dtype != (torch.int32 if costs else torch.float32):
            raise PregoError(f"{who}: expected scores as a {'int32' if costs else 'float32'} cuda tensor (costs={costs}); there is no CPU fallback")
        if scores.dim() == 3 and counts is None:
            if scores.shape[0] != n or scores.shape[2] != Cn:
                raise PregoError(f"{who}: expected scores as [{n}, K, {Cn}], got {tuple(scores.shape)}")
            counts = [int(scores.shape[1])] * n
            scores = scores.reshape(n * scores.shape[1], Cn)
        elif scores.dim() == 2 and counts is None:
            counts = [1] * n
        else:
            counts = SC.counts_list(who, counts, n)
        R = sum(counts)
        if scores.dim() != 2 or tuple(scores.shape) != (R, Cn) or (scores.stride(1) != 1 and R > 0):
            raise PregoError(f"{who}: expected scores as [{R}, {Cn}] rows (sum(counts) = {R}) with contiguous rows, got {tuple(scores.shape)}")
        ld = int(scores.stride(0)) if R > 1 else Cn
        labels, commit, now = self._out(labels, (max(R, 0),), "labels"), self._out(commit, (n, 2), "commit"), self._out(now, (max(R, 0),), "now")
        entry = self.lib.prego_decode_pool_push_costs if costs else self.lib.prego_decode_pool_push
        with torch.cuda.device(self.device):
            self._check(entry(self.p, n, self._slot_array(slots), self._slot_array(counts), C.c_void_p(scores.data_ptr()), ld,
                              C.c_void_p(labels.data_ptr()), C.c_void_p(commit.data_ptr()), C.c_void_p(now.data_ptr()),
                              C.c_void_p(self._stream_ptr(self.device))))
        return labels, commit, now

    def flush(self, slots, labels=None, commit=None):
        """Ends the streams named without freeing them: the tail is committed from the last frame's chain, the record's unfinished window
        voted, the slot marked flushed (a later push ingests nothing; `close` reopens it).  Returns (labels int32 [n, lag]: slot i's tail
        then DECODE_PENDING, commit int32 [n, 2]) on the device; nothing waits."""
        slots = self.slots.check(slots, "flush")
        n = len(slots)
        labels, commit = self._out(labels, (n, self.lag), "labels"), self._out(commit, (n, 2), "commit")
        with torch.cuda.device(self.device):
            self._check(self.lib.prego_decode_pool_flush(self.p, n, self._slot_array(slots), C.c_void_p(labels.data_ptr()) if self.lag else None,
                                                         C.c_void_p(commit.data_ptr()), C.c_void_p(self._stream_ptr(self.device))))
        return labels, commit

    def _state_view(self, slot: int):
        ptr, nbytes = C.c_void_p(), C.c_size_t()
        self._check(self.lib.prego_decode_pool_state(self.p, slot, C.byref(ptr), C.byref(nbytes)))
        off = ptr.value - self._block.data_ptr()
        return self._block[off:off + nbytes.value].view(torch.int32)

    def state_words(self, slot: int):
        """the slot's header and keys as int32 numpy words (prego_decode_pool_state; `OnlineDecoder.state_words`): one D2H copy, it waits"""
        slot = self.slots.check([slot], "state_words")[0]
        return self._state_view(slot).cpu().numpy()

    def headers(self):
        """int32 [capacity, 8] on the device: a copy of every slot's header; nothing waits"""
        a = self._state_view(0)
        base = a.data_ptr() - self._block.data_ptr()
        stride = (self._state_view(1).data_ptr() - a.data_ptr()) if self.capacity > 1 else a.numel() * 4
        return torch.as_strided(self._block[base:].view(torch.int32), (self.capacity, 8), (stride // 4, 1)).clone()

    def status(self, slot: int) -> dict:
        """the slot's header: {'frames', 'committed', 'dead', 'flushed', 'pushed_after_flush', 'end', 'cost'} ('end' -1 for an empty or
        a dead stream, 'cost' -1 for a dead one).  One small D2H copy; it waits."""
        w = self.state_words(slot)
        frames, st = int(w[0]), int(w[2])
        return {"frames": frames, "committed": int(w[1]), "dead": bool(st & 1), "flushed": bool(st & 2), "pushed_after_flush": bool(st & 4),
                "end": int(w[3]) if frames else -1, "cost": int(w[4:6].view("int64")[0])}

    def _raise_overflow(self, slot: int, overflow: int):
        if overflow & OVERFLOW_BAD_ID:
            raise PregoError(f"decode pool: the stream of slot {slot} is infeasible: at some frame no state had a finite cost under the model "
                             "(forbidden transitions or starts); the labels committed from then on are -1")
        super()._raise_overflow(slot, overflow)

    def close(self, slot: int) -> dict:
        """Ends the stream: commits its tail, votes the record's unfinished window, reads header and record (small D2H copies), zeroes the
        slot and frees it.  Returns {'pred', 'changes_pred'} of the committed labels as the other pools give them for their ids, plus
        'labels_tail' (the labels the flush committed) and 'cost' (the decoded path's total).  Raises PregoError, the slot freed all
        the same, for a dead (infeasible) stream or a record that overflowed."""
        slot = self.slots.check([slot], "close")[0]
        arr, s = self._slot_array([slot]), C.c_void_p(self._stream_ptr(self.device))
        with torch.cuda.device(self.device):
            tail, commit = self.flush([slot])
            w = self._state_view(slot).cpu().numpy()
            frames, overflow, ev_id, ev_start = self._record(slot)
            m = int(commit[0, 1])
            self._check(self.lib.prego_decode_pool_reset(self.p, 1, arr, s))
            for feed in self._feeds:
                feed.forget([slot])
        self.slots.release(slot)
        if int(w[2]) & 1:
            self._raise_overflow(slot, OVERFLOW_BAD_ID)
        self._raise_overflow(slot, overflow)
        return {"pred": ev_id, "changes_pred": ev_start[1:] + [frames], "labels_tail": tail[0, :m].cpu().tolist(), "cost": int(w[4:6].view("int64")[0])}

    def _no_images(self, *a, **k):
        raise PregoError("decode pool: slot images of decode pools are not supported yet (snapshot / restore / detach)")

    snapshot = restore = detach = _no_images
