"""Procedure model: a symbolic step anticipator that says "this step should not have come here" - the deterministic stand-in for the
LLM branch of step_anticipation.  A corpus of correct-procedure transcripts, grouped (the toy class), is counted as
a back-off n-gram model over step ids with a virtual START in front of every sequence; a step is a MISTAKE when, after the longest
context the corpus knows (at most `order` symbols, START included), it was seen too rarely: cnt * den < tot * num, or never.  With order
1 and threshold 1 / N this is the rule of step_anticipation/src/data/frequentist_baseline.py; a context the corpus never saw gives
UNKNOWN, which is not a mistake (its lines 43-48, 58-59).  Integers only: the device (csrc/procedure.hip) and `ProcedureModel.judge`
agree on every verdict word.

`ProcedureModel` is the host model and the oracle of the kernel; `.to(device)` gives a `DeviceProcedureModel`, whose
`judge_sequences` is the offline / evaluation entry (prego_procedure_judge) and which `pool.mistake_monitor(model)` judges a stream
pool's event feed with (prego_stream_pool_feed_judge; prego_amd/stream_pool.py).

The same histogram answers "what should come next" (DESIGN section 13m): `ProcedureModel.forecast(history, group)` gives a `Forecast`,
the first 8 steps seen after the longest known context by count, `forecast_sequences` / `anticipation_metrics` score it offline
(prego_procedure_forecast on the device) and `pool.forecast_monitor(model)` reports it beside every verdict."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

JUDGED, MISTAKE, UNKNOWN, SKIPPED = 1, 2, 4, 8          # bits of a verdict's flags word; j* in bits 8..15 (csrc/kernels.h: kProc*)
JSTAR_SHIFT = 8
MAX_ORDER, MAX_CLASSES, MAX_DEN = 8, 128, 32768
MAX_GROUPS, MAX_EXAMPLES, MAX_SYMBOLS = 1 << 20, 1 << 24, 1 << 30      # csrc/procedure.cpp: kProcMax*
VERDICT_WORDS = 8
START = -1                                               # the reference's prompts write the virtual first symbol as -1
NO_MATCH = -2                                            # what a queried symbol outside the classes is compared as


class Verdict(NamedTuple):
    """One judged step: flags (JUDGED | MISTAKE | UNKNOWN | SKIPPED, j* in bits 8..15), cnt = cnt(cur) and tot at j*, the group the
    query used (-1: every group) and the 128-bit mask of the allowed classes."""
    flags: int
    cnt: int
    tot: int
    group: int
    mask: int

    @property
    def mistake(self) -> bool:
        return bool(self.flags & MISTAKE)

    @property
    def unknown(self) -> bool:
        return bool(self.flags & UNKNOWN)

    @property
    def skipped(self) -> bool:
        return bool(self.flags & SKIPPED)

    @property
    def jstar(self) -> int:
        return (self.flags >> JSTAR_SHIFT) & 0xFF

    @property
    def allowed(self) -> list:
        return [c for c in range(MAX_CLASSES) if self.mask >> c & 1]

    def words(self) -> list:
        """the 8 int32 words the device writes: flags | cnt(cur) | tot | group | mask bits 0..31 | 32..63 | 64..95 | 96..127"""
        m = [(self.mask >> (32 * k)) & 0xFFFFFFFF for k in range(4)]
        return [self.flags, self.cnt, self.tot, self.group] + [w - (1 << 32) if w >> 31 else w for w in m]

    @classmethod
    def from_words(cls, w) -> "Verdict":
        w = [int(v) for v in w]
        return cls(w[0], w[1], w[2], w[3], sum((w[4 + k] & 0xFFFFFFFF) << (32 * k) for k in range(4)))


SKIPPED_VERDICT = Verdict(SKIPPED, 0, 0, -1, 0)          # an overflow entry of a feed, or an event the record no longer holds

MADE = JUDGED                                            # a forecast's flags word: MADE | UNKNOWN | SKIPPED, j* as a verdict's,
RANKED_SHIFT, RANKS, FORECAST_WORDS = 16, 8, 24          # the ranked entries (0..8) in bits 16..19 (csrc/kernels.h: kProcRank*)


class Forecast(NamedTuple):
    """What may come next after a history: flags (MADE | UNKNOWN | SKIPPED, j* in bits 8..15, ranked entries in
    bits 16..19), n_cand = the classes seen after the longest known context, tot = their examples, the group the query used, the
    128-bit mask of the allowed classes (a verdict's rule) and the first 8 candidates by count descending, equal counts by ascending
    id: `ids` and `cnts`, unused ranks -1 and 0."""
    flags: int
    n_cand: int
    tot: int
    group: int
    mask: int
    ids: tuple
    cnts: tuple

    @property
    def made(self) -> bool:
        return bool(self.flags & MADE)

    @property
    def unknown(self) -> bool:
        return bool(self.flags & UNKNOWN)

    @property
    def skipped(self) -> bool:
        return bool(self.flags & SKIPPED)

    @property
    def jstar(self) -> int:
        return (self.flags >> JSTAR_SHIFT) & 0xFF

    @property
    def n_ranked(self) -> int:
        return (self.flags >> RANKED_SHIFT) & 0xF

    def ranked(self) -> list:
        """[(id, cnt)] of the ranked entries, the likeliest first"""
        return list(zip(self.ids[:self.n_ranked], self.cnts[:self.n_ranked]))

    def allowed(self) -> list:
        return [c for c in range(MAX_CLASSES) if self.mask >> c & 1]

    def words(self) -> list:
        """the 24 int32 words the device writes: flags | n_cand | tot | group | mask [4] | id [8] | cnt [8]"""
        m = [(self.mask >> (32 * k)) & 0xFFFFFFFF for k in range(4)]
        return [self.flags, self.n_cand, self.tot, self.group] + [w - (1 << 32) if w >> 31 else w for w in m] + list(self.ids) + list(self.cnts)

    @classmethod
    def from_words(cls, w) -> "Forecast":
        w = [int(v) for v in w]
        return cls(w[0], w[1], w[2], w[3], sum((w[4 + k] & 0xFFFFFFFF) << (32 * k) for k in range(4)), tuple(w[8:16]), tuple(w[16:24]))


SKIPPED_FORECAST = Forecast(SKIPPED, 0, 0, -1, 0, (-1,) * RANKS, (0,) * RANKS)     # where a verdict would be SKIPPED_VERDICT; a slot outside the pool


class ProcedureModel:
    """ProcedureModel(n_classes, order=2, threshold=(0, 1), targets='all' | 'last').  `add(sequence, group)` takes one correct
    transcript (step ids in [0, n_classes), group >= 0); with targets='all' every position of it is an example (context: START and
    the steps before it, next symbol: the step), with 'last' only its last position - the reference's prompt blocks, each a context
    and ONE next symbol.  `judge(history, cur, group)` is the definition the device implements (group -1: every group)."""

    def __init__(self, n_classes: int, order: int = 2, threshold=(0, 1), targets: str = "all"):
        num, den = (int(v) for v in threshold)
        if not 1 <= int(n_classes) <= MAX_CLASSES:
            raise ValueError(f"ProcedureModel: n_classes {n_classes} (1..{MAX_CLASSES})")
        if not 1 <= int(order) <= MAX_ORDER:
            raise ValueError(f"ProcedureModel: order {order} (1..{MAX_ORDER})")
        if not 0 <= num <= den <= MAX_DEN or den < 1:
            raise ValueError(f"ProcedureModel: threshold {num}/{den} (0 <= num <= den, 1 <= den <= {MAX_DEN})")
        if targets not in ("all", "last"):
            raise ValueError(f"ProcedureModel: targets {targets!r} ('all' or 'last')")
        self.n_classes, self.order, self.num, self.den, self.targets = int(n_classes), int(order), num, den, targets
        self.transcripts = []                                 # (group, [symbols], [target flags])
        self._index = None

    # -- the corpus ------------------------------------------------------------------------------
    def add(self, sequence, group: int = 0, targets=None):
        """one transcript; `targets` (a flag per position) overrides the model's 'all' / 'last'"""
        seq, group = [int(s) for s in sequence], int(group)
        if group < 0:
            raise ValueError(f"ProcedureModel.add: group {group} (>= 0; -1 is the query for every group)")
        for s in seq:
            if not 0 <= s < self.n_classes:
                raise ValueError(f"ProcedureModel.add: step id {s} outside [0, {self.n_classes})")
        if targets is None:
            flags = [1] * len(seq) if self.targets == "all" else [0] * (len(seq) - 1) + [1] * min(len(seq), 1)
        else:
            flags = [1 if t else 0 for t in targets]
            if len(flags) != len(seq):
                raise ValueError(f"ProcedureModel.add: {len(flags)} target flags for {len(seq)} symbols")
        self.transcripts.append((group, seq, flags))
        self._index = None
        return self

    @classmethod
    def from_transcripts(cls, transcripts, n_classes: int, **kw) -> "ProcedureModel":
        """transcripts: (sequence, group) pairs"""
        m = cls(n_classes, **kw)
        for seq, group in transcripts:
            m.add(seq, group)
        return m

    @staticmethod
    def parse_context_prompt(text: str) -> list:
        """The transcripts of one prompt of step_anticipation/data/context_prompt/*_context_prompt_train.json: blocks split on '---',
        each 'Input Sequence:\\n -1, a, b\\nNext Symbol:\\n c' (a 'Sequence type:' line in front is ignored); the transcript is the
        context without its leading -1, followed by the next symbol."""
        out = []
        for block in text.split("---"):
            lines = [ln.strip() for ln in block.strip().splitlines()]
            if not any(lines):
                continue
            try:
                ctx = [int(v) for v in lines[lines.index("Input Sequence:") + 1].split(",")]
                nxt = int(lines[lines.index("Next Symbol:") + 1])
            except (ValueError, IndexError):
                raise ValueError(f"ProcedureModel.parse_context_prompt: not a prompt block: {block.strip()!r}") from None
            if not ctx or ctx[0] != START or START in ctx[1:]:
                raise ValueError(f"ProcedureModel.parse_context_prompt: a context must start with {START} and hold it once: {ctx}")
            out.append(ctx[1:] + [nxt])
        return out

    def from_context_prompt(self, text: str, group: int = 0) -> "ProcedureModel":
        """adds every transcript of the prompt `text` to `group`"""
        for seq in self.parse_context_prompt(text):
            self.add(seq, group)
        return self

    @property
    def n_groups(self) -> int:
        return 1 + max((g for g, _, _ in self.transcripts), default=-1)

    @property
    def n_symbols(self) -> int:
        """symbols of the corpus, START excluded"""
        return sum(len(s) for _, s, _ in self.transcripts)

    @property
    def n_examples(self) -> int:
        return sum(sum(f) for _, _, f in self.transcripts)

    # -- judging -----------------------------------------------------------------------------------
    def _examples(self):
        """group -> {context suffix of 1..order symbols (START = -1 included): [count per next symbol]}, None: every group"""
        if self._index is None:
            idx = {}
            for group, seq, flags in self.transcripts:
                ctx = [START] + seq
                for p, t in enumerate(flags):
                    if not t:
                        continue
                    for j in range(1, min(self.order, p + 1) + 1):
                        key = tuple(ctx[p + 1 - j:p + 1])
                        for g in (group, None):
                            row = idx.setdefault(g, {}).setdefault(key, [0] * self.n_classes)
                            row[seq[p]] += 1
            self._index = idx
        return self._index

    def judge(self, history, cur: int, group: int = -1) -> Verdict:
        """history: the steps before `cur` (START is implied).  A symbol outside [0, n_classes) matches nothing."""
        group, cur = int(group), int(cur)
        ctx = [START] + [int(s) if 0 <= int(s) < self.n_classes else NO_MATCH for s in history]
        rows = self._examples().get(None if group == -1 else group, {})
        for j in range(min(self.order, len(ctx)), 0, -1):
            row = rows.get(tuple(ctx[len(ctx) - j:]))
            if row is None:
                continue
            tot = sum(row)
            mask = sum(1 << c for c, n in enumerate(row) if n > 0 and n * self.den >= tot * self.num)
            cnt = row[cur] if 0 <= cur < self.n_classes else 0
            ok = 0 <= cur < self.n_classes and mask >> cur & 1
            return Verdict(JUDGED | (0 if ok else MISTAKE) | j << JSTAR_SHIFT, cnt, tot, group, mask)
        return Verdict(JUDGED | UNKNOWN, 0, 0, group, 0)

    def judge_sequences(self, sequences, groups=None) -> list:
        """one list of Verdicts per sequence, a Verdict per position (the history: the sequence's steps in front of it)"""
        sequences = [list(s) for s in sequences]
        groups = [-1] * len(sequences) if groups is None else [int(g) for g in groups]
        if len(groups) != len(sequences):
            raise ValueError(f"ProcedureModel.judge_sequences: {len(sequences)} sequences, {len(groups)} groups")
        return [[self.judge(s[:i], s[i], g) for i in range(len(s))] for s, g in zip(sequences, groups)]

    def mistake_metrics(self, sequences, groups=None, judged=None) -> dict:
        """tp / fp / fn / tn, precision, recall and F1 by the counting rule of step_anticipation's get_metrics (llama_meta.py:14-58):
        the last step of every sequence is the mistake, every step before it is correct; UNKNOWN counts as "seen as correct".
        `judged`: verdicts from elsewhere (the device's), as `judge_sequences` shapes them."""
        judged = self.judge_sequences(sequences, groups) if judged is None else judged
        tp = fp = fn = tn = unknown = 0
        for vs in judged:
            if not vs:
                continue
            unknown += sum(v.unknown for v in vs)
            fp += sum(v.mistake for v in vs[:-1])
            tn += sum(not v.mistake for v in vs[:-1])
            tp += int(vs[-1].mistake)
            fn += int(not vs[-1].mistake)
        precision = tp / (tp + fp) if tp + fp else 0.0
        recall = tp / (tp + fn) if tp + fn else 0.0
        f1 = 2 * precision * recall / (precision + recall) if precision + recall else 0.0
        return {"tp": tp, "fp": fp, "fn": fn, "tn": tn, "unknown": unknown, "precision": precision, "recall": recall, "f1": f1}

    # -- forecasting ---------------------------------------------------------------------------------
    def forecast(self, history, group: int = -1) -> Forecast:
        """history: every step so far, all of it context (START is implied); what the corpus saw next after the longest context it
        knows.  The definition the device implements (group -1: every group); a symbol outside [0, n_classes) matches nothing."""
        group = int(group)
        ctx = [START] + [int(s) if 0 <= int(s) < self.n_classes else NO_MATCH for s in history]
        rows = self._examples().get(None if group == -1 else group, {})
        for j in range(min(self.order, len(ctx)), 0, -1):
            row = rows.get(tuple(ctx[len(ctx) - j:]))
            if row is None:
                continue
            tot = sum(row)
            mask = sum(1 << c for c, n in enumerate(row) if n > 0 and n * self.den >= tot * self.num)
            cand = sorted((c for c, n in enumerate(row) if n > 0), key=lambda c: (-row[c], c))
            top = cand[:RANKS]
            pad = RANKS - len(top)
            return Forecast(MADE | j << JSTAR_SHIFT | len(top) << RANKED_SHIFT, len(cand), tot, group, mask,
                            tuple(top) + (-1,) * pad, tuple(row[c] for c in top) + (0,) * pad)
        return Forecast(MADE | UNKNOWN, 0, 0, group, 0, (-1,) * RANKS, (0,) * RANKS)

    def forecast_sequences(self, sequences, groups=None) -> list:
        """one list per sequence of len + 1 Forecasts: after its first p = 0 .. len steps.  Entry p forecasts step p, the last one
        what would follow the sequence."""
        sequences = [list(s) for s in sequences]
        groups = [-1] * len(sequences) if groups is None else [int(g) for g in groups]
        if len(groups) != len(sequences):
            raise ValueError(f"ProcedureModel.forecast_sequences: {len(sequences)} sequences, {len(groups)} groups")
        return [[self.forecast(s[:p], g) for p in range(len(s) + 1)] for s, g in zip(sequences, groups)]

    def anticipation_metrics(self, sequences, groups=None, ks=(1, 3, 5), forecasts=None) -> dict:
        """How often the true next step is among the model's first k: over every position p of every sequence, 'positions', 'unknown'
        (an UNKNOWN forecast is a miss for every k and counted on its own) and 'top' = {k: the positions whose step is among the first
        k ranked ids}, k <= 8.  `forecasts`: from elsewhere (the device's), as `forecast_sequences` shapes them."""
        ks = tuple(int(k) for k in ks)
        if any(not 1 <= k <= RANKS for k in ks):
            raise ValueError(f"ProcedureModel.anticipation_metrics: ks {ks} (each 1..{RANKS}: a forecast holds {RANKS} ranks)")
        sequences = [list(s) for s in sequences]
        forecasts = self.forecast_sequences(sequences, groups) if forecasts is None else forecasts
        positions = unknown = 0
        top = {k: 0 for k in ks}
        for s, fs in zip(sequences, forecasts):
            for p, step in enumerate(s):
                positions += 1
                unknown += int(fs[p].unknown)
                ids = [c for c, _ in fs[p].ranked()]
                for k in ks:
                    top[k] += int(int(step) in ids[:k])
        return {"positions": positions, "unknown": unknown, "top": top}

    # -- a decoding grammar ----------------------------------------------------------------------------
    def transition_costs(self, group: int = -1, switch_cost: int = 2048, unseen: int = -1, stay_cost: int = 0):
        """(trans int32 [C, C], init int32 [C]) for prego_amd.decode (`viterbi_decode`, `viterbi_decode_device`) from the corpus's
        order-1 counts of `group` (-1: every group).  trans[i][i] = stay_cost; trans[i][j] = switch_cost where step j followed step i
        somewhere in the group, `unseen` otherwise (default DECODE_FORBIDDEN = -1: such a switch cannot be decoded at all); init[j] = 0
        where a transcript of the group starts with j, `unseen` otherwise.  Costs are in 1/256 bit; 2048 = 8 bits per switch, not tuned.
        Host only.  A grammar of CORRECT procedures with unseen = FORBIDDEN decodes mistakes away: whatever the recogniser saw is bent
        into an order the corpus knows.  That is what transcript scoring (Edit / F1 against a correct ground truth) wants and the
        opposite of what the mistake monitor needs - feed the monitor from a decode with a finite `unseen`, or from none."""
        import numpy as np
        C_ = self.n_classes
        rows = self._examples().get(None if int(group) == -1 else int(group), {})
        trans = np.full((C_, C_), int(unseen), np.int32)
        init = np.full(C_, int(unseen), np.int32)
        for i in range(C_):
            for j, n in enumerate(rows.get((i,), ())):
                if n > 0:
                    trans[i, j] = int(switch_cost)
        for j, n in enumerate(rows.get((START,), ())):
            if n > 0:
                init[j] = 0
        np.fill_diagonal(trans, int(stay_cost))
        return trans, init

    # -- the device ----------------------------------------------------------------------------------
    def flat(self):
        """(groups, offsets, symbols, target flags) of the corpus as prego_procedure_model_create takes them"""
        groups, offsets, symbols, flags = [], [0], [], []
        for g, seq, fl in self.transcripts:
            groups.append(g)
            symbols += seq
            flags += fl
            offsets.append(len(symbols))
        return groups, offsets, symbols, flags

    def to(self, device, lib=None) -> "DeviceProcedureModel":
        """lib: the loaded library to run on (default: the product library; a pool on the debug library passes its own)"""
        return DeviceProcedureModel(self, device, lib)


class DeviceProcedureModel:
    """The corpus of a `ProcedureModel` in one device block (csrc/procedure.cpp lays it out, sorted by group): `.m` is the handle the
    judging entries take, `.host` the model it was made from.  The corpus as it was at `.to(device)`: later `add`s do not reach it."""

    def __init__(self, host: ProcedureModel, device, lib=None):
        import torch

        from . import _lib
        from .engine import _stream_ptr
        self.host, self.lib, self.device = host, lib if lib is not None else _lib.load(), torch.device(device)
        self._stream_ptr = _stream_ptr
        groups, offsets, symbols, flags = host.flat()
        n_t = len(groups)
        need = self.lib.prego_procedure_model_bytes(host.n_groups, n_t, len(symbols), sum(flags))
        if need == 0:
            raise _lib.PregoError(f"procedure model: {host.n_groups} groups (1..{MAX_GROUPS}), {len(symbols)} symbols (with a START per "
                                  f"transcript at most {MAX_SYMBOLS}), {sum(flags)} examples (at most {MAX_EXAMPLES})")
        self._block = torch.empty(need, dtype=torch.uint8, device=self.device)
        self.m = None
        m = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.prego_procedure_model_create(
                C.byref(m), host.n_classes, host.order, host.num, host.den, n_t, (C.c_int32 * max(n_t, 1))(*groups),
                (C.c_int64 * (n_t + 1))(*offsets), (C.c_int32 * max(len(symbols), 1))(*symbols), (C.c_uint8 * max(len(flags), 1))(*flags),
                C.c_void_p(self._block.data_ptr()), need, C.c_void_p(_stream_ptr(self.device)))
        if rc != 0:
            raise _lib.PregoError(f"prego_amd error {rc}: {self.lib.prego_last_error().decode()}")
        self.m = m

    def __del__(self):
        try:
            if getattr(self, "m", None):
                self.lib.prego_procedure_model_destroy(self.m)
                self.m = None
        except Exception:
            pass

    def judge_words(self, sequences, groups=None):
        """int32 cuda [n_positions, 8]: the verdict words of every position of every sequence, in order; nothing waits"""
        import torch

        from ._lib import PregoError
        sequences = [[int(v) for v in s] for s in sequences]
        groups = [-1] * len(sequences) if groups is None else [int(g) for g in groups]
        if len(groups) != len(sequences):
            raise PregoError(f"procedure judge: {len(sequences)} sequences, {len(groups)} groups")
        offsets = [0]
        for s in sequences:
            offsets.append(offsets[-1] + len(s))
        n_pos = offsets[-1]
        out = torch.empty((n_pos, VERDICT_WORDS), dtype=torch.int32, device=self.device)
        if n_pos == 0:
            return out
        dev = lambda v: torch.tensor(v, dtype=torch.int32).to(self.device)
        off_d, sym_d, grp_d = dev(offsets), dev([v for s in sequences for v in s]), dev(groups)
        with torch.cuda.device(self.device):
            rc = self.lib.prego_procedure_judge(self.m, len(sequences), n_pos, C.c_void_p(off_d.data_ptr()), C.c_void_p(sym_d.data_ptr()),
                                                C.c_void_p(grp_d.data_ptr()), C.c_void_p(out.data_ptr()), out.numel() * 4,
                                                C.c_void_p(self._stream_ptr(self.device)))
        if rc != 0:
            raise PregoError(f"prego_amd error {rc}: {self.lib.prego_last_error().decode()}")
        return out

    def forecast_words(self, sequences, groups=None):
        """int32 cuda [n_positions + n_sequences, 24]: the forecast words after the first p = 0 .. len steps of every sequence, in
        order (prego_procedure_forecast); nothing waits"""
        import torch

        from ._lib import PregoError
        sequences = [[int(v) for v in s] for s in sequences]
        groups = [-1] * len(sequences) if groups is None else [int(g) for g in groups]
        if len(groups) != len(sequences):
            raise PregoError(f"procedure forecast: {len(sequences)} sequences, {len(groups)} groups")
        offsets = [0]
        for s in sequences:
            offsets.append(offsets[-1] + len(s))
        n_pos = offsets[-1]
        out = torch.empty((n_pos + len(sequences), FORECAST_WORDS), dtype=torch.int32, device=self.device)
        if not sequences:
            return out
        dev = lambda v: torch.tensor(v, dtype=torch.int32).to(self.device)
        off_d, sym_d, grp_d = dev(offsets), dev([v for s in sequences for v in s] or [0]), dev(groups)
        with torch.cuda.device(self.device):
            rc = self.lib.prego_procedure_forecast(self.m, len(sequences), n_pos, C.c_void_p(off_d.data_ptr()), C.c_void_p(sym_d.data_ptr()),
                                                   C.c_void_p(grp_d.data_ptr()), C.c_void_p(out.data_ptr()), out.numel() * 4,
                                                   C.c_void_p(self._stream_ptr(self.device)))
        if rc != 0:
            raise PregoError(f"prego_amd error {rc}: {self.lib.prego_last_error().decode()}")
        return out

    def forecast_sequences(self, sequences, groups=None) -> list:
        """`ProcedureModel.forecast_sequences` on the device: one list of len + 1 Forecasts per sequence.  One D2H copy; it waits."""
        sequences = [list(s) for s in sequences]
        rows = self.forecast_words(sequences, groups).cpu().tolist()
        out, at = [], 0
        for s in sequences:
            out.append([Forecast.from_words(w) for w in rows[at:at + len(s) + 1]])
            at += len(s) + 1
        return out

    def judge_sequences(self, sequences, groups=None) -> list:
        """`ProcedureModel.judge_sequences` on the device: one list of Verdicts per sequence.  One D2H copy; it waits."""
        sequences = [list(s) for s in sequences]
        rows = self.judge_words(sequences, groups).cpu().tolist()
        out, at = [], 0
        for s in sequences:
            out.append([Verdict.from_words(w) for w in rows[at:at + len(s)]])
            at += len(s)
        return out
