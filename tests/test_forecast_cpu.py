"""The next-step forecast of the procedure model on the host (prego_amd/procedure.py: ProcedureModel.forecast, Forecast,
anticipation_metrics; prego_amd/stream_pool.py: MonitorModel.forecast_entry / forecast_slots).  The oracle of the
device kernels is held here against a restatement of the definitions written in this file: a dict from context tuples to Counters,
back-off by shortening the tuple.  Everything is integers and exact."""
import json
import os
import random
from collections import Counter

import pytest

from prego_amd.aggregate import OVERFLOW_BAD_ID, OnlineRecord
from prego_amd.procedure import (FORECAST_WORDS, JUDGED, MADE, SKIPPED, SKIPPED_FORECAST, SKIPPED_VERDICT, UNKNOWN, Forecast,
                                 ProcedureModel)
from prego_amd.stream_pool import MonitorModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
START_, NOTHING = "START", "NOTHING"


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------------
def brute_table(transcripts, order, group):
    """{context tuple of 1..order symbols: Counter of next symbols} over the transcripts (group, symbols, target flags) of `group`"""
    table = {}
    for g, seq, flags in transcripts:
        if group != -1 and g != group:
            continue
        ctx = [START_] + list(seq)
        for p, is_target in enumerate(flags):
            if is_target:
                for j in range(1, min(order, p + 1) + 1):
                    table.setdefault(tuple(ctx[p + 1 - j:p + 1]), Counter())[seq[p]] += 1
    return table


def brute_forecast(model, history, group):
    """the words of the forecast, from the definitions: len = min(order, n + 1), j* the largest j <= len with examples, the candidates by
    (count descending, id ascending), the first 8 of them, the allowed mask by cnt den >= tot num"""
    table = brute_table(model.transcripts, model.order, group)
    ctx = [START_] + [s if 0 <= s < model.n_classes else NOTHING for s in history]
    for j in range(min(model.order, len(history) + 1), 0, -1):
        row = table.get(tuple(ctx[len(ctx) - j:]))
        if row:
            tot = sum(row.values())
            cand = sorted(row, key=lambda c: (-row[c], c))
            top = cand[:8]
            mask = sum(1 << c for c in row if row[c] * model.den >= tot * model.num)
            words = [(mask >> 32 * k) & 0xFFFFFFFF for k in range(4)]
            return ([1 | j << 8 | len(top) << 16, len(cand), tot, group] + [w - (1 << 32) if w >> 31 else w for w in words]
                    + top + [-1] * (8 - len(top)) + [row[c] for c in top] + [0] * (8 - len(top)))
    return [1 | 4, 0, 0, group, 0, 0, 0, 0] + [-1] * 8 + [0] * 8


def same_as_brute(model, history, group=-1):
    f = model.forecast(history, group)
    assert f.words() == brute_forecast(model, history, group), (history, group)
    return f


# ---- hand-made corpora (tests/test_gpu_forecast.py runs the same ones on the device) ----------------------------------------------------------------
def tie_corpora():
    """name -> (model, [(history, group)]): candidate counts 0, 1, 8, 9 and 128, and the ties the ranking has to break by id"""
    out = {}
    m = ProcedureModel(128, order=2, threshold=(1, 10))
    for c in range(128):                                                          # after [0]: every class once - 128 candidates, one tie
        m.add([0, c], 0)
    out["128 candidates, all tied"] = (m, [([0], 0), ([0], -1), ([5, 0], 0), ([], 0)])
    m = ProcedureModel(128, order=1)
    for c, n in ((5, 3), (69, 3), (63, 2), (64, 2), (127, 2), (0, 1)):            # 5 / 69 and 63 / 64: a lane's two halves, the lane edge
        for _ in range(n):
            m.add([1, c], 0)
    out["ties between ids 5 and 69, 63 and 64"] = (m, [([1], 0), ([9, 1], -1)])
    m = ProcedureModel(40, order=3, threshold=(1, 6))
    for c, n in zip(range(30, 21, -1), (9, 7, 7, 5, 5, 5, 5, 2, 2)):              # 9 candidates; ranks 8 and 9 tie at 2: id 22 wins, 23 is cut
        for _ in range(n):
            m.add([2, 3, c], 1)
    for c in range(8):
        m.add([4, c], 1)                                                          # exactly 8 candidates after [4]
    m.add([6, 7], 1)                                                              # exactly one after [6]; none after [7]
    m.add([11, 12], 3)                                                            # group 2 is empty, group 3 is the last
    out["8 and 9 candidates, a tie across the rank-8 boundary"] = (m, [
        ([2, 3], 1), ([4], 1), ([6], 1), ([7], 1), ([], 1), ([2], 1), ([9, 2, 3], 1), ([2, 40, 3], 1), ([2, 3, -7], 1), ([2, 3, 128], 1),
        ([2, 3], 2), ([2, 3], 0), ([2, 3], 4), ([2, 3], 1000), ([2, 3], -1), ([2, 3], -2), ([11], 3), ([11], -1), ([], -1), ([], 2)])
    return out


def test_the_hand_made_corpora_hit_what_they_are_for():
    c = tie_corpora()
    m, qs = c["128 candidates, all tied"]
    f = same_as_brute(m, [0], 0)
    assert f.n_cand == 128 and f.tot == 128 and f.ranked() == [(i, 1) for i in range(8)] and f.jstar == 2
    assert f.allowed() == [] and m.forecast([0], -1).words()[:3] == f.words()[:3]      # 1 * 10 < 128 * 1: nothing reaches the threshold
    assert same_as_brute(m, [], 0).ranked() == [(0, 128)]                              # START-only: one candidate
    m, qs = c["ties between ids 5 and 69, 63 and 64"]
    f = same_as_brute(m, [1], 0)
    assert f.ranked() == [(5, 3), (69, 3), (63, 2), (64, 2), (127, 2), (0, 1)] and f.n_cand == 6 and f.n_ranked == 6
    assert f.ids[6:] == (-1, -1) and f.cnts[6:] == (0, 0)
    m, qs = c["8 and 9 candidates, a tie across the rank-8 boundary"]
    f = same_as_brute(m, [2, 3], 1)
    assert f.n_cand == 9 and f.n_ranked == 8 and f.jstar == 3 and f.tot == 47
    assert f.ranked() == [(30, 9), (28, 7), (29, 7), (24, 5), (25, 5), (26, 5), (27, 5), (22, 2)]
    assert 23 not in f.ids and f.allowed() == [30]                                     # 9 * 6 >= 47, 7 * 6 < 47
    assert same_as_brute(m, [4], 1).ranked() == [(i, 1) for i in range(8)] and m.forecast([4], 1).n_cand == 8
    assert same_as_brute(m, [6], 1).ranked() == [(7, 1)]
    assert same_as_brute(m, [7], 1).words() == [MADE | UNKNOWN, 0, 0, 1] + [0] * 4 + [-1] * 8 + [0] * 8        # zero candidates
    assert same_as_brute(m, [2], 1).jstar == 2                                         # a history shorter than order: len = 2
    assert same_as_brute(m, [2, 40, 3], 1).jstar == 1                                  # an id outside the classes stops the match behind it
    assert same_as_brute(m, [2, 3, 128], 1).unknown and same_as_brute(m, [2, 3, -7], 1).unknown
    for g in (2, 0, 4, 1000, -2):                                                      # an empty group, groups outside the corpus
        assert same_as_brute(m, [2, 3], g).words() == [MADE | UNKNOWN, 0, 0, g] + [0] * 4 + [-1] * 8 + [0] * 8
    assert same_as_brute(m, [11], -1).ranked() == [(12, 1)] and same_as_brute(m, [], -1).n_cand == 4
    for name, (m, qs) in c.items():
        for h, g in qs:
            same_as_brute(m, h, g)


def _random_model(seed, ncls, order, threshold, targets="all"):
    rng = random.Random(seed)
    m = ProcedureModel(ncls, order=order, threshold=threshold, targets=targets)
    base = [[rng.randrange(ncls) for _ in range(rng.randint(3, 9))] for _ in range(4)]
    for _ in range(60):
        g = rng.randrange(4)
        m.add([s if rng.random() < 0.8 else rng.randrange(ncls) for s in base[g]][:rng.randint(1, 9)], g + (g == 3))      # group 3 stays empty
    seqs = [[rng.choice(base[rng.randrange(4)]) if rng.random() < 0.9 else rng.choice((ncls, -1, 200)) for _ in range(n)] for n in range(0, 14)]
    return m, seqs, [rng.choice((-1, 0, 1, 2, 3, 4, 9)) for _ in seqs]


@pytest.mark.parametrize("order,threshold,targets", [(1, (1, 6), "all"), (2, (0, 1), "all"), (3, (1, 3), "last"), (8, (1, 2), "all")])
def test_forecast_equals_the_restatement_and_the_judge_identity_holds(order, threshold, targets):
    m, seqs, grps = _random_model(order, 7, order, threshold, targets)
    all_f = m.forecast_sequences(seqs, grps)
    assert [len(fs) for fs in all_f] == [len(s) + 1 for s in seqs]
    n_known = 0
    for s, g, fs in zip(seqs, grps, all_f):
        for p in range(len(s) + 1):
            assert fs[p].words() == brute_forecast(m, s[:p], g), (s, p, g)
            if p < len(s):                                                         # the verdict of s[p] after s[:p] reads the same row
                v = m.judge(s[:p], s[p], g)
                assert (v.jstar, v.tot, v.mask, v.group, v.unknown) == (fs[p].jstar, fs[p].tot, fs[p].mask, fs[p].group, fs[p].unknown)
                table = brute_table(m.transcripts, m.order, g)
                if not v.unknown:
                    ctx = [START_] + [x if 0 <= x < 7 else NOTHING for x in s[:p]]
                    assert v.cnt == table[tuple(ctx[len(ctx) - v.jstar:])][s[p]]
                    n_known += 1
                assert v.mistake == (not v.unknown and s[p] not in fs[p].allowed())
    assert n_known >= 20


def test_words_round_trip_and_the_fixed_records():
    m, seqs, grps = _random_model(5, 128, 2, (1, 3))
    for fs in m.forecast_sequences(seqs, grps):
        for f in fs:
            w = f.words()
            assert len(w) == FORECAST_WORDS and all(-(1 << 31) <= x < 1 << 31 for x in w) and Forecast.from_words(w) == f
    f = Forecast.from_words([1 | 2 << 8 | 2 << 16, 2, 5, 3, -1, 0, 0, -(1 << 31)] + [127, 31] + [-1] * 6 + [3, 2] + [0] * 6)
    assert f.made and not f.unknown and not f.skipped and f.jstar == 2 and f.ranked() == [(127, 3), (31, 2)]
    assert f.allowed() == list(range(32)) + [127] and Forecast.from_words(f.words()) == f
    assert SKIPPED_FORECAST.words() == [SKIPPED, 0, 0, -1, 0, 0, 0, 0] + [-1] * 8 + [0] * 8
    assert SKIPPED_FORECAST.skipped and not SKIPPED_FORECAST.made and SKIPPED_FORECAST.ranked() == [] and MADE == JUDGED
    with pytest.raises(ValueError, match="2 sequences, 1 groups"):
        m.forecast_sequences([[1], [2]], [0])


# ---- Assembly101-O: how often the true next step is among the first k -------------------------------------------------------------------------------
def _golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "procedure_assembly101o.json")))


def brute_metrics(model, seqs, grps, ks):
    r = {"positions": 0, "unknown": 0, "top": {k: 0 for k in ks}}
    for s, g in zip(seqs, grps):
        for p in range(len(s)):
            w = brute_forecast(model, s[:p], g)
            r["positions"] += 1
            r["unknown"] += bool(w[0] & 4)
            for k in ks:
                r["top"][k] += s[p] in [c for c in w[8:8 + k] if c >= 0]
    return r


@pytest.mark.parametrize("which", ["gt", "pred"])
@pytest.mark.parametrize("order", [1, 2])
def test_anticipation_metrics_on_assembly101o(order, which):
    np = pytest.importorskip("numpy")
    golden = _golden()
    ncls = golden["n_classes"]
    m = ProcedureModel(ncls, order=order)
    for t in golden["transcripts"]:
        m.add(t["symbols"], t["group"])
    seqs, grps = [s[which] for s in golden["sequences"]], [s["group"] for s in golden["sequences"]]
    got = m.anticipation_metrics(seqs, grps)
    assert got == brute_metrics(m, seqs, grps, (1, 3, 5)) and got["positions"] == sum(len(s) for s in seqs)
    assert 0 <= got["top"][1] <= got["top"][3] <= got["top"][5] <= got["positions"] - got["unknown"]
    per_class = {}
    for g in sorted(set(grps)):                                                    # the rows of the DESIGN table add up to the total
        sub = [s for s, gg in zip(seqs, grps) if gg == g]
        per_class[g] = m.anticipation_metrics(sub, [g] * len(sub))
    assert sum(r["positions"] for r in per_class.values()) == got["positions"]
    assert {k: sum(r["top"][k] for r in per_class.values()) for k in (1, 3, 5)} == got["top"]
    if order == 1:                                                                 # order 1 is an argsort of the transition-count matrix
        T = np.zeros((len(golden["group_names"]), ncls + 1, ncls), dtype=np.int64)     # [group][previous step; ncls: START][next step]
        for t in golden["transcripts"]:
            prev = ncls
            for s in t["symbols"]:
                T[t["group"], prev, s] += 1
                prev = s
        want = {"positions": 0, "unknown": 0, "top": {1: 0, 3: 0, 5: 0}}
        for s, g in zip(seqs, grps):
            prev = ncls
            for step in s:
                row = T[g, prev]
                ranked = [int(c) for c in np.argsort(-row, kind="stable") if row[c] > 0]       # stable: equal counts by ascending id
                want["positions"] += 1
                want["unknown"] += not ranked
                for k in (1, 3, 5):
                    want["top"][k] += step in ranked[:k]
                prev = step
        assert got == want
    with pytest.raises(ValueError, match="each 1..8"):
        m.anticipation_metrics(seqs, grps, ks=(1, 9))


# ---- the monitor's host model -----------------------------------------------------------------------------------------------------------------------
def test_monitor_model_forecasts_on_hand_built_records():
    model = ProcedureModel(6, order=2, threshold=(1, 4))
    for seq, g in (([0, 1, 2, 3], 0), ([0, 1, 3], 0), ([0, 2, 1], 1), ([1, 2, 3, 4], 1)):
        model.add(seq, g)
    records = [OnlineRecord(1, 6, 3) for _ in range(4)]
    mirror = MonitorModel(records, model, max_out=16)
    mirror.set_group([0, 1], [0, 1])
    for i in (0, 1):
        records[0].push(i)
    for i in (0, 2, 1, 4, 5):                                                     # max_events 3: the record is full, OVERFLOW_FULL
        records[1].push(i)
    records[2].push(7)                                                            # an id outside the classes: an overflow entry, no event
    r = mirror.drain()
    fs = [mirror.forecast_entry(e) for e in r["entries"]]
    assert [e[:2] for e in r["entries"]] == [(0, 0), (0, 1), (1, -1), (1, 0), (1, 1), (1, 2), (2, -1)]
    assert r["entries"][6][2] == OVERFLOW_BAD_ID
    want = [model.forecast([0], 0), model.forecast([0, 1], 0), SKIPPED_FORECAST, model.forecast([0], 1), model.forecast([0, 2], 1),
            model.forecast([0, 2, 1], 1), SKIPPED_FORECAST]
    assert fs == want and [f.skipped for f in fs] == [v.skipped for v in r["verdicts"]]
    assert fs[1].ranked() == [(2, 1), (3, 1)] and fs[4].ranked() == [(1, 1)] and r["verdicts"][2] == SKIPPED_VERDICT
    # the forecast after entry k is the row the NEXT entry of the slot is judged on
    assert (fs[3].jstar, fs[3].tot, fs[3].mask) == (r["verdicts"][4].jstar, r["verdicts"][4].tot, r["verdicts"][4].mask)
    # an event the record no longer holds: the slot was reset behind the feed's back
    stale = r["entries"][1]
    records[0] = OnlineRecord(1, 6, 3)
    assert mirror.forecast_entry(stale) == SKIPPED_FORECAST and mirror.judge_entry(stale) == SKIPPED_VERDICT
    # by slot: every event the record holds; no event: START-only; a full record: max_events of them; outside: SKIPPED; a slot twice
    got = mirror.forecast_slots([1, 3, 0, 1, 4, -1])
    assert got == [model.forecast([0, 2, 1], 1), model.forecast([], -1), model.forecast([], 0), model.forecast([0, 2, 1], 1),
                   SKIPPED_FORECAST, SKIPPED_FORECAST]
    assert got[1].ranked() == [(0, 3), (1, 1)] and got[2].group == 0
    mirror.forget([1])
    assert mirror.forecast_slots([1])[0] == model.forecast([0, 2, 1], -1)
