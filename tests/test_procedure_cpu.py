"""CPU side of the procedure model (prego_amd/procedure.py: ProcedureModel, Verdict; prego_amd/stream_pool.py: MonitorModel): the host
model the device is held against in tests/test_gpu_procedure.py.  Hand-computed verdicts for every clause of the definition (DESIGN
13l), order 1 against a restatement of the reference's transition-matrix rule (step_anticipation/src/data/frequentist_baseline.py) in
integers, and the Assembly101-O numbers of the golden fixture tests/golden/procedure_assembly101o.json (scripts/gen_procedure_golden.py
wrote it from the reference's data files), which must be the counts measured when the model was proposed."""
import json
import os
import random
import re

import pytest

from prego_amd.aggregate import OVERFLOW_BAD_ID, OnlineRecord
from prego_amd.procedure import JUDGED, MISTAKE, SKIPPED, SKIPPED_VERDICT, UNKNOWN, ProcedureModel, Verdict
from prego_amd.stream_pool import FeedModel, MonitorModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = (([0, 1, 2], 0), ([0, 1, 3], 0), ([0, 2], 0), ([4, 1, 2], 1))


def _model(order=2, threshold=(0, 1), targets="all", n_classes=5):
    return ProcedureModel.from_transcripts(CORPUS, n_classes, order=order, threshold=threshold, targets=targets)


def _v(mistake, j, cnt, tot, group, allowed):
    return Verdict(JUDGED | (MISTAKE if mistake else 0) | j << 8, cnt, tot, group, sum(1 << c for c in allowed))


def test_hand_computed_verdicts():
    m = _model()
    assert (m.n_groups, m.n_symbols, m.n_examples) == (2, 11, 11)
    # START matches only START: the three transcripts of group 0 begin with 0, and nothing else is an example of the empty history
    assert m.judge([], 0, 0) == _v(False, 1, 3, 3, 0, [0])
    assert m.judge([], 1, 0) == _v(True, 1, 0, 3, 0, [0])
    # the whole order: after START, 0 came 1, 1, 2
    assert m.judge([0], 1, 0) == _v(False, 2, 2, 3, 0, [1, 2])
    # back-off: (3, 0) was never seen, (0) was
    assert m.judge([3, 0], 2, 0) == _v(False, 1, 1, 3, 0, [1, 2])
    assert m.judge([3, 0], 3, 0) == _v(True, 1, 0, 3, 0, [1, 2])
    # (START, 1) was never seen - 1 never began a transcript -, (1) was
    assert m.judge([1], 3, 0) == _v(False, 1, 1, 2, 0, [2, 3])
    # nothing ever followed 2: UNKNOWN, and not a mistake
    for g in (0, 1, -1):
        v = m.judge([0, 1, 2], 0, g)
        assert v == Verdict(JUDGED | UNKNOWN, 0, 0, g, 0) and v.unknown and not v.mistake and v.jstar == 0
    # a symbol outside the classes equals nothing: the history ends there
    assert m.judge([0, 99], 1, 0).unknown and m.judge([0, -1], 1, 0).unknown
    assert m.judge([0], 99, 0) == _v(True, 2, 0, 3, 0, [1, 2])
    assert m.judge([0], -1, 0).mistake


def test_a_history_shorter_than_the_order():
    m = _model(order=8)
    assert m.judge([], 0, 0) == _v(False, 1, 3, 3, 0, [0])                    # j <= i + 1 = 1
    assert m.judge([0], 2, 0) == _v(False, 2, 1, 3, 0, [1, 2])
    assert m.judge([0, 1], 3, 0) == _v(False, 3, 1, 2, 0, [2, 3])             # START, 0, 1 in full
    assert m.judge([4, 0, 1], 3, 0) == _v(False, 2, 1, 2, 0, [2, 3])          # (4, 0, 1) backs off to (0, 1)


def test_the_threshold_boundary_is_allowed():
    assert _model(threshold=(1, 3)).judge([0], 2, 0) == _v(False, 2, 1, 3, 0, [1, 2])        # 1 * 3 == 3 * 1
    assert _model(threshold=(2, 5)).judge([0], 2, 0) == _v(True, 2, 1, 3, 0, [1])            # 1 * 5 < 3 * 2
    assert _model(threshold=(2, 3)).judge([0], 1, 0) == _v(False, 2, 2, 3, 0, [1])           # 2 * 3 == 3 * 2
    assert _model(threshold=(1, 1)).judge([0], 1, 0) == _v(True, 2, 2, 3, 0, [])             # only a step that always came
    assert _model(threshold=(1, 1)).judge([], 0, 0) == _v(False, 1, 3, 3, 0, [0])
    assert _model(threshold=(0, 1)).judge([0], 3, 0).mistake                                   # never seen is never allowed
    for bad in ((2, 1), (-1, 2), (0, 0), (1, 32769)):
        with pytest.raises(ValueError, match="threshold"):
            ProcedureModel(5, threshold=bad)
    assert ProcedureModel(5, threshold=(32768, 32768)).den == 32768


def test_groups_are_isolated_and_minus_one_is_all_of_them():
    m = _model()
    assert m.judge([4], 1, 0).unknown                                          # 4 belongs to group 1 alone
    assert m.judge([4], 1, 1) == _v(False, 2, 1, 1, 1, [1])
    assert m.judge([4], 1, -1) == _v(False, 2, 1, 1, -1, [1])
    assert m.judge([1], 2, 0) == _v(False, 1, 1, 2, 0, [2, 3])
    assert m.judge([1], 2, 1) == _v(False, 1, 1, 1, 1, [2])
    assert m.judge([1], 2, -1) == _v(False, 1, 2, 3, -1, [2, 3])
    assert m.judge([], 4, -1) == _v(False, 1, 1, 4, -1, [0, 4])
    assert m.judge([0], 1, 7) == Verdict(JUDGED | UNKNOWN, 0, 0, 7, 0)         # a group the corpus does not have
    with pytest.raises(ValueError, match="group -1"):
        m.add([0], -1)
    with pytest.raises(ValueError, match=r"step id 5 outside \[0, 5\)"):
        m.add([0, 5], 0)


def test_targets_last_against_all():
    every, last = _model(), _model(targets="last")
    assert (last.n_symbols, last.n_examples) == (11, 4)
    assert not every.judge([], 0, 0).unknown and last.judge([], 0, 0).unknown  # no transcript of one symbol: START is no example's context
    assert not every.judge([0], 1, 0).mistake
    assert last.judge([0], 1, 0) == _v(True, 2, 0, 1, 0, [2])                  # only [0, 2] ends after START, 0
    assert last.judge([0, 1], 3, 0) == every.judge([0, 1], 3, 0) == _v(False, 2, 1, 2, 0, [2, 3])
    m = ProcedureModel(5).add([0, 1, 2], 0, targets=[0, 1, 0])                 # a flag per position
    assert m.n_examples == 1 and m.judge([0], 1, 0) == _v(False, 2, 1, 1, 0, [1]) and m.judge([0, 1], 2, 0).unknown


def test_the_prompt_parser():
    text = ("Sequence type: a21\nInput Sequence:\n -1, 39, 74, 58, 13\nNext Symbol:\n 37\n---\nSequence type: c03d\nInput Sequence:\n -1\n"
            "Next Symbol:\n 5\n---\nInput Sequence:\n -1, 2\nNext Symbol:\n 2\n---\n")
    assert ProcedureModel.parse_context_prompt(text) == [[39, 74, 58, 13, 37], [5], [2, 2]]
    m = ProcedureModel(86, order=1).from_context_prompt(text, group=3)
    assert (m.n_groups, m.n_symbols, len(m.transcripts)) == (4, 8, 3) and m.judge([13], 37, 3) == _v(False, 1, 1, 1, 3, [37])
    for bad in ("Input Sequence:\n 1, 2\nNext Symbol:\n 3", "Input Sequence:\n -1, 2\n", "Input Sequence:\n -1, -1\nNext Symbol:\n 3", "hello"):
        with pytest.raises(ValueError, match="parse_context_prompt"):
            ProcedureModel.parse_context_prompt(bad)


def test_verdict_words_round_trip_and_the_flat_corpus():
    v = Verdict(JUDGED | MISTAKE | 3 << 8, 5, 9, -1, 1 << 127 | 1 << 64 | 1 << 31 | 1)
    assert v.words() == [0x303, 5, 9, -1, -(1 << 31) + 1, 0, 1, -(1 << 31)] and Verdict.from_words(v.words()) == v
    assert v.allowed == [0, 31, 64, 127] and v.jstar == 3 and SKIPPED_VERDICT.words() == [SKIPPED, 0, 0, -1, 0, 0, 0, 0]
    groups, offsets, symbols, flags = _model(targets="last").flat()
    assert groups == [0, 0, 0, 1] and offsets == [0, 3, 6, 8, 11] and symbols == [0, 1, 2, 0, 1, 3, 0, 2, 4, 1, 2]
    assert flags == [0, 0, 1, 0, 0, 1, 0, 1, 0, 0, 1]


# ---- order 1 is the reference's baseline --------------------------------------------------------------------------------------------------------
def _baseline_mistake(A, n_states, prev, cur):
    """frequentist_baseline.py:28-59 without the division: row `prev` of the transition counts (START is state -1), threshold
    1 / n_states; a row without counts is filled with the threshold, which is not below it"""
    row = A.get(prev, {})
    tot = sum(row.values())
    return tot > 0 and row.get(cur, 0) * n_states < tot                       # p = cnt / tot < 1 / n_states


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_order_1_is_the_transition_matrix_rule(seed):
    rng = random.Random(seed)
    ncls = rng.choice((4, 9, 30))
    transcripts = [[rng.randrange(ncls) for _ in range(rng.randint(1, 12))] for _ in range(rng.randint(5, 60))]
    n_states = 1 + len({s for t in transcripts for s in t})                   # all_samples: the steps seen and the initial padding
    A = {}
    for t in transcripts:
        prev = -1
        for s in t:
            A.setdefault(prev, {}).setdefault(s, 0)
            A[prev][s] += 1
            prev = s
    m = ProcedureModel.from_transcripts([(t, 0) for t in transcripts], ncls, order=1, threshold=(1, n_states))
    n_mistakes = n_unknown = 0
    for _ in range(300):
        seq = [rng.randrange(ncls) for _ in range(rng.randint(1, 10))]
        prev = -1
        for i, s in enumerate(seq):
            v = m.judge(seq[:i], s, 0)
            assert v.mistake == _baseline_mistake(A, n_states, prev, s), (seq, i)
            assert v.unknown == (prev not in A) and (v.tot, v.cnt) == (sum(A.get(prev, {}).values()), A.get(prev, {}).get(s, 0))
            n_mistakes += v.mistake
            n_unknown += v.unknown
            prev = s
    assert n_mistakes > 20 and (n_unknown > 0 or ncls < 30)


# ---- Assembly101-O ---------------------------------------------------------------------------------------------------------------------------------
# (order, targets, sequences) -> tp, fp, fn, tn, unknown (None: not recorded): the numbers measured when the model was proposed
MEASURED = {(1, "all", "gt"): (136, 184, 46, 298, 26), (1, "all", "pred"): (93, 211, 89, 250, 47),
            (2, "all", "gt"): (146, 215, 36, 267, None), (2, "all", "pred"): (111, 242, 71, 219, None),
            (1, "last", "gt"): (65, 92, 117, 390, 486)}


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "procedure_assembly101o.json")))


def golden_model(golden, order, targets="all", threshold=(0, 1)):
    m = ProcedureModel(golden["n_classes"], order=order, threshold=threshold, targets=targets)
    for t in golden["transcripts"]:
        m.add(t["symbols"], t["group"])
    return m


def test_the_golden_corpus(golden):
    assert golden["n_classes"] == 86 and len(golden["group_names"]) == 15 and len(golden["sequences"]) == 182
    m = golden_model(golden, 2)
    # 1105 symbols as the prompts write them: 970 steps and the -1 in front of each of the 135 transcripts
    assert (m.n_groups, m.n_symbols, len(m.transcripts), m.n_symbols + len(m.transcripts)) == (15, 970, 135, 1105)
    assert golden["n_symbols"] == m.n_symbols == m.n_examples
    assert all(0 <= s["group"] < 15 and s["pred"] and s["gt"] for s in golden["sequences"])


@pytest.mark.parametrize("key", sorted(MEASURED))
def test_assembly101o_counts_are_the_measured_ones(golden, key):
    order, targets, which = key
    r = golden_model(golden, order, targets).mistake_metrics([s[which] for s in golden["sequences"]], [s["group"] for s in golden["sequences"]])
    tp, fp, fn, tn, unknown = MEASURED[key]
    assert (r["tp"], r["fp"], r["fn"], r["tn"]) == (tp, fp, fn, tn)
    assert unknown is None or r["unknown"] == unknown
    assert tp + fn == 182 and r["f1"] == pytest.approx(2 * tp / (2 * tp + fp + fn))
    recorded = [e for e in golden["expected"] if (e["order"], e["targets"], e["sequences"]) == key]
    assert len(recorded) == 1 and {k: r[k] for k in ("tp", "fp", "fn", "tn", "unknown")} == {k: recorded[0][k] for k in ("tp", "fp", "fn", "tn", "unknown")}


def test_f1_of_the_proposal(golden):
    f1 = {w: golden_model(golden, 2).mistake_metrics([s[w] for s in golden["sequences"]], [s["group"] for s in golden["sequences"]])["f1"]
          for w in ("pred", "gt")}
    assert round(f1["pred"], 3) == 0.415 and round(f1["gt"], 3) == 0.538


# ---- the monitor's host model -------------------------------------------------------------------------------------------------------------------------
def test_monitor_model_judges_what_the_feed_model_drains():
    m = _model()
    records = [OnlineRecord(1, 5, 3) for _ in range(3)]
    mon, plain = MonitorModel(records, m, max_out=4), FeedModel([OnlineRecord(1, 5, 3) for _ in range(3)], 4)
    mon.set_group([0, 2], [0, 1])
    for ids in ((0, 0, 4), (1, 9, 1), (3, 2, 2)):
        for s, i in enumerate(ids):
            records[s].push(i)
            plain.records[s].push(i)
    r = mon.drain()
    assert {k: r[k] for k in ("count", "pending", "seq", "entries")} == plain.drain()           # the feed is FeedModel's
    assert r["entries"] == [(0, 0, 0, 0), (0, 1, 1, 1), (0, 2, 3, 2), (1, -1, OVERFLOW_BAD_ID, 2)] and r["pending"] == 5
    assert r["verdicts"] == [m.judge([], 0, 0), m.judge([0], 1, 0), m.judge([0, 1], 3, 0), SKIPPED_VERDICT]
    r = mon.drain()
    assert r["entries"] == [(1, 0, 0, 0), (1, 1, 2, 1), (2, 0, 4, 0), (2, 1, 1, 1)]
    assert r["verdicts"] == [m.judge([], 0, -1), m.judge([0], 2, -1), m.judge([], 4, 1), m.judge([4], 1, 1)]
    records[2] = OnlineRecord(1, 5, 3)                                          # the pool closed slot 2 ...
    mon.forget([2])
    assert mon.groups == [0, -1, -1]                                            # ... and its group went with it
    records[2].push(0)
    r = mon.drain()
    assert r["entries"] == [(2, 0, 0, 0)] and r["verdicts"] == [m.judge([], 0, -1)]
    assert mon.judge_entry((0, 3, 1, 3)).skipped                                # an event the record does not hold


def test_the_entry_points_are_declared_and_bound():
    from prego_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "prego_amd.h")).read()
    for name, n_args in (("prego_procedure_model_bytes", 4), ("prego_procedure_model_create", 13), ("prego_procedure_model_destroy", 1),
                         ("prego_procedure_judge", 9), ("prego_stream_pool_feed_judge", 8), ("prego_vit_stream_pool_feed_judge", 8)):
        m = re.search(r"\b(?:int|size_t|void)\s+" + name + r"\s*\(([^;]*)\);", hdr)
        assert m, f"{name} is not declared in include/prego_amd.h"
        assert len(m.group(1).split(",")) == n_args, name
        assert name in _lib.SYMBOLS
    assert "#define PREGO_ABI_VERSION 7" in hdr
