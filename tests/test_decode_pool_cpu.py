"""CPU: the host model of online fixed-lag Viterbi decoding (prego_amd/decode.py, `OnlineDecoder`) held to the existing offline
`viterbi_decode` through the prefix identity label(f) = viterbi_decode(x[: min(f + L, T - 1) + 1])[0][f]; the cuts of a stream into
pushes; the far-state stream; `SlotTable.open(slot)`; the public header's declarations."""
import os
import re

import numpy as np
import pytest

from prego_amd import _lib
from prego_amd.aggregate import OVERFLOW_BAD_ID, OnlineRecord
from prego_amd.decode import DECODE_PENDING, OnlineDecoder, viterbi_decode
from tests.helpers.decode_pool_cases import CLASSES_CPU, LAGS_CPU, cpu_cases, cuts, dying_stream, far_state_stream, prefix_labels, run_host

CASES = cpu_cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_case_set_covers_what_it_must():
    names = " ".join(c[0] for c in CASES)
    for C in CLASSES_CPU:
        assert f"C{C}_" in names
    for lag in LAGS_CPU:
        assert f"_L{lag}_" in names
    assert {len(c[1]) for c in CASES} >= {1, 2, 90} and "_p" in names and "_c" in names and "hand_" in names
    assert any(c[3] is None for c in CASES) and any(c[3] is not None for c in CASES)


def test_prefix_identity_cost_and_end_after_every_frame():
    differ, died_late = 0, 0
    for name, x, trans, init, lag in CASES:
        want, recs = prefix_labels(x, trans, init, lag)
        dec = OnlineDecoder(trans, init, lag=lag, n_classes=x.shape[1])
        got = []
        for t in range(len(x)):
            lab, now = dec.push(x[t:t + 1])
            got.append(lab)
            cost, end = recs[t]
            assert (dec.cost, dec.end) == (cost, end) and now.tolist() == [end], (name, t)
            assert dec.frames == t + 1 and dec.committed == max(0, t + 1 - lag) and dec.dead == (end < 0)
        got.append(dec.flush())
        got = np.concatenate(got)
        assert got.dtype == np.int32 and np.array_equal(got, want), (name, got.tolist(), want.tolist())
        assert dec.committed == len(x) and dec.flushed
        offline = viterbi_decode(x, trans, init)[0]
        if lag >= len(x) - 1:
            assert np.array_equal(got, offline), name
        differ += int((got != offline).sum())
        died_late += int(dec.dead and (got >= 0).any())
    assert differ > 0, "no case shows the lag: every label equals the offline decode"
    assert died_late > 0, "no dead stream with labels committed before it died"


def test_dead_stream_keeps_committed_labels_and_sets_the_bad_id_bit():
    x, trans, init = dying_stream()
    dec, labels, now = run_host(x, trans, init, 2, [1] * len(x))
    assert labels.tolist() == [0] + [-1] * 7 and now.tolist() == [0, 1, 2] + [-1] * 5
    assert dec.dead and dec.cost == -1 and dec.end == -1
    assert dec.record.overflow & OVERFLOW_BAD_ID and dec.record.frames == 1 and dec.record.event_id == [0]


@pytest.mark.parametrize("kind", ["burst", "ragged", "whole"])
def test_any_cut_into_pushes_gives_the_same_outputs_and_record(kind):
    rng = np.random.default_rng(5)
    for name, x, trans, init, lag in CASES[::3]:
        ref, lab0, now0 = run_host(x, trans, init, lag, [1] * len(x))
        counts = [len(x)] if kind == "whole" else cuts(len(x), kind, rng)
        dec, lab1, now1 = run_host(x, trans, init, lag, counts)
        assert np.array_equal(lab0, lab1) and np.array_equal(now0, now1), name
        assert np.array_equal(ref.state_words(), dec.state_words()) and ref.record.to_words() == dec.record.to_words(), name


def test_record_takes_the_committed_labels_in_frame_order():
    rng = np.random.default_rng(6)
    x = rng.integers(0, 3000, (80, 5)).astype(np.int32)
    trans = np.full((5, 5), 300, np.int64) - np.diag(np.full(5, 300))
    for window in (1, 7):
        dec, labels, _ = run_host(x, trans, None, 5, [16] * 5, vote_window=window)
        rec = OnlineRecord(window, 5, 1024)
        rec.push_frames(labels.tolist())
        rec.flush()
        assert rec.to_words() == dec.record.to_words()
    dec, labels, _ = run_host(x, trans, None, 5, [16] * 5)
    changes = [0] + [f for f in range(1, 80) if labels[f] != labels[f - 1]]
    assert dec.record.event_start == changes and dec.record.event_id == [int(labels[f]) for f in changes]


def test_push_after_flush_ingests_nothing():
    x, trans, init = far_state_stream()
    dec, _, _ = run_host(x[:10], trans, init, 4, [10])
    before = dec.state_words().copy()
    lab, now = dec.push(x[10:13])
    assert lab.tolist() == [DECODE_PENDING] * 3 and now.tolist() == [DECODE_PENDING] * 3
    after = dec.state_words()
    assert after[2] == before[2] | 4 and np.array_equal(np.delete(after, 2), np.delete(before, 2)) and dec.flush().size == 0


def test_far_state_stream_needs_the_exact_keys():
    x, trans, init = far_state_stream()
    dec = OnlineDecoder(trans, init, lag=64)
    labels, spread, at = [], 0, 0
    while at < len(x):
        labels.append(dec.push(x[at:at + 1])[0])
        at += 1
        d = dec.keys()[:3] >> 7
        spread = max(spread, int(d.max() - d.min()))
    labels.append(dec.flush())
    labels = np.concatenate(labels)
    assert spread == 19_660_200 and spread >= 1 << 24
    assert (dec.keys()[:3] >> 7).tolist() == [22_936_900, 22_939_900, 19_660_200] and (dec.keys()[:3] & 127).tolist() == [0, 1, 2]
    assert (labels[:1136] == 0).all() and (labels[1136:] == 2).all() and len(labels) == 1300
    assert np.array_equal(labels, prefix_labels_sparse(x, trans, init, 64, (0, 600, 1071, 1072, 1135, 1136, 1299)))


def prefix_labels_sparse(x, trans, init, lag, frames):
    """the prefix identity at a few frames only (a prefix decode per frame is quadratic), the others as the run above says"""
    want = np.where(np.arange(len(x)) < 1136, 0, 2).astype(np.int32)
    for f in frames:
        want[f] = viterbi_decode(x[:min(f + lag, len(x) - 1) + 1], trans, init)[0][f]
    return want


def test_slot_table_opens_a_named_slot_and_keeps_its_default():
    from prego_amd._lib import PregoError
    from prego_amd.stream_pool import SlotTable
    t = SlotTable(6)
    assert t.open() == 0 and t.open(slot=4) == 4 and t.open() == 1 and t.open(2) == 2 and t.open() == 3 and t.open() == 5 and t.free == 0
    with pytest.raises(PregoError):
        t.open()
    t.release(4)
    for bad in (2, 6, -1):
        with pytest.raises(PregoError):
            t.open(bad)
    assert t.open() == 4


def test_header_declares_every_new_symbol_and_the_abi_is_still_7():
    hdr = open(os.path.join(ROOT, "include", "prego_amd.h")).read()
    assert re.search(r"#define PREGO_ABI_VERSION 7\b", hdr)
    assert re.search(r"#define PREGO_DECODE_POOL_MAX_LAG 256\b", hdr) and re.search(r"#define PREGO_DECODE_PENDING \(-2\)", hdr)
    assert (_lib.DECODE_POOL_MAX_LAG, _lib.DECODE_PENDING) == (256, -2) == (256, DECODE_PENDING)
    new = ["prego_decode_pool_bytes", "prego_decode_pool_create", "prego_decode_pool_destroy", "prego_decode_pool_push",
           "prego_decode_pool_push_costs", "prego_decode_pool_flush", "prego_decode_pool_reset", "prego_decode_pool_record",
           "prego_decode_pool_state", "prego_decode_pool_feed_create", "prego_decode_pool_feed_judge", "prego_decode_pool_feed_forecast",
           "prego_decode_pool_forecast"]
    for sym in new:
        assert re.search(r"\b" + sym + r"\(", hdr), sym
        assert sym in _lib.SYMBOLS
    # the binding's definitions are the header's, word for word
    doc = __import__("prego_amd.decode", fromlist=["x"]).__doc__
    for line in ("label(f) = viterbi_decode(x[: min(f + L, T - 1) + 1])[0][f]", "Consecutive labels come from different chains",
                 "e_t is the lowest j with the smallest finite d_t(j)"):
        assert line in doc and line in hdr
