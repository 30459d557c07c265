"""The next-step forecast on the device (prego_procedure_forecast, prego_*stream_pool_feed_forecast, prego_*stream_pool_forecast,
`pool.forecast_monitor`; csrc/procedure.hip).  Every comparison is of integers and exact, word for word, against the
host model (prego_amd/procedure.py: ProcedureModel.forecast, itself held against a restatement in tests/test_forecast_cpu.py; for the
monitor prego_amd/stream_pool.py: MonitorModel over one OnlineRecord per slot fed the same ids):
  1. the offline entry over n_classes {1, 12, 86, 128} x order {1, 2, 8} on the 15-group corpora of tests/test_gpu_procedure.py,
     sequences of every length 0..40, and the judge identity against the device's own verdicts;  2. the tie and boundary corpora of the
     CPU test, a one-group corpus, an empty corpus, n_pos = 0;  3. the ForecastMonitor on a StreamPool of 300 slots under churn, beside
     a plain MistakeMonitor on a twin pool;  4. forecast_slots;  5. a TransformerStreamPool;  6. refusals, and no allocation or wait."""
import ctypes as C
import random

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import _lib                                            # noqa: E402
from prego_amd._lib import PregoError                                 # noqa: E402
from prego_amd.aggregate import OVERFLOW_BAD_ID, OVERFLOW_FULL, OnlineRecord   # noqa: E402
from prego_amd.procedure import FORECAST_WORDS, MADE, SKIPPED_FORECAST, UNKNOWN, ProcedureModel   # noqa: E402
from prego_amd.stream_pool import ForecastMonitor, MistakeMonitor, MonitorModel, StreamPool   # noqa: E402
from tests import test_forecast_cpu as FC                             # noqa: E402  the hand-made corpora
from tests import test_gpu_procedure as GP                            # noqa: E402  the 15-group corpora, the monitor's model
from tests import test_gpu_step_wide as TW                            # noqa: E402  the engines are built once and shared

DEV = "cuda:0"
EINVAL, EWORKSPACE = -1, -3
SENTINEL = 0x5A5A5A5A
UNKNOWN_TAIL = [0] * 4 + [-1] * 8 + [0] * 8


def _same_as_host(m, seqs, grps, dev=None):
    got = (dev or m.to(DEV)).forecast_sequences(seqs, grps)
    want = m.forecast_sequences(seqs, grps)
    assert [len(fs) for fs in got] == [len(s) + 1 for s in seqs]
    for s, (a, b) in enumerate(zip(got, want)):
        assert [f.words() for f in a] == [f.words() for f in b], (s, grps[s], seqs[s])
    return got


# ---- 1. the offline entry --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,threshold", [(1, (1, 12)), (2, (0, 1)), (8, (1, 3))])
@pytest.mark.parametrize("ncls", [1, 12, 86, 128])
def test_offline_forecast_equals_the_host_model(ncls, order, threshold):
    rng = random.Random(1000 * ncls + order)
    sizes = list(GP.EDGE_SIZES) + [0, 7, 130, 2, 64, 129, 3, 300, 0]         # 15 groups, two of them empty
    m, bases = GP._corpus(rng, ncls, sizes, order=order, threshold=threshold)
    seqs, grps = GP._queries(rng, ncls, bases, list(range(15)) + [-1, -1, 6, 40, -2])
    seqs, grps = [[]] + seqs[:20] + [[], []] + seqs[20:] + [[]], [3] + grps[:20] + [-1, 6] + grps[20:] + [0]      # length 0: first, inside, last
    assert sorted({len(s) for s in seqs}) == list(range(41))
    dev = m.to(DEV)
    got = _same_as_host(m, seqs, grps, dev)
    fs = [f for row in got for f in row]
    assert len(fs) == 820 + len(seqs) and all(f.flags & MADE and not f.skipped for f in fs)
    for s, g, row in zip(seqs, grps, got):
        if g in (6, 14, 40, -2):
            assert all(f.words() == [MADE | UNKNOWN, 0, 0, g] + UNKNOWN_TAIL for f in row)
    assert all(f.n_ranked == min(f.n_cand, 8) and sum(f.cnts) <= f.tot and (f.n_cand > 8 or sum(f.cnts) == f.tot) for f in fs)
    if ncls > 1:
        assert {f.jstar for f in fs} >= set(range(min(order, 3) + 1)), "the queries did not reach every back-off level"
    if ncls >= 86:
        assert any(f.n_cand > 8 for f in fs), "no forecast had to cut its candidates"
    # the judge identity, against the device's own verdicts: row (s, p) and the verdict of symbol p read the same histogram row
    verdicts = dev.judge_sequences(seqs, grps)
    for s, (row, vs) in enumerate(zip(got, verdicts)):
        for p, v in enumerate(vs):
            f = row[p]
            assert (v.jstar, v.tot, v.mask, v.group, v.unknown) == (f.jstar, f.tot, f.mask, f.group, f.unknown), (s, p)
            ranked = dict(f.ranked())
            if seqs[s][p] in ranked:
                assert v.cnt == ranked[seqs[s][p]]
            elif f.n_cand <= 8:
                assert v.cnt == 0


# ---- 2. ties, boundaries, small corpora ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FC.tie_corpora()))
def test_tie_and_boundary_corpora(name):
    m, queries = FC.tie_corpora()[name]
    seqs, grps = [h for h, _ in queries], [g for _, g in queries]
    got = _same_as_host(m, seqs, grps)
    for (h, g), row in zip(queries, got):                                     # the last row of a sequence: what follows all of it
        assert row[-1].words() == FC.brute_forecast(m, h, g), (h, g)


@pytest.mark.parametrize("n_examples", GP.EDGE_SIZES)
def test_one_group_of_every_edge_size(n_examples):
    rng = random.Random(n_examples)
    m, bases = GP._corpus(rng, 12, [n_examples], order=2, threshold=(1, 5))
    seqs, grps = GP._queries(rng, 12, bases, [0, -1])
    fs = [f for row in _same_as_host(m, seqs, grps) for f in row]
    assert max(f.tot for f in fs) <= n_examples and any(f.tot for f in fs)


def test_an_empty_corpus_and_no_positions():
    m = ProcedureModel(12)
    got = _same_as_host(m, [[1, 2, 3], [4], []], [-1, 0, 5])
    assert [f.words() for row in got for f in row] == [[MADE | UNKNOWN, 0, 0, g] + UNKNOWN_TAIL for g in (-1,) * 4 + (0,) * 2 + (5,)]
    assert m.to(DEV).forecast_sequences([], []) == []
    m = ProcedureModel(12, order=3).add([3, 4, 5], 0).add([3, 1], 0).add([2], 1)
    got = _same_as_host(m, [[], [], []], [0, 1, -1])                         # n_pos = 0: every row is START-only
    assert [row[0].ranked() for row in got] == [[(3, 2)], [(2, 1)], [(3, 2), (2, 1)]]


# ---- 3. the ForecastMonitor on a StreamPool -----------------------------------------------------------------------------------------------------------
NCLS = GP.NCLS


def _drain_same(mon, mirror, twin=None):
    t, want = mon.drain(), mirror.drain()
    got = {"count": t.count, "pending": t.pending, "seq": t.seq, "entries": t.events()}
    assert got == {k: want[k] for k in got}, (got, want)
    assert [v.words() for v in t.verdicts()] == [v.words() for v in want["verdicts"]], want["entries"]
    want["forecasts"] = [mirror.forecast_entry(e) for e in want["entries"]]
    assert [f.words() for f in t.forecasts()] == [f.words() for f in want["forecasts"]], want["entries"]
    assert len(t.forecasts()) == len(t.verdicts()) == len(t.events()) == t.count
    if twin is not None:                                                      # a plain MistakeMonitor on a pool fed the same
        tt = twin.drain()
        assert tt.events() == t.events() and [v.words() for v in tt.verdicts()] == [v.words() for v in t.verdicts()]
    return want


def test_forecast_monitor_equals_the_host_models_under_churn():
    e = TW._real_engine("bf16", 3)
    cap, max_out = 300, 5                                                     # up to 9 entries are due per tick
    pool, twin_pool = (StreamPool(e, capacity=cap, window=1, max_events=6) for _ in range(2))
    model = GP._monitor_model()
    mon = pool.forecast_monitor(model, max_out=max_out, depth=2)
    twin = twin_pool.mistake_monitor(mon.model, max_out=max_out, depth=2)
    assert isinstance(mon, ForecastMonitor) and isinstance(mon, MistakeMonitor) and type(twin) is MistakeMonitor
    records = [OnlineRecord(1, NCLS, 6) for _ in range(cap)]
    mirror = MonitorModel(records, model, max_out)
    for _ in range(cap):
        pool.open(), twin_pool.open()
    rng = random.Random(11)
    live = [0, 1, 63, 64, 255, 256, 257, 299]                                 # both workgroups of the drain, both sides of their boundary
    for x in (mon, twin, mirror):
        x.set_group(live[:6], [0, 1, 2, 0, 1, 2])                             # 257 and 299 stay at -1: every group
    seen, n_pending = [], 0
    for tick in range(9):
        votes = {s: rng.randrange(6) for s in live if rng.random() < 0.8}
        GP._vote(pool, records, votes)
        twin_pool.vote(list(votes), list(votes.values()))
        if tick == 3:
            GP._vote(pool, records, {1: NCLS})                                # an id outside the classes: an overflow entry, once
            twin_pool.vote([1], [NCLS])
        while True:
            r = _drain_same(mon, mirror, twin)
            seen += list(zip(r["entries"], r["forecasts"]))
            n_pending += r["pending"] > 0
            if not r["pending"]:
                break
    assert n_pending >= 3, "max_out never left entries pending"
    skipped = [(en, f) for en, f in seen if f.skipped]
    assert {en[2] for en, _ in skipped} == {OVERFLOW_BAD_ID, OVERFLOW_FULL} and all(en[1] == -1 and f == SKIPPED_FORECAST for en, f in skipped)
    made = [f for _, f in seen if not f.skipped]
    assert len(made) >= 30 and {f.group for f in made} == {-1, 0, 1, 2} and all(f.made for f in made)
    assert any(f.jstar >= 2 for f in made) and any(f.n_ranked >= 2 for f in made)


def test_a_reopened_slot_starts_again_and_set_group_holds_from_the_next_drain():
    e = TW._real_engine("bf16", 3)
    pool = StreamPool(e, capacity=300, window=1, max_events=16)
    model = GP._monitor_model()
    mon = pool.forecast_monitor(model, max_out=16, depth=2)
    records = [OnlineRecord(1, NCLS, 16) for _ in range(300)]
    mirror = MonitorModel(records, model, 16)
    slots = [pool.open() for _ in range(260)]
    a, b = slots[2], slots[258]
    ga, seq, _ = next(t for t in model.transcripts if len(t[1]) >= 5 and all(x != y for x, y in zip(t[1][:4], t[1][1:5])))
    mon.set_group([a], [ga])
    mirror.set_group([a], [ga])
    for i in seq[:3]:
        GP._vote(pool, records, {a: i, b: i})
    r = _drain_same(mon, mirror)
    assert [f.group for f in r["forecasts"]] == [ga] * 3 + [-1] * 3
    assert [f.words() for f in r["forecasts"][:3]] == [model.forecast(seq[:k], ga).words() for k in (1, 2, 3)]
    assert all(seq[k] in f.ids for k, f in zip((1, 2, 3), r["forecasts"][:3]))      # the corpus's own transcript: its next step is expected
    # close and reopen: the history and the group start again
    pool.close(a)
    records[a] = OnlineRecord(1, NCLS, 16)
    mirror.forget([a])
    assert mon.groups()[a] == -1 and pool.open() == a
    GP._vote(pool, records, {a: seq[3], b: seq[3]})
    r = _drain_same(mon, mirror)
    fa, fb = r["forecasts"]
    assert r["entries"][0][:2] == (a, 0) and fa.words() == model.forecast([seq[3]], -1).words() and fa.jstar <= 2
    assert r["entries"][1][:2] == (b, 3) and fb.words() == model.forecast(seq[:4], -1).words()
    # set_group between two drains that are both in flight: the first still forecasts b against every group
    nxt = seq[4 % len(seq)]
    GP._vote(pool, records, {b: nxt})
    t1 = mon.drain()
    mon.set_group([b], [2 - ga])
    nxt2 = (nxt + 1) % 6
    GP._vote(pool, records, {b: nxt2})
    t2 = mon.drain()
    with pytest.raises(PregoError, match="all 2 report buffers hold unread tickets"):
        mon.drain()
    assert t1.events() == [(b, 4, nxt, 4)] and t2.events() == [(b, 5, nxt2, 5)]
    h = seq[:4] + [nxt]
    assert [f.words() for f in t1.forecasts()] == [model.forecast(h, -1).words()]
    assert [f.words() for f in t2.forecasts()] == [model.forecast(h + [nxt2], 2 - ga).words()]
    assert [v.words() for v in t2.verdicts()] == [model.judge(h, nxt2, 2 - ga).words()] and t2.forecasts()[0].group == 2 - ga


# ---- 4. forecast_slots ----------------------------------------------------------------------------------------------------------------------------------
def test_forecast_slots_reads_what_the_records_hold():
    e = TW._real_engine("bf16", 3)
    cap, max_events = 300, 5
    pool = StreamPool(e, capacity=cap, window=1, max_events=max_events)
    model = GP._monitor_model()                                               # order 3
    mon = pool.forecast_monitor(model, max_out=64, depth=2)
    records = [OnlineRecord(1, NCLS, max_events) for _ in range(cap)]
    mirror = MonitorModel(records, model, 64)
    slots = [pool.open() for _ in range(cap)]
    g, seq, _ = next(t for t in model.transcripts if len(t[1]) >= 5 and all(x != y for x, y in zip(t[1], t[1][1:])))
    fed = {0: [], 1: seq[:1], 64: seq[:2], 257: seq[:4], 299: (seq + [seq[0], seq[1], seq[0]])[:8]}      # 0, 1, order - 1, many, a full record
    for k in range(8):
        GP._vote(pool, records, {s: ids[k] for s, ids in fed.items() if k < len(ids)})
    assert len(records[299].event_id) == max_events and records[299].overflow == OVERFLOW_FULL
    for x in (mon, mirror):
        x.set_group([64, 257], [g, 2 - g])
    ask = [299, 0, 1, 64, 257, 64, 2, 299]                                    # slots 64 and 299 twice
    t = mon.forecast_slots(ask)
    want = mirror.forecast_slots(ask)
    got = t.forecasts()
    assert [f.words() for f in got] == [f.words() for f in want]
    assert got[1].words() == model.forecast([], -1).words() and got[1].jstar == 1 and got[6] == got[1]
    assert got[3].words() == model.forecast(seq[:2], g).words() and got[3].jstar == 3 and got[3] == got[5] and got[0] == got[7]
    assert got[0].words() == model.forecast(records[299].event_id[:max_events], -1).words()
    assert all(f.made and not f.skipped for f in got)
    # the records are read as they are, drained or not; the whole pool in one call; `depth` tickets in flight
    mon.drain().events()
    every = list(range(cap))
    t1, t2 = mon.forecast_slots(every), mon.forecast_slots(ask[:3])
    with pytest.raises(PregoError, match="all 2 forecast buffers hold unread tickets"):
        mon.forecast_slots([0])
    assert [f.words() for f in t1.forecasts()] == [f.words() for f in mirror.forecast_slots(every)]
    assert [f.words() for f in t2.forecasts()] == [f.words() for f in want[:3]]
    pool.close(2)
    for bad, msg in (([2], "slot 2 is not open"), ([300], "slot 300 is not open"), ([], "0 slots"), (every + [0], "301 slots")):
        with pytest.raises(PregoError, match=msg):
            mon.forecast_slots(bad)


# ---- 5. a TransformerStreamPool ---------------------------------------------------------------------------------------------------------------------------
def test_forecast_monitor_on_a_transformer_pool():
    from tests import test_gpu_vit_stream_pool as VT
    m = VT._model()
    pool = m.stream_pool(capacity=2, vote_window=2, max_events=64)
    ncls = pool._ncls
    rng = random.Random(2)
    model = ProcedureModel(ncls, order=2, threshold=(1, 20))
    for k in range(400):                                                      # ~3000 examples over the classes: most single steps are known
        model.add([rng.randrange(ncls) for _ in range(rng.randint(4, 10))], k % 3)
    mon = pool.forecast_monitor(model, max_out=64)
    records = [OnlineRecord(2, ncls, 64) for _ in range(2)]
    mirror = MonitorModel(records, model, 64)
    slots = [pool.open() for _ in range(2)][::-1]                            # 1, 0
    mon.set_group(slots[:1], [1])
    mirror.set_group(slots[:1], [1])
    assert [f.words() for f in mon.forecast_slots(slots).forecasts()] == [model.forecast([], 1).words(), model.forecast([], -1).words()]
    vids = [(torch.from_numpy(r).to(DEV), torch.from_numpy(f).to(DEV)) for r, f in VT._videos()[:2]]
    n = 0
    for t in range(0, 16, 4):
        rgb = torch.cat([v[0][t:t + 4] for v in vids]).contiguous()
        flow = torch.cat([v[1][t:t + 4] for v in vids]).contiguous()
        _, argmax = pool.push_bursts(slots, 4, rgb, flow)
        for i, s in enumerate(slots):
            records[s].push_frames(argmax[4 * i:4 * i + 4].tolist())
        n += _drain_same(mon, mirror)["count"]
        twice = [slots[t // 4 % 2]] * 2                                         # a repeated slot, within the capacity of 2
        assert [f.words() for f in mon.forecast_slots(twice).forecasts()] == [f.words() for f in mirror.forecast_slots(twice)]
    assert n >= 2 and all(pool.events(s)["frames"] == 16 for s in slots)


# ---- 6. refusals write nothing ------------------------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def test_refusals_and_what_a_forecast_leaves_untouched():
    e = TW._real_engine("bf16", 3)
    lib = e.lib
    err = lambda: lib.prego_last_error().decode()
    host = ProcedureModel(5).add([0, 1, 2], 0).add([3, 4], 1)
    dm = host.to(DEV, lib=lib)
    m = dm.m

    # -- the offline entry: 2 sequences, 3 positions, 5 rows
    off_d = torch.tensor([0, 2, 3], dtype=torch.int32, device=DEV)
    sym_d = torch.tensor([0, 1, 3], dtype=torch.int32, device=DEV)
    grp_d = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    out = torch.full((5 * FORECAST_WORDS + 64,), SENTINEL, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    snaps = [t.clone() for t in (dm._block, out)]

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(t, s) for t, s in zip((dm._block, out), snaps))

    def forecast(mod=m, ns=2, npos=3, off=_p(off_d), sym=_p(sym_d), grp=_p(grp_d), o=_p(out), nb=5 * 96):
        return lib.prego_procedure_forecast(mod, ns, npos, off, sym, grp, o, nb, None)
    for kw, rc, msg in ((dict(mod=None), EINVAL, "model is NULL"), (dict(off=None), EINVAL, "offsets is NULL"), (dict(sym=None), EINVAL, "symbols is NULL"),
                        (dict(grp=None), EINVAL, "groups is NULL"), (dict(o=None), EINVAL, "forecasts is NULL"), (dict(ns=0), EINVAL, "0 sequences"),
                        (dict(npos=-1), EINVAL, "-1 positions"), (dict(ns=1 << 30, npos=1), EINVAL, "together at most"),
                        (dict(o=C.c_void_p(out.data_ptr() + 8)), EINVAL, "16-byte aligned"),
                        (dict(nb=5 * 96 - 1), EWORKSPACE, "5 rows need 480 (96 each)"), (dict(nb=0), EWORKSPACE, "need 480")):
        assert forecast(**kw) == rc and msg in err() and err().startswith("procedure_forecast"), (kw, err())
        assert untouched(), kw
    assert forecast(o=C.c_void_p(out.data_ptr() + 16)) == 0                  # 16-byte alignment is enough
    torch.cuda.synchronize()
    want = [f.words() for fs in host.forecast_sequences([[0, 1], [3]], [0, 1]) for f in fs]
    assert out[4:124].view(5, 24).cpu().tolist() == want and bool((out[:4] == SENTINEL).all()) and bool((out[124:] == SENTINEL).all())
    assert torch.equal(dm._block, snaps[0])

    # -- the feed entry and the slot entry, both pool types' symbols
    cap, max_out = 300, 8
    pool = StreamPool(e, capacity=cap, window=1, max_events=4)
    feed = pool.event_feed(max_out=max_out)
    s = pool.open()
    pool.vote([s], [0])
    rbytes, report = feed._report_bytes, feed._dev[0]
    assert lib.prego_stream_pool_feed_drain(feed.f, _p(report), rbytes, None) == 0
    grp = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
    ask = torch.tensor([s, cap, -1, s], dtype=torch.int32, device=DEV)       # outside the pool: SKIPPED rows, not a refusal (device words)
    out = torch.full((max_out * FORECAST_WORDS + 64,), SENTINEL, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    blocks = (pool._block, feed._block, report, grp, ask, dm._block, out)
    snaps = [t.clone() for t in blocks]

    def untouched_pool():
        torch.cuda.synchronize()
        return all(torch.equal(t, sn) for t, sn in zip(blocks, snaps))

    def ffeed(fn=lib.prego_stream_pool_feed_forecast, f=feed.f, mod=m, rep=_p(report), rb=rbytes, g=_p(grp), o=_p(out), nb=max_out * 96):
        return fn(f, mod, rep, rb, g, o, nb, None)
    for fn, who in ((lib.prego_stream_pool_feed_forecast, "stream_pool_feed_forecast"),
                    (lib.prego_vit_stream_pool_feed_forecast, "vit_stream_pool_feed_forecast")):
        for kw, rc, msg in ((dict(f=None), EINVAL, "feed is NULL"), (dict(mod=None), EINVAL, "model is NULL"), (dict(rep=None), EINVAL, "report is NULL"),
                            (dict(rep=C.c_void_p(report.data_ptr() + 16)), EINVAL, "the report must be 256-byte aligned"),
                            (dict(rb=rbytes - 1), EWORKSPACE, f"need {rbytes}"), (dict(g=None), EINVAL, "slot_groups is NULL"),
                            (dict(o=None), EINVAL, "forecasts is NULL"), (dict(o=C.c_void_p(out.data_ptr() + 4)), EINVAL, "the forecasts must be 16-byte aligned"),
                            (dict(nb=max_out * 96 - 96), EWORKSPACE, f"{max_out} entries need {max_out * 96}")):
            assert ffeed(fn=fn, **kw) == rc and msg in err() and err().startswith(who), (kw, err())
            assert untouched_pool(), kw
    assert ffeed() == 0
    torch.cuda.synchronize()
    assert out[:24].cpu().tolist() == host.forecast([0], -1).words()
    assert bool((out[24:] == SENTINEL).all()), "written behind forecast `count`"
    assert all(torch.equal(t, sn) for t, sn in zip(blocks[:6], snaps[:6])), "the forecast wrote what it only reads"
    out.fill_(SENTINEL)
    torch.cuda.synchronize()

    def fslots(fn=lib.prego_stream_pool_forecast, p=pool.p, mod=m, sl=_p(ask), n=4, g=_p(grp), o=_p(out), nb=4 * 96):
        return fn(p, mod, sl, n, g, o, nb, None)
    for kw, rc, msg in ((dict(p=None), EINVAL, "pool is NULL"), (dict(mod=None), EINVAL, "model is NULL"), (dict(sl=None), EINVAL, "slots is NULL"),
                        (dict(n=0), EINVAL, "0 slots (1..300"), (dict(n=cap + 1, nb=1 << 20), EINVAL, "301 slots (1..300"),
                        (dict(g=None), EINVAL, "slot_groups is NULL"), (dict(o=None), EINVAL, "forecasts is NULL"),
                        (dict(o=C.c_void_p(out.data_ptr() + 8)), EINVAL, "the forecasts must be 16-byte aligned"),
                        (dict(nb=4 * 96 - 1), EWORKSPACE, "4 slots need 384")):
        assert fslots(**kw) == rc and msg in err() and err().startswith("stream_pool_forecast"), (kw, err())
        assert untouched_pool(), kw
    for kw, msg in ((dict(p=None), "pool is NULL"), (dict(p=None, mod=None), "pool is NULL"), (dict(p=None, n=0), "pool is NULL")):
        assert fslots(fn=lib.prego_vit_stream_pool_forecast, **kw) == EINVAL and msg in err() and err().startswith("vit_stream_pool_forecast")
        assert untouched_pool(), kw
    assert fslots() == 0
    torch.cuda.synchronize()
    first = host.forecast([0], -1).words()
    assert out[:96].view(4, 24).cpu().tolist() == [first, SKIPPED_FORECAST.words(), SKIPPED_FORECAST.words(), first]
    assert bool((out[96:] == SENTINEL).all()) and all(torch.equal(t, sn) for t, sn in zip(blocks[:6], snaps[:6]))


def test_vit_pool_entries_refuse_as_the_gru_pool_entries():
    from tests import test_gpu_vit_stream_pool as VT
    pool = VT._model().stream_pool(capacity=2, vote_window=2, max_events=8)
    lib = pool.lib
    err = lambda: lib.prego_last_error().decode()
    dm = ProcedureModel(pool._ncls).add([0, 1], 0).to(DEV, lib=lib)
    grp = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    ask = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    out = torch.full((2 * FORECAST_WORDS + 16,), SENTINEL, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    snap = pool._block.clone()

    def fslots(p=pool.p, mod=dm.m, sl=_p(ask), n=2, g=_p(grp), o=_p(out), nb=2 * 96):
        return lib.prego_vit_stream_pool_forecast(p, mod, sl, n, g, o, nb, None)
    for kw, rc, msg in ((dict(mod=None), EINVAL, "model is NULL"), (dict(sl=None), EINVAL, "slots is NULL"), (dict(n=0), EINVAL, "0 slots (1..2"),
                        (dict(n=3), EINVAL, "3 slots (1..2"), (dict(g=None), EINVAL, "slot_groups is NULL"), (dict(o=None), EINVAL, "forecasts is NULL"),
                        (dict(o=C.c_void_p(out.data_ptr() + 4)), EINVAL, "16-byte aligned"), (dict(nb=95), EWORKSPACE, "2 slots need 192")):
        assert fslots(**kw) == rc and msg in err() and err().startswith("vit_stream_pool_forecast"), (kw, err())
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and torch.equal(pool._block, snap), kw
    assert fslots() == 0
    torch.cuda.synchronize()
    assert out[:48].view(2, 24).cpu().tolist() == [dm.host.forecast([], -1).words()] * 2 and bool((out[48:] == SENTINEL).all())


def test_forecasting_allocates_nothing_and_waits_for_nothing():
    dbg = _lib.load_debug()
    e = TW._real_engine("bf16", 8, lib=dbg)
    pool = StreamPool(e, capacity=300, window=1)
    slots = [pool.open() for _ in range(300)][::3]
    pool.vote(slots, [3] * len(slots))
    mon = pool.forecast_monitor(GP._monitor_model(), max_out=128)
    assert pool.lib is dbg and mon.lib is dbg and mon.model.lib is dbg
    mon.drain().forecasts()
    mon.forecast_slots(slots).forecasts()
    off_d, sym_d, grp_d = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in ([0, 3], [0, 1, 2], [0]))
    out = torch.empty(4 * FORECAST_WORDS, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()

    def counts():
        a, w = C.c_int64(), C.c_int64()
        assert dbg.prego_debug_alloc_count(C.byref(a), C.byref(w)) == 0
        return a.value, w.value
    n0 = counts()
    rep, rb, grp = _p(mon.feed._dev[0]), mon.feed._report_bytes, _p(mon._groups)
    assert dbg.prego_stream_pool_feed_drain(mon.feed.f, rep, rb, None) == 0
    assert dbg.prego_stream_pool_feed_judge(mon.feed.f, mon.model.m, rep, rb, grp, _p(mon._dev[0]), mon._dev[0].numel() * 4, None) == 0
    assert dbg.prego_stream_pool_feed_forecast(mon.feed.f, mon.model.m, rep, rb, grp, _p(mon._fdev[0]), mon._fdev[0].numel() * 4, None) == 0
    assert dbg.prego_stream_pool_forecast(pool.p, mon.model.m, _p(mon._slots_dev[0]), 100, grp, _p(mon._sdev[0]), mon._sdev[0].numel() * 4, None) == 0
    assert dbg.prego_procedure_forecast(mon.model.m, 1, 3, _p(off_d), _p(sym_d), _p(grp_d), _p(out), 4 * 96, None) == 0
    assert counts() == n0
    torch.cuda.synchronize()
