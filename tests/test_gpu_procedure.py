"""The procedure model on the device (prego_procedure_*, prego_stream_pool_feed_judge, `pool.mistake_monitor`; csrc/procedure.hip).  Every
comparison is of integers and exact, word for word, against the host model (prego_amd/procedure.py: ProcedureModel.judge; for the
monitor prego_amd/stream_pool.py: MonitorModel over one OnlineRecord per slot fed the same ids):
  1. the offline judge over n_classes {1, 12, 86, 128} x order {1, 2, 8}: 15 groups whose example counts sit on the wave edges (1, 63,
     64, 65), at the Assembly101-O corpus's size (1105) and at ~5000, an empty group, a group outside the corpus, group -1, ids outside
     the classes, sequences of every length 1..40;  2. one-group corpora of those sizes;  3. the golden Assembly101-O counts;
  4. the monitor on a StreamPool of 300 slots (two workgroups of the drain) with a max_out that leaves entries pending, overflow
     entries, a closed and reopened slot, set_group between two drains;  5. the monitor on a TransformerStreamPool;  6. refusals."""
import ctypes as C
import json
import os
import random

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import _lib                                            # noqa: E402
from prego_amd._lib import PregoError                                 # noqa: E402
from prego_amd.aggregate import OVERFLOW_BAD_ID, OVERFLOW_FULL, OnlineRecord   # noqa: E402
from prego_amd.procedure import JUDGED, SKIPPED_VERDICT, UNKNOWN, VERDICT_WORDS, ProcedureModel, Verdict   # noqa: E402
from prego_amd.stream_pool import MonitorModel, StreamPool            # noqa: E402
from tests import test_gpu_step_wide as TW                            # noqa: E402  the engines are built once and shared

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EWORKSPACE = -1, -3
EDGE_SIZES = (1, 63, 64, 65, 1105, 5000)                              # examples in a group: the wave's edges, the real corpus, many trips


def _group_transcripts(rng, ncls, n_examples):
    """transcripts with exactly n_examples symbols: variations of one base procedure, so that long contexts do repeat"""
    base = [rng.randrange(ncls) for _ in range(rng.randint(4, 14))]
    out, left = [], n_examples
    while left > 0:
        t = [s if rng.random() < 0.8 else rng.randrange(ncls) for s in base[rng.randrange(3):]]
        if rng.random() < 0.3 and len(t) > 2:
            i = rng.randrange(len(t) - 1)
            t[i], t[i + 1] = t[i + 1], t[i]
        t = t[:left]
        out.append(t)
        left -= len(t)
    return out, base


def _corpus(rng, ncls, sizes, **kw):
    """group g has sizes[g] examples (0: the group is empty); the transcripts come in shuffled order, the device sorts them"""
    m, bases, pairs = ProcedureModel(ncls, **kw), {}, []
    for g, n in enumerate(sizes):
        ts, bases[g] = _group_transcripts(rng, ncls, n)
        pairs += [(t, g) for t in ts]
    rng.shuffle(pairs)
    for t, g in pairs:
        m.add(t, g)
    return m, bases


def _queries(rng, ncls, bases, groups):
    """sequences of every length 1..40, mostly walks along a base procedure, with foreign steps and ids outside the classes"""
    seqs, grps = [], []
    for n in range(1, 41):
        g = groups[n % len(groups)]
        base = bases.get(g if g in bases else rng.choice(sorted(bases)))
        s = [base[(i + n) % len(base)] if rng.random() < 0.75 else rng.randrange(ncls) for i in range(n)]
        if n % 9 == 0:
            s[rng.randrange(n)] = rng.choice((ncls, 128, 255, -1, 1 << 20))
        seqs.append(s)
        grps.append(g)
    return seqs, grps


def _same_as_host(m, seqs, grps):
    got = m.to(DEV).judge_sequences(seqs, grps)
    want = m.judge_sequences(seqs, grps)
    for s, (a, b) in enumerate(zip(got, want)):
        assert [v.words() for v in a] == [v.words() for v in b], (s, grps[s], seqs[s])
    return [v for vs in got for v in vs]


# ---- 1. the offline judge --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,threshold", [(1, (1, 12)), (2, (0, 1)), (8, (1, 3))])
@pytest.mark.parametrize("ncls", [1, 12, 86, 128])
def test_offline_judge_equals_the_host_model(ncls, order, threshold):
    rng = random.Random(1000 * ncls + order)
    sizes = list(EDGE_SIZES) + [0, 7, 130, 2, 64, 129, 3, 300, 0]          # 15 groups, two of them empty
    m, bases = _corpus(rng, ncls, sizes, order=order, threshold=threshold)
    assert m.n_groups == 14 and m.n_examples == sum(sizes)                # the trailing empty group is a group the corpus does not have
    seqs, grps = _queries(rng, ncls, bases, list(range(15)) + [-1, -1, 6, 40, -2])
    vs = _same_as_host(m, seqs, grps)
    assert len(vs) == 820 and all(v.flags & JUDGED for v in vs)
    empty = [v for s, g in zip(seqs, grps) if g in (6, 14, 40, -2) for v in m.judge_sequences([s], [g])[0]]
    assert empty and all(v.words() == [JUDGED | UNKNOWN, 0, 0, v.group, 0, 0, 0, 0] for v in empty)
    if ncls > 1:
        assert {v.jstar for v in vs} >= set(range(min(order, 3) + 1)), "the queries did not reach every back-off level"
        assert any(v.mistake for v in vs) and any(not v.mistake and not v.unknown for v in vs)


# ---- 2. one group ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_examples", EDGE_SIZES)
def test_one_group_of_every_edge_size(n_examples):
    rng = random.Random(n_examples)
    m, bases = _corpus(rng, 12, [n_examples], order=2, threshold=(1, 5))
    seqs, grps = _queries(rng, 12, bases, [0, -1])
    vs = _same_as_host(m, seqs, grps)
    assert max(v.tot for v in vs) <= n_examples and any(v.tot for v in vs)


def test_an_empty_corpus_knows_nothing():
    m = ProcedureModel(12)
    vs = _same_as_host(m, [[1, 2, 3], [4]], [-1, 0])
    assert [v.words() for v in vs] == [[JUDGED | UNKNOWN, 0, 0, g, 0, 0, 0, 0] for g in (-1, -1, -1, 0)]
    assert m.to(DEV).judge_sequences([], []) == []


# ---- 3. Assembly101-O ----------------------------------------------------------------------------------------------------------------------------
def test_assembly101o_on_the_device():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "procedure_assembly101o.json")))
    m = ProcedureModel(golden["n_classes"], order=2)
    for t in golden["transcripts"]:
        m.add(t["symbols"], t["group"])
    seqs, grps = [s["pred"] for s in golden["sequences"]], [s["group"] for s in golden["sequences"]]
    dev = m.to(DEV)
    judged = dev.judge_sequences(seqs, grps)
    assert [[v.words() for v in vs] for vs in judged] == [[v.words() for v in vs] for vs in m.judge_sequences(seqs, grps)]
    r = m.mistake_metrics(seqs, judged=judged)
    assert (r["tp"], r["fp"], r["fn"], r["tn"]) == (111, 242, 71, 219)


# ---- 4. the monitor on a StreamPool -----------------------------------------------------------------------------------------------------------------
NCLS = 86


def _monitor_model():
    rng = random.Random(5)
    m, _ = _corpus(rng, 6, [40, 25, 60], order=3, threshold=(1, 4))      # steps 0..5 of the pool's 86 classes, three groups
    wide = ProcedureModel(NCLS, order=3, threshold=(1, 4))
    for g, seq, _ in m.transcripts:
        wide.add(seq, g)
    return wide


def _vote(pool, records, votes):
    slots = list(votes)
    pool.vote(slots, [votes[s] for s in slots])
    for s, i in votes.items():
        records[s].push(i)


def _drain_same(mon, mirror):
    t, want = mon.drain(), mirror.drain()
    got = {"count": t.count, "pending": t.pending, "seq": t.seq, "entries": t.events()}
    assert got == {k: want[k] for k in got}, (got, want)
    assert [v.words() for v in t.verdicts()] == [v.words() for v in want["verdicts"]], want["entries"]
    assert len(t.verdicts()) == len(t.events()) == t.count
    return want


def test_monitor_verdicts_equal_the_host_models_under_churn():
    e = TW._real_engine("bf16", 3)
    cap, max_out = 300, 5                                                     # up to 9 entries are due per tick
    pool = StreamPool(e, capacity=cap, window=1, max_events=6)
    model = _monitor_model()
    mon = pool.mistake_monitor(model, max_out=max_out, depth=2)
    records = [OnlineRecord(1, NCLS, 6) for _ in range(cap)]
    mirror = MonitorModel(records, model, max_out)
    for _ in range(cap):
        pool.open()
    rng = random.Random(11)
    live = [0, 1, 63, 64, 255, 256, 257, 299]                                 # both workgroups of the drain, both sides of their boundary
    mon.set_group(live[:6], [0, 1, 2, 0, 1, 2])
    mirror.set_group(live[:6], [0, 1, 2, 0, 1, 2])                            # 257 and 299 stay at -1: every group
    seen, n_pending = [], 0
    for tick in range(9):
        _vote(pool, records, {s: rng.randrange(6) for s in live if rng.random() < 0.8})
        if tick == 3:
            _vote(pool, records, {1: NCLS})                                   # an id outside the classes: an overflow entry, once
        while True:
            r = _drain_same(mon, mirror)
            seen += list(zip(r["entries"], r["verdicts"]))
            n_pending += r["pending"] > 0
            if not r["pending"]:
                break
    assert n_pending >= 3, "max_out never left entries pending"
    skipped = [(en, v) for en, v in seen if v.skipped]
    assert {en[2] for en, _ in skipped} == {OVERFLOW_BAD_ID, OVERFLOW_FULL} and all(en[1] == -1 and v == SKIPPED_VERDICT for en, v in skipped)
    judged = [v for _, v in seen if not v.skipped]
    assert len(judged) >= 30 and {v.group for v in judged} == {-1, 0, 1, 2}
    assert any(v.mistake for v in judged) and any(v.jstar == 2 for v in judged) and any(not v.mistake and not v.unknown for v in judged)
    assert mon.groups() == mirror.groups


def test_a_reopened_slot_starts_again_and_set_group_holds_from_the_next_drain():
    e = TW._real_engine("bf16", 3)
    pool = StreamPool(e, capacity=300, window=1, max_events=16)
    model = _monitor_model()
    mon = pool.mistake_monitor(model, max_out=16, depth=2)
    records = [OnlineRecord(1, NCLS, 16) for _ in range(300)]
    mirror = MonitorModel(records, model, 16)
    slots = [pool.open() for _ in range(260)]
    a, b = slots[2], slots[258]
    ga, seq, _ = next(t for t in model.transcripts if len(t[1]) >= 5 and all(x != y for x, y in zip(t[1][:4], t[1][1:5])))
    mon.set_group([a], [ga])
    mirror.set_group([a], [ga])
    for i in seq[:3]:
        _vote(pool, records, {a: i, b: i})
    r = _drain_same(mon, mirror)
    assert [v.group for v in r["verdicts"]] == [ga] * 3 + [-1] * 3
    assert [v.jstar for v in r["verdicts"]] == [1, 2, 3] * 2 and all(v.cnt >= 1 for v in r["verdicts"])      # the corpus's own transcript
    # close and reopen: the history and the group start again
    pool.close(a)
    records[a] = OnlineRecord(1, NCLS, 16)
    mirror.forget([a])
    assert mon.groups()[a] == -1 and pool.open() == a
    _vote(pool, records, {a: seq[3], b: seq[3]})
    r = _drain_same(mon, mirror)
    va, vb = r["verdicts"]
    assert r["entries"][0][:2] == (a, 0) and va.words() == model.judge([], seq[3], -1).words() and va.jstar <= 1
    assert r["entries"][1][:2] == (b, 3) and vb.words() == model.judge(seq[:3], seq[3], -1).words()
    # set_group between two drains that are both in flight: the first still judges b against every group
    nxt = seq[4 % len(seq)]
    _vote(pool, records, {b: nxt})
    t1 = mon.drain()
    mon.set_group([b], [2 - ga])
    nxt2 = (nxt + 1) % 6
    _vote(pool, records, {b: nxt2})
    t2 = mon.drain()
    with pytest.raises(PregoError, match="all 2 report buffers hold unread tickets"):
        mon.drain()
    assert t1.events() == [(b, 4, nxt, 4)] and t2.events() == [(b, 5, nxt2, 5)]
    h = seq[:3] + [seq[3]]
    assert [v.words() for v in t1.verdicts()] == [model.judge(h, nxt, -1).words()]
    assert [v.words() for v in t2.verdicts()] == [model.judge(h + [nxt], nxt2, 2 - ga).words()]
    assert t2.verdicts()[0].group == 2 - ga
    with pytest.raises(PregoError, match="slot 299 is not open"):
        mon.set_group([299], [0])
    with pytest.raises(PregoError, match="each >= -1"):
        mon.set_group([a], [-2])


# ---- 5. the monitor on a TransformerStreamPool ------------------------------------------------------------------------------------------------------
def test_monitor_on_a_transformer_pool():
    from tests import test_gpu_vit_stream_pool as VT
    m = VT._model()
    pool = m.stream_pool(capacity=8, vote_window=2, max_events=64)
    ncls = pool._ncls
    rng = random.Random(2)
    model = ProcedureModel(ncls, order=2, threshold=(1, 20))
    for k in range(400):                                                      # ~3000 examples over the classes: most single steps are known
        model.add([rng.randrange(ncls) for _ in range(rng.randint(4, 10))], k % 3)
    mon = pool.mistake_monitor(model, max_out=64)
    records = [OnlineRecord(2, ncls, 64) for _ in range(8)]
    mirror = MonitorModel(records, model, 64)
    slots = [pool.open() for _ in range(5)][::-1][:3]                        # 4, 3, 2
    mon.set_group(slots[:2], [1, 2])
    mirror.set_group(slots[:2], [1, 2])
    vids = [(torch.from_numpy(r).to(DEV), torch.from_numpy(f).to(DEV)) for r, f in VT._videos()]
    n = 0
    for t in range(0, 16, 4):
        rgb = torch.cat([v[0][t:t + 4] for v in vids]).contiguous()
        flow = torch.cat([v[1][t:t + 4] for v in vids]).contiguous()
        _, argmax = pool.push_bursts(slots, 4, rgb, flow)
        for i, s in enumerate(slots):
            records[s].push_frames(argmax[4 * i:4 * i + 4].tolist())
        n += _drain_same(mon, mirror)["count"]
    assert n >= 3 and all(pool.events(s)["frames"] == 16 for s in slots)


# ---- 6. refusals write nothing ------------------------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _i32(*v):
    return (C.c_int32 * len(v))(*v)


def test_refusals_and_what_a_judge_leaves_untouched():
    e = TW._real_engine("bf16", 3)
    lib = e.lib
    err = lambda: lib.prego_last_error().decode()
    # -- create
    groups, offsets, symbols = _i32(0, 1), (C.c_int64 * 3)(0, 3, 5), _i32(0, 1, 2, 3, 4)
    need = lib.prego_procedure_model_bytes(2, 2, 5, 5)
    assert need % 256 == 0 and need >= 12 + 20 + 7 and lib.prego_procedure_model_bytes(-1, 2, 5, 5) == 0
    assert lib.prego_procedure_model_bytes(2, 2, 5, 6) == 0 and lib.prego_procedure_model_bytes(2, 2, 1 << 30, 5) == 0
    assert lib.prego_procedure_model_bytes(2, 2, 1 << 25, (1 << 24) + 1) == 0
    block = torch.full((need + 512,), 0x6B, dtype=torch.uint8, device=DEV)
    m = C.c_void_p()

    def create(out=C.byref(m), ncls=5, order=2, num=0, den=1, n=2, g=groups, off=offsets, sym=symbols, blk=_p(block), nb=need):
        return lib.prego_procedure_model_create(out, ncls, order, num, den, n, g, off, sym, None, blk, nb, None)
    for kw, rc, msg in ((dict(out=None), EINVAL, "out is NULL"), (dict(order=0), EINVAL, "order 0 (1..8)"), (dict(order=9), EINVAL, "order 9 (1..8)"),
                        (dict(ncls=0), EINVAL, "n_classes 0"), (dict(ncls=129), EINVAL, "n_classes 129"),
                        (dict(ncls=4), EINVAL, "symbols[4] = 4 is outside [0, 4)"), (dict(sym=_i32(0, -1, 2, 3, 4)), EINVAL, "symbols[1] = -1"),
                        (dict(num=2, den=1), EINVAL, "threshold 2/1"), (dict(den=32769), EINVAL, "threshold 0/32769"),
                        (dict(g=_i32(0, -1)), EINVAL, "groups[1] = -1"), (dict(g=None), EINVAL, "groups is NULL"),
                        (dict(off=None), EINVAL, "offsets is NULL"), (dict(off=(C.c_int64 * 3)(0, 3, 2)), EINVAL, "offsets[2] = 2 is below"),
                        (dict(sym=None), EINVAL, "symbols is NULL"), (dict(blk=None), EINVAL, "block is NULL"),
                        (dict(blk=C.c_void_p(block.data_ptr() + 16)), EINVAL, "256-byte aligned"), (dict(nb=need - 1), EWORKSPACE, f"need {need}")):
        assert create(**kw) == rc and msg in err() and not m.value, (kw, err())
    torch.cuda.synchronize()
    assert bool((block == 0x6B).all()), "a refused create wrote the block"
    assert create() == 0 and m.value
    torch.cuda.synchronize()
    assert bool((block[need:] == 0x6B).all()) and block[:12].view(torch.int32).cpu().tolist() == [0, 3, 5]      # goff: where each group's examples begin

    # -- the offline judge
    off_d = torch.tensor([0, 2, 3], dtype=torch.int32, device=DEV)
    sym_d = torch.tensor([0, 1, 3], dtype=torch.int32, device=DEV)
    grp_d = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    out = torch.full((3 * VERDICT_WORDS + 64,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    snaps = [t.clone() for t in (block, out)]

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(t, s) for t, s in zip((block, out), snaps))

    def judge(mod=m, ns=2, npos=3, off=_p(off_d), sym=_p(sym_d), grp=_p(grp_d), o=_p(out), nb=3 * 32):
        return lib.prego_procedure_judge(mod, ns, npos, off, sym, grp, o, nb, None)
    for kw, rc, msg in ((dict(mod=None), EINVAL, "model is NULL"), (dict(off=None), EINVAL, "offsets is NULL"), (dict(sym=None), EINVAL, "symbols is NULL"),
                        (dict(grp=None), EINVAL, "groups is NULL"), (dict(o=None), EINVAL, "verdicts is NULL"), (dict(ns=0), EINVAL, "0 sequences"),
                        (dict(npos=0), EINVAL, "0 positions"), (dict(o=C.c_void_p(out.data_ptr() + 16)), EINVAL, "256-byte aligned"),
                        (dict(nb=3 * 32 - 32), EWORKSPACE, "3 positions need 96"), (dict(nb=0), EWORKSPACE, "need 96")):
        assert judge(**kw) == rc and msg in err(), (kw, err())
        assert untouched(), kw
    assert judge() == 0
    torch.cuda.synchronize()
    host = ProcedureModel(5).add([0, 1, 2], 0).add([3, 4], 1)
    want = [v.words() for vs in host.judge_sequences([[0, 1], [3]], [0, 1]) for v in vs]
    assert out[:24].view(3, 8).cpu().tolist() == want and bool((out[24:] == 0x5A5A5A5A).all()) and torch.equal(block, snaps[0])

    # -- the feed judge
    cap, max_out = 300, 8
    pool = StreamPool(e, capacity=cap, window=1, max_events=4)
    feed = pool.event_feed(max_out=max_out)
    s = pool.open()
    pool.vote([s], [0])
    rbytes = feed._report_bytes
    report = feed._dev[0]
    assert lib.prego_stream_pool_feed_drain(feed.f, _p(report), rbytes, None) == 0
    grp = torch.full((cap,), -1, dtype=torch.int32, device=DEV)
    out = torch.full((max_out * VERDICT_WORDS + 64,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    snaps = [t.clone() for t in (pool._block, feed._block, report, grp, out)]

    def untouched_feed():
        torch.cuda.synchronize()
        return all(torch.equal(t, sn) for t, sn in zip((pool._block, feed._block, report, grp, out), snaps))

    def fjudge(fn=lib.prego_stream_pool_feed_judge, f=feed.f, mod=m, rep=_p(report), rb=rbytes, g=_p(grp), o=_p(out), nb=max_out * 32):
        return fn(f, mod, rep, rb, g, o, nb, None)
    for fn, who in ((lib.prego_stream_pool_feed_judge, "stream_pool_feed_judge"), (lib.prego_vit_stream_pool_feed_judge, "vit_stream_pool_feed_judge")):
        for kw, rc, msg in ((dict(f=None), EINVAL, "feed is NULL"), (dict(mod=None), EINVAL, "model is NULL"), (dict(rep=None), EINVAL, "report is NULL"),
                            (dict(rep=C.c_void_p(report.data_ptr() + 16)), EINVAL, "the report must be 256-byte aligned"),
                            (dict(rb=rbytes - 1), EWORKSPACE, f"need {rbytes}"), (dict(g=None), EINVAL, "slot_groups is NULL"),
                            (dict(o=None), EINVAL, "verdicts is NULL"), (dict(o=C.c_void_p(out.data_ptr() + 32)), EINVAL, "the verdicts must be 256-byte aligned"),
                            (dict(nb=max_out * 32 - 32), EWORKSPACE, f"{max_out} entries need {max_out * 32}")):
            assert fjudge(fn=fn, **kw) == rc and msg in err() and err().startswith(who), (kw, err())
            assert untouched_feed(), kw
    assert fjudge() == 0
    torch.cuda.synchronize()
    assert out[:8].cpu().tolist() == host.judge([], 0, -1).words()
    assert bool((out[8:] == 0x5A5A5A5A).all()), "written behind verdict `count`"
    assert all(torch.equal(t, sn) for t, sn in zip((pool._block, feed._block, report, grp), snaps[:4])), "the judge wrote what it only reads"
    lib.prego_procedure_model_destroy(m)


def test_judging_allocates_nothing_and_waits_for_nothing():
    dbg = _lib.load_debug()
    e = TW._real_engine("bf16", 8, lib=dbg)
    pool = StreamPool(e, capacity=300, window=1)
    assert pool.lib is dbg
    slots = [pool.open() for _ in range(300)][::3]
    pool.vote(slots, [3] * len(slots))
    model = _monitor_model()
    mon = pool.mistake_monitor(model, max_out=128)
    assert mon.lib is dbg and mon.model.lib is dbg
    mon.drain().events()
    off_d, sym_d, grp_d = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in ([0, 3], [0, 1, 2], [0]))
    out = torch.empty(24, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()

    def counts():
        a, w = C.c_int64(), C.c_int64()
        assert dbg.prego_debug_alloc_count(C.byref(a), C.byref(w)) == 0
        return a.value, w.value
    n0 = counts()
    assert dbg.prego_stream_pool_feed_drain(mon.feed.f, _p(mon.feed._dev[0]), mon.feed._report_bytes, None) == 0
    assert dbg.prego_stream_pool_feed_judge(mon.feed.f, mon.model.m, _p(mon.feed._dev[0]), mon.feed._report_bytes, _p(mon._groups), _p(mon._dev[0]),
                                            mon._dev[0].numel() * 4, None) == 0
    assert dbg.prego_procedure_judge(mon.model.m, 1, 3, _p(off_d), _p(sym_d), _p(grp_d), _p(out), 96, None) == 0
    assert counts() == n0
    torch.cuda.synchronize()
