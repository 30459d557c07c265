"""GPU: the decode pool (prego_decode_pool_*, csrc/decode_pool.hip; `stream_pool.DecodePool`) word for word against its host model
(`decode.OnlineDecoder`, which tests/test_decode_pool_cpu.py holds to the offline `viterbi_decode`): every class-count instantiation and
lag, the edge lengths, the same stream fed as single frames, bursts of 32 and ragged counts, padded and misaligned rows, both input modes,
ties, permuted slots, a full pool, dead streams, push after flush, the far-state stream, the event feed and both monitors on the decoded
transcript, `online_decode_device`, every refusal, and the allocation / host-wait counters of the debug library."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import _lib                                                     # noqa: E402
from prego_amd._lib import PregoError                                          # noqa: E402
from prego_amd.aggregate import OVERFLOW_BAD_ID, OnlineRecord                  # noqa: E402
from prego_amd.decode import (DECODE_CAP, DECODE_PENDING, OnlineDecoder, emission_costs_device, online_decode_device,      # noqa: E402
                              uniform_transitions, viterbi_decode_device)
from prego_amd.procedure import ProcedureModel                                 # noqa: E402
from prego_amd.stream_pool import DecodePool, FeedModel, MonitorModel          # noqa: E402
from tests.helpers.decode_cases import random_costs, random_model, random_probs      # noqa: E402
from tests.helpers.decode_pool_cases import cuts, dying_stream, far_state_stream, run_host      # noqa: E402

DEV = "cuda:0"
EINVAL = -1
_p = lambda t: C.c_void_p(t.data_ptr())


def _rows(rows, pad=0, misalign=False):
    """rows [R, C] as a device matrix with a row stride of C + pad words - the pad words would change every result if they were read -
    and, with misalign, a first word 4 bytes behind a 16-byte boundary"""
    R, C_ = rows.shape
    wide = np.full((R, C_ + pad), -3 if rows.dtype.kind == "i" else 0.999, rows.dtype)
    wide[:, :C_] = rows
    buf = torch.from_numpy(np.concatenate((np.zeros(1, rows.dtype), wide.reshape(-1)))).to(DEV)
    body = buf[1:] if misalign else buf[1:].clone()
    x = body.view(R, C_ + pad)[:, :C_]
    assert (x.data_ptr() % 16 == 4) == misalign
    return x


def _rec_words(pool, slot):
    ptr, nb = C.c_void_p(), C.c_size_t()
    assert pool.lib.prego_decode_pool_record(pool.p, slot, C.byref(ptr), C.byref(nb)) == 0
    off = ptr.value - pool._block.data_ptr()
    return pool._block[off:off + nb.value].view(torch.int32).cpu().tolist()


def _drive(pool, feeds, pad=0, misalign=False, shuffle=None, flush=True):
    """feeds: [(slot, x [T, C], counts)]: every tick each slot takes its next count of frames, packed into calls of at most 256 rows;
    nothing is read back before the end.  Returns {slot: (committed labels, now)} after checking the layout of every output: the first
    m words of a slot's block are labels, the rest DECODE_PENDING, commit = (frames committed before, m)."""
    costs = feeds[0][1].dtype.kind == "i"
    at = {s: [0, 0] for s, _, _ in feeds}                     # next count, next frame
    calls = []
    while True:
        due = [(s, x, c) for s, x, c in feeds if at[s][0] < len(c)]
        if not due:
            break
        if shuffle is not None:
            shuffle.shuffle(due)
        call, rows = [], 0
        for s, x, c in due:
            k = c[at[s][0]]
            if len(call) == 256 or rows + k > 256:
                break
            call.append((s, x[at[s][1]:at[s][1] + k]))
            at[s][0] += 1
            at[s][1] += k
            rows += k
        out = pool.push([s for s, _ in call], _rows(np.concatenate([r for _, r in call]), pad, misalign), counts=[len(r) for _, r in call],
                        costs=costs)
        calls.append(([(s, len(r)) for s, r in call], out))
    tails = []
    if flush:
        slots = [s for s, _, _ in feeds]
        for a in range(0, len(slots), 256):
            tails.append((slots[a:a + 256], pool.flush(slots[a:a + 256])))
    got = {s: ([], []) for s, _, _ in feeds}
    for layout, (labels, commit, now) in calls:
        labels, commit, now, o = labels.cpu().tolist(), commit.cpu().tolist(), now.cpu().tolist(), 0
        for i, (s, k) in enumerate(layout):
            first, m = commit[i]
            assert first == len(got[s][0]) and 0 <= m <= k and labels[o + m:o + k] == [DECODE_PENDING] * (k - m), (s, commit[i])
            got[s][0].extend(labels[o:o + m])
            got[s][1].extend(now[o:o + k])
            o += k
    for slots, (labels, commit) in tails:
        labels, commit = labels.cpu().tolist(), commit.cpu().tolist()
        for i, s in enumerate(slots):
            first, m = commit[i]
            assert first == len(got[s][0]) and labels[i][m:] == [DECODE_PENDING] * (pool.lag - m)
            got[s][0].extend(labels[i][:m])
    return got


def _same_as_host(pool, got, slot, x, trans, init, lag, window=1, max_events=1024):
    dec, labels, now = run_host(x, trans, init, lag, [len(x)] if len(x) else [], vote_window=window, max_events=max_events)
    assert got[slot][0] == labels.tolist(), (slot, len(x))
    assert got[slot][1] == now.tolist(), (slot, len(x))
    assert np.array_equal(pool.state_words(slot), dec.state_words()), (slot, len(x), pool.state_words(slot)[:8], dec.state_words()[:8])
    assert _rec_words(pool, slot) == dec.record.to_words(pool._ncls, pool.max_events), (slot, len(x))
    return dec


def _lengths(lag):
    return sorted({0, 1, 2, max(lag - 1, 0), lag, lag + 1, lag + 31, lag + 32, lag + 33, 600})


# every lag with the class counts in turn (all five instantiations of the step), every class count at a lag beside a burst
SHAPES = [(0, 12), (1, 86), (2, 128), (31, 1), (32, 2), (33, 12), (64, 86), (256, 128), (33, 1), (33, 2), (33, 86), (33, 128), (64, 3)]


@pytest.mark.parametrize("lag,C_", SHAPES)
def test_single_frames_bursts_and_ragged_counts_agree_with_the_host_model(lag, C_):
    rng = np.random.default_rng(100 * lag + C_)
    costs = (lag + C_) % 2 == 0
    trans, init = random_model(rng, C_, 0.3 if C_ > 2 else 0.0, given_init=lag % 2 == 0, out_of_range=True)
    streams = [random_costs(rng, T, C_, out_of_range=True) if costs else random_probs(rng, T, C_) for T in _lengths(lag)]
    pool = DecodePool(C_, trans, init, lag=lag, capacity=3 * len(streams), device=DEV)
    feeds = []
    for x in streams:
        for kind in ("single", "burst", "ragged"):
            feeds.append((pool.open(), x, cuts(len(x), kind, rng)))
    got = _drive(pool, feeds, pad=3 if costs else 0, misalign=not costs)
    differ = 0
    for k, x in enumerate(streams):
        dec = _same_as_host(pool, got, feeds[3 * k][0], x, trans, init, lag)
        ref = pool.state_words(feeds[3 * k][0])
        for s, _, _ in feeds[3 * k + 1:3 * k + 3]:             # header, keys and record word for word across the three feedings
            assert got[s] == got[feeds[3 * k][0]] and np.array_equal(pool.state_words(s), ref)
            assert _rec_words(pool, s) == _rec_words(pool, feeds[3 * k][0])
        st = pool.status(feeds[3 * k][0])
        assert (st["frames"], st["committed"], st["flushed"], st["cost"], st["end"]) == (len(x), len(x), True, dec.cost, dec.end)


def test_misaligned_padded_rows_in_both_modes_and_device_made_costs():
    rng = np.random.default_rng(3)
    C_, lag = 86, 16
    trans, init = random_model(rng, C_, 0.2, True)
    probs = random_probs(rng, 150, C_)
    pool = DecodePool(C_, trans, init, lag=lag, capacity=4, device=DEV)
    a, b, c, d = (pool.open() for _ in range(4))
    got = _drive(pool, [(a, probs, cuts(150, "ragged", rng))], pad=5, misalign=True)
    _same_as_host(pool, got, a, probs, trans, init, lag)
    costs = emission_costs_device(torch.from_numpy(probs).to(DEV)).cpu().numpy()
    got_c = _drive(pool, [(b, costs, cuts(150, "burst"))], pad=2, misalign=True)
    got_p = _drive(pool, [(c, probs, cuts(150, "burst"))])
    assert got_c[b] == got_p[c] == got[a] and np.array_equal(pool.state_words(b), pool.state_words(a))
    # [n, K, C] and [n, C] scores, as StreamPool.push_frames / push return them
    x3 = torch.from_numpy(probs[:64].reshape(1, 64, C_)[:, :32]).to(DEV)
    lab, com, now = pool.push([d], x3)
    lab1, com1, now1 = pool.push([d], torch.from_numpy(probs[32:33]).to(DEV))
    dec = OnlineDecoder(trans, init, lag=lag)
    hl, hn = dec.push(probs[:33])
    assert lab.shape == (32,) and com.cpu().tolist() == [[0, 16]] and com1.cpu().tolist() == [[16, 1]]
    assert lab[:16].cpu().tolist() + lab1.cpu().tolist() == hl.tolist() and now.cpu().tolist() + now1.cpu().tolist() == hn.tolist()


def test_ties_take_the_lowest_state():
    C_, lag = 12, 5
    x = np.full((100, C_), 7, np.int32)
    trans = np.full((C_, C_), 3, np.int64)
    pool = DecodePool(C_, trans, None, lag=lag, capacity=2, device=DEV)
    a, b = pool.open(), pool.open()
    got = _drive(pool, [(a, x, cuts(100, "burst")), (b, x, cuts(100, "single"))])
    _same_as_host(pool, got, a, x, trans, None, lag)
    assert got[a] == got[b] and set(got[a][0]) == {0} and set(got[a][1]) == {0}


def test_slots_permuted_within_a_call_and_other_slots_do_not_matter():
    rng = np.random.default_rng(8)
    C_, lag = 12, 9
    trans, init = random_model(rng, C_, 0.3, True)
    streams = [random_costs(rng, int(T), C_) for T in rng.integers(40, 120, 12)]
    pool = DecodePool(C_, trans, init, lag=lag, capacity=40, device=DEV)
    slots = [pool.open(s) for s in (39, 3, 17, 0, 25, 8, 31, 12, 5, 38, 20, 1)]
    feeds = [(s, x, cuts(len(x), "ragged", rng)) for s, x in zip(slots, streams)]
    got = _drive(pool, feeds, shuffle=rng)
    for s, x in zip(slots, streams):
        _same_as_host(pool, got, s, x, trans, init, lag)


def test_a_full_pool_of_256_slots_of_different_lengths_with_a_vote_window():
    rng = np.random.default_rng(9)
    C_, lag = 12, 8
    trans, init = random_model(rng, C_, 0.1, False)
    pool = DecodePool(C_, trans, init, lag=lag, capacity=256, vote_window=3, max_events=8, device=DEV)
    streams = [random_probs(rng, s % 41, C_) for s in range(256)]
    feeds = [(pool.open(), x, cuts(len(x), "burst")) for x in streams]
    got = _drive(pool, feeds)
    full = 0
    for (s, x, _) in feeds:
        dec = run_host(x, trans, init, lag, [len(x)] if len(x) else [], vote_window=3, max_events=8)[0]
        assert got[s][0] == run_host(x, trans, init, lag, [len(x)] if len(x) else [])[1].tolist()
        assert np.array_equal(pool.state_words(s), dec.state_words()) and _rec_words(pool, s) == dec.record.to_words(C_, 8)
        full += dec.record.overflow & 1
    assert full > 0, "no record filled up"


def test_a_stream_that_dies_in_mid_burst_and_close_names_it():
    x, trans, init = dying_stream()
    pool = DecodePool(3, trans, init, lag=2, capacity=2, device=DEV)
    a, b = pool.open(), pool.open()
    got = _drive(pool, [(a, x, [8]), (b, x[:3], [3])], flush=False)
    assert got[a] == ([0, -1, -1, -1, -1, -1], [0, 1, 2, -1, -1, -1, -1, -1]) and got[b] == ([0], [0, 1, 2])
    st = pool.status(a)
    assert st["dead"] and st["cost"] == -1 and st["end"] == -1 and st["frames"] == 8 and st["committed"] == 6 and not pool.status(b)["dead"]
    dec = OnlineDecoder(trans, init, lag=2)
    dec.push(x)
    assert np.array_equal(pool.state_words(a), dec.state_words()) and _rec_words(pool, a) == dec.record.to_words()
    assert dec.record.overflow & OVERFLOW_BAD_ID
    with pytest.raises(PregoError, match="infeasible"):
        pool.events(a)
    with pytest.raises(PregoError, match="infeasible"):
        pool.close(a)
    assert pool.free == 1
    out = pool.close(b)                                      # alive: the tail comes from the last frame's chain
    assert out == {"pred": [0, 1, 2], "changes_pred": [1, 2, 3], "labels_tail": [1, 2], "cost": 21}
    # a chain 0 -> 1 -> .. -> 11 that cannot stay: whatever the costs, frame 12 has no finite state; the cuts put it anywhere in a burst
    rng = np.random.default_rng(12)
    trans = np.full((12, 12), -1, np.int64)
    trans[np.arange(11), np.arange(1, 12)] = rng.integers(0, 4000, 11)
    init = rng.integers(0, 4000, 12)
    streams = [random_costs(rng, 70, 12) for _ in range(8)]
    pool = DecodePool(12, trans, init, lag=4, capacity=8, device=DEV)
    feeds = [(pool.open(), x, cuts(70, "ragged" if k else "burst", rng)) for k, x in enumerate(streams)]
    got = _drive(pool, feeds)
    decs = [_same_as_host(pool, got, s, x, trans, init, 4) for s, x, _ in feeds]
    assert all(d.dead and d.record.frames == 8 for d in decs) and all(got[s][1][11] == 11 and got[s][1][12] == -1 for s in got)


def test_push_after_flush_close_and_reopen():
    rng = np.random.default_rng(13)
    C_, lag = 12, 6
    trans, init = random_model(rng, C_, 0.0, True)
    x = random_costs(rng, 50, C_)
    pool = DecodePool(C_, trans, init, lag=lag, capacity=3, device=DEV)
    a = pool.open()
    got = _drive(pool, [(a, x[:40], [20, 20])])
    dec = _same_as_host(pool, got, a, x[:40], trans, init, lag)
    before, rec = pool.state_words(a), _rec_words(pool, a)
    lab, com, now = pool.push([a], torch.from_numpy(x[40:43]).to(DEV), counts=[3], costs=True)
    assert lab.cpu().tolist() == [DECODE_PENDING] * 3 == now.cpu().tolist() and com.cpu().tolist() == [[40, 0]]
    dec.push(x[40:43])
    after = pool.state_words(a)
    assert after[2] == before[2] | 4 and np.array_equal(after, dec.state_words()) and _rec_words(pool, a) == rec
    assert pool.status(a)["pushed_after_flush"] and pool.flush([a])[1].cpu().tolist() == [[40, 0]]
    out = pool.close(a)
    assert out["pred"] == dec.record.event_id and out["changes_pred"] == dec.record.event_start[1:] + [40] and out["cost"] == dec.cost
    assert out["labels_tail"] == []                          # the flush before it had committed the tail
    assert pool.open() == a and not pool.state_words(a).any() and not any(_rec_words(pool, a))
    got = _drive(pool, [(a, x, cuts(50, "ragged", rng))], flush=False)      # the reopened slot is a fresh stream
    dec = OnlineDecoder(trans, init, lag=lag)
    hl, hn = dec.push(x)
    assert got[a] == (hl.tolist(), hn.tolist()) and np.array_equal(pool.state_words(a), dec.state_words())
    out = pool.close(a)
    assert out["labels_tail"] == dec.flush().tolist() and len(out["labels_tail"]) == lag and out["cost"] == dec.cost
    for call in (pool.snapshot, lambda: pool.detach([0]), lambda: pool.restore(None)):
        with pytest.raises(PregoError, match="slot images of decode pools are not supported yet"):
            call()


def test_far_state_stream_runs_on_the_exact_keys():
    x, trans, init = far_state_stream()
    pool = DecodePool(3, trans, init, lag=64, capacity=2, device=DEV)
    a = pool.open()
    got = _drive(pool, [(a, x, cuts(1300, "burst"))], flush=False)
    keys = pool.state_words(a)[8:].view(np.int64)[:3]
    assert (keys >> 7).tolist() == [22_936_900, 22_939_900, 19_660_200] and (keys & 127).tolist() == [0, 1, 2]
    tail = pool.flush([a])[0].cpu().tolist()[0]
    labels = got[a][0] + tail
    assert len(labels) == 1300 and set(labels[:1136]) == {0} and set(labels[1136:]) == {2}
    dec, want, now = run_host(x, trans, init, 64, [1300])
    assert labels == want.tolist() and got[a][1] == now.tolist() and np.array_equal(pool.state_words(a), dec.state_words())
    b = pool.open()                                          # and at the frame of the largest spread
    _drive(pool, [(b, x[:600], cuts(600, "burst"))], flush=False)
    keys = pool.state_words(b)[8:].view(np.int64)[:3] >> 7
    assert keys.tolist() == [0, 3000, 600 * DECODE_CAP] and int(keys.max() - keys.min()) == 19_660_200 >= 1 << 24


def _monitor_setup(max_out=64):
    rng = np.random.default_rng(21)
    C_, lag, cap = 5, 3, 6
    trans = uniform_transitions(C_, 400)
    pool = DecodePool(C_, trans, None, lag=lag, capacity=cap, max_events=128, device=DEV)
    decs = [OnlineDecoder(trans, None, lag=lag, max_events=128) for _ in range(cap)]
    live = [pool.open(s) for s in (0, 2, 3, 5)]
    streams = {s: random_costs(rng, 96, C_) for s in live}
    return pool, decs, live, streams


def _tick(pool, decs, live, streams, t0, k):
    pool.push(live, torch.from_numpy(np.concatenate([streams[s][t0:t0 + k] for s in live])).to(DEV), counts=[k] * len(live), costs=True)
    for s in live:
        decs[s].push(streams[s][t0:t0 + k])


def test_event_feed_drains_equal_the_feed_model_over_the_host_records():
    pool, decs, live, streams = _monitor_setup()
    feed, model = pool.event_feed(max_out=7, depth=2), FeedModel([d.record for d in decs], max_out=7)
    n_entries = 0
    for t0 in range(0, 96, 16):
        _tick(pool, decs, live, streams, t0, 16)
        while True:
            t, want = feed.drain(), model.drain()
            assert (t.count, t.pending, t.seq, t.events()) == (want["count"], want["pending"], want["seq"], want["entries"])
            n_entries += t.count
            if not want["pending"]:
                break
    assert n_entries >= 12 and n_entries == sum(len(decs[s].record.event_id) for s in live)
    assert pool.events(live[0])["pred"] == decs[live[0]].record.event_id


def test_monitors_judge_and_forecast_the_decoded_transcript():
    pool, decs, live, streams = _monitor_setup()
    model = ProcedureModel(5, order=2).add([0, 1, 2, 3, 4], 0).add([0, 2, 1, 3], 0).add([4, 3, 2, 1, 0], 1).add([1, 1, 2], 1)
    mon, plain = pool.forecast_monitor(model, max_out=9), pool.mistake_monitor(model, max_out=9)
    mirror = MonitorModel([d.record for d in decs], model, max_out=9)
    for m in (mon, plain, mirror):
        m.set_group(live[:3], [0, 1, 0])
    n = 0
    for t0 in range(0, 96, 24):
        _tick(pool, decs, live, streams, t0, 24)
        while True:
            t, tp, want = mon.drain(), plain.drain(), mirror.drain()
            assert t.events() == want["entries"] == tp.events()
            assert [v.words() for v in t.verdicts()] == [v.words() for v in want["verdicts"]] == [v.words() for v in tp.verdicts()]
            assert [f.words() for f in t.forecasts()] == [mirror.forecast_entry(e).words() for e in want["entries"]]
            n += t.count
            if not want["pending"]:
                break
    assert n >= 12
    assert [f.words() for f in mon.forecast_slots(live).forecasts()] == [f.words() for f in mirror.forecast_slots(live)]
    other = ProcedureModel(6, order=2).add([0, 1, 5], 0)      # a model of another class count is refused before anything is launched
    with pytest.raises(PregoError, match="classes"):
        pool.mistake_monitor(other, max_out=9).drain()


def test_online_decode_device_equals_the_host_model_and_with_a_long_lag_the_offline_decode():
    rng = np.random.default_rng(30)
    C_ = 12
    trans, init = random_model(rng, C_, 0.1, True)
    trans = trans + 3000 * (1 - np.eye(C_, dtype=np.int32)) * (trans >= 0)      # sticky: what comes later changes a label
    lens = [0, 1, 50, 257, 300, 33]
    videos = [random_probs(rng, T, C_) for T in lens]
    scores = torch.from_numpy(np.concatenate(videos)).to(DEV)
    off = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    labels, records = online_decode_device(scores, off.tolist(), trans, init, lag=4)
    host = [run_host(v, trans, init, 4, [len(v)] if len(v) else []) for v in videos]
    assert labels.cpu().tolist() == np.concatenate([h[1] for h in host]).tolist()
    assert records.cpu().tolist() == [[h[0].cost, h[0].end] for h in host]
    offline_l, offline_r = viterbi_decode_device(scores, torch.from_numpy(off).to(DEV), trans, init)
    assert not torch.equal(labels, offline_l), "lag 4 shows on none of the videos"
    costs = emission_costs_device(scores)
    for src, mode in ((scores, False), (costs, True)):
        long_l, long_r = online_decode_device(src, torch.from_numpy(off), trans, init, lag=256, costs=mode)
        short = torch.tensor([T - 1 <= 256 for T in lens for _ in range(T)])
        assert torch.equal(long_l.cpu()[short], offline_l.cpu()[short]) and torch.equal(long_r, offline_r)
        assert torch.equal(long_l.cpu(), torch.from_numpy(np.concatenate([run_host(v, trans, init, 256, [len(v)] if len(v) else [])[1] for v in videos])))


def test_every_refusal_leaves_the_outputs_and_the_block_untouched():
    lib = _lib.load()
    C_, lag, cap = 12, 8, 4
    need = lib.prego_decode_pool_bytes(cap, C_, lag, 16)
    assert need > 0 and [lib.prego_decode_pool_bytes(*a) for a in ((0, C_, lag, 16), (cap, 0, lag, 16), (cap, 129, lag, 16), (cap, C_, -1, 16),
                                                                   (cap, C_, 257, 16), (cap, C_, lag, 0))] == [0] * 6
    assert lib.prego_decode_pool_bytes(1, 128, 256, 1) > 0
    trans = torch.from_numpy(uniform_transitions(C_, 500)).to(DEV)
    block = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device=DEV)
    assert block.data_ptr() % 256 == 0
    p = C.c_void_p()

    def create(cap_=cap, C__=C_, lag_=lag, win=1, mev=16, tr=trans, blk=block.data_ptr(), nb=need, out=p):
        return lib.prego_decode_pool_create(C.byref(out) if out is not None else None, cap_, C__, lag_, win, mev, _p(tr) if tr is not None else None,
                                            None, C.c_void_p(blk), nb, None)
    refused = [create(out=None), create(cap_=0), create(C__=0), create(C__=129), create(lag_=-1), create(lag_=257), create(win=0), create(mev=0),
               create(tr=None), create(blk=0), create(blk=block.data_ptr() + 16), create(nb=need - 1),
               create(tr=block[256:].view(torch.int32)[:C_ * C_])]
    assert refused == [EINVAL] * len(refused) and b"decode_pool_create" in lib.prego_last_error() and not p.value
    torch.cuda.synchronize()
    assert bool((block == 0x5A).all())
    assert create() == 0 and p.value
    rows = torch.from_numpy(random_costs(np.random.default_rng(1), 40, C_ + 2)).to(DEV)
    ld = C_ + 2
    labels, commit, now = (torch.full((n,), -77, dtype=torch.int32, device=DEV) for n in (64, 16, 64))
    torch.cuda.synchronize()
    before = block.clone()
    arr = lambda v: (C.c_int32 * len(v))(*v) if v is not None else None

    def push(entry=lib.prego_decode_pool_push_costs, pool=p, n=2, slots=(0, 3), counts=(8, 32), src=rows.data_ptr(), ld_=ld, lab=labels.data_ptr(),
             com=commit.data_ptr(), nw=now.data_ptr()):
        return entry(pool, n, arr(slots), arr(counts), C.c_void_p(src), ld_, C.c_void_p(lab), C.c_void_p(com), C.c_void_p(nw), None)
    for entry in (lib.prego_decode_pool_push, lib.prego_decode_pool_push_costs):
        refused = [push(entry, pool=None), push(entry, n=0), push(entry, n=5, slots=(0, 1, 2, 3, 0), counts=(1,) * 5), push(entry, slots=None),
                   push(entry, slots=(0, 4)), push(entry, slots=(-1, 0)), push(entry, slots=(3, 3)), push(entry, counts=None),
                   push(entry, counts=(0, 8)), push(entry, counts=(8, 33)), push(entry, counts=(8, -1)), push(entry, src=0), push(entry, ld_=C_ - 1),
                   push(entry, lab=rows.data_ptr() + 16), push(entry, nw=rows.data_ptr() + 4 * ld * 39), push(entry, com=block.data_ptr() + need - 8),
                   push(entry, lab=block.data_ptr()), push(entry, nw=labels.data_ptr() + 4 * 39), push(entry, com=now.data_ptr())]
        assert refused == [EINVAL] * len(refused), refused
        assert b"decode_pool_push" in lib.prego_last_error()
    big = torch.zeros((257, C_), dtype=torch.int32, device=DEV)
    lab9 = torch.full((300,), -77, dtype=torch.int32, device=DEV)
    assert lib.prego_decode_pool_push_costs(p, 4, arr((0, 1, 2, 3)), arr((32,) * 4), _p(big), C_, _p(lab9), None, None, None) == 0      # R = 128
    wide = DecodePool(C_, uniform_transitions(C_, 500), lag=lag, capacity=9, device=DEV)
    assert lib.prego_decode_pool_push_costs(wide.p, 9, arr(tuple(range(9))), arr((32,) * 8 + (1,)), _p(big), C_, _p(lab9), None, None, None) == EINVAL
    assert b"257 rows" in lib.prego_last_error()
    assert lib.prego_decode_pool_reset(p, 4, arr((0, 1, 2, 3)), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(block, before) and bool((lab9[128:] == -77).all())
    fl = torch.full((2 * lag + 8,), -77, dtype=torch.int32, device=DEV)
    refused = [lib.prego_decode_pool_flush(None, 1, arr((0,)), _p(fl), None, None), lib.prego_decode_pool_flush(p, 0, arr((0,)), _p(fl), None, None),
               lib.prego_decode_pool_flush(p, 2, arr((1, 1)), _p(fl), None, None), lib.prego_decode_pool_flush(p, 1, arr((4,)), _p(fl), None, None),
               lib.prego_decode_pool_flush(p, 2, arr((0, 1)), _p(fl), C.c_void_p(fl.data_ptr() + 4 * (2 * lag - 1)), None),
               lib.prego_decode_pool_flush(p, 1, arr((0,)), C.c_void_p(block.data_ptr() + 1024), None, None),
               lib.prego_decode_pool_reset(None, 1, arr((0,)), None), lib.prego_decode_pool_reset(p, 1, arr((7,)), None)]
    assert refused == [EINVAL] * len(refused)
    ptr, nb = C.c_void_p(), C.c_size_t()
    assert lib.prego_decode_pool_state(p, 4, C.byref(ptr), C.byref(nb)) == EINVAL and lib.prego_decode_pool_record(p, -1, C.byref(ptr), C.byref(nb)) == EINVAL
    assert lib.prego_decode_pool_state(p, 1, C.byref(ptr), C.byref(nb)) == 0 and nb.value == 32 + 8 * C_
    torch.cuda.synchronize()
    assert torch.equal(block, before) and bool((fl == -77).all())
    assert bool((labels == -77).all()) and bool((commit == -77).all()) and bool((now == -77).all()) and bool((block[need:] == 0x5A).all())
    # and the same arguments unrefused run inside their outputs, with nullable outputs left out
    assert push() == 0 and push(slots=(1, 2), lab=0, com=0, nw=0) == 0
    torch.cuda.synchronize()
    dec = [OnlineDecoder(uniform_transitions(C_, 500), lag=lag) for _ in range(2)]
    host = rows.cpu().numpy()[:, :C_]
    (l0, n0), (l1, n1) = dec[0].push(host[:8]), dec[1].push(host[8:40])
    assert labels[:40].cpu().tolist() == [DECODE_PENDING] * 8 + l1.tolist() + [DECODE_PENDING] * 8 and now[:40].cpu().tolist() == n0.tolist() + n1.tolist()
    assert commit[:4].cpu().tolist() == [0, 0, 0, 24] and bool((labels[40:] == -77).all()) and bool((commit[4:] == -77).all()) and bool((now[40:] == -77).all())
    assert bool((block[need:] == 0x5A).all())
    lib.prego_decode_pool_destroy(p)
    with pytest.raises(PregoError):
        DecodePool(C_, uniform_transitions(C_, 500), lag=300, device=DEV)
    pool = DecodePool(C_, uniform_transitions(C_, 500), lag=lag, capacity=2, device=DEV)
    s = pool.open()
    for bad in (lambda: pool.push([s], rows[:1, :C_]), lambda: pool.push([s], rows[:2, :C_].float(), counts=[3]), lambda: pool.push([1], rows[:1, :C_], costs=True),
                lambda: pool.push([s], rows[:1, :C_ - 1], costs=True), lambda: pool.push([s], rows[:1, :C_].cpu(), costs=True)):
        with pytest.raises(PregoError):
            bad()


def test_no_allocation_and_no_host_wait_in_push_and_flush():
    dbg = _lib.load_debug()
    C_, lag, cap = 86, 64, 8
    rng = np.random.default_rng(40)
    trans, init = random_model(rng, C_, 0.2, True)
    x = random_probs(rng, 8 * 32, C_)
    need = dbg.prego_decode_pool_bytes(cap, C_, lag, 64)
    block = torch.empty(need, dtype=torch.uint8, device=DEV)
    td, idv, rows = torch.from_numpy(trans).to(DEV), torch.from_numpy(init).to(DEV), torch.from_numpy(x).to(DEV)
    labels, commit, now = (torch.empty(n, dtype=torch.int32, device=DEV) for n in (256, 16, 256))
    tail = torch.empty(cap * lag, dtype=torch.int32, device=DEV)
    p = C.c_void_p()
    assert dbg.prego_decode_pool_create(C.byref(p), cap, C_, lag, 1, 64, _p(td), _p(idv), _p(block), need, None) == 0
    torch.cuda.synchronize()

    def counts():
        a, w = C.c_int64(), C.c_int64()
        assert dbg.prego_debug_alloc_count(C.byref(a), C.byref(w)) == 0
        return a.value, w.value
    n0 = counts()
    slots, k = (C.c_int32 * cap)(*range(cap)), (C.c_int32 * cap)(*([32] * cap))
    for _ in range(3):
        assert dbg.prego_decode_pool_push(p, cap, slots, k, _p(rows), C_, _p(labels), _p(commit), _p(now), None) == 0
    assert dbg.prego_decode_pool_flush(p, cap, slots, _p(tail), _p(commit), None) == 0
    assert counts() == n0
    torch.cuda.synchronize()
    dec = OnlineDecoder(trans, init, lag=lag)
    for _ in range(3):
        hl, hn = dec.push(x[:32])
    assert labels[:32].cpu().tolist() == hl.tolist() and now[:32].cpu().tolist() == hn.tolist() and tail[:lag].cpu().tolist() == dec.flush().tolist()
    dbg.prego_decode_pool_destroy(p)
