"""GPU: Viterbi decoding on the device (prego_viterbi_decode, prego_viterbi_decode_costs, prego_emission_costs; csrc/decode.hip) word
for word against the host model (prego_amd/decode.py, which tests/test_decode_cpu.py holds to hand-computed paths and to the brute
force over all paths): the hand cases, random video sets in both input modes, ties, the accumulator width, the quantiser, `Evaluate`
under cfg['eval_decode'], every refusal, and the allocation / host-wait counters of the debug library."""
import ctypes as C
import json
import logging
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from prego_amd import _lib                                                     # noqa: E402
from prego_amd._lib import DECODE_BLOCK, DECODE_PREFETCH, PregoError           # noqa: E402
from prego_amd.decode import (DECODE_CAP, emission_costs, emission_costs_device, path_cost, uniform_transitions, viterbi_decode,      # noqa: E402
                              viterbi_decode_device)
from prego_amd.segmental import segmental_scores                               # noqa: E402
from tests.helpers.decode_cases import HAND_CASES, random_costs, random_lengths, random_model, random_probs      # noqa: E402

DEV = "cuda:0"


def _to_device(videos, C_, pad=0, misalign=False):
    """the videos' rows one after the other as a device matrix [n, C] with a row stride of C + pad words (the pad columns hold words
    that would change every result if they were read) and, with misalign, a first word 4 bytes behind a 16-byte boundary"""
    flat = np.concatenate([np.asarray(v).reshape(-1, C_) for v in videos], 0) if videos else np.zeros((0, C_), np.int32)
    n, ld = flat.shape[0], C_ + pad
    wide = np.full((n, ld), -3 if flat.dtype.kind == "i" else 0.999, flat.dtype)
    wide[:, :C_] = flat
    buf = torch.from_numpy(np.concatenate((np.zeros(1, flat.dtype), wide.reshape(-1)))).to(DEV)
    assert buf.data_ptr() % 16 == 0
    body = buf[1:] if misalign else buf[1:].clone()
    x = body.view(n, ld)[:, :C_]
    assert n == 0 or (x.data_ptr() % 16 == 4) == misalign
    off = np.concatenate(([0], np.cumsum([len(v) for v in videos]))).astype(np.int32)
    return x, torch.from_numpy(off).to(DEV)


def _oracle(videos, trans, init):
    labs, recs = [], []
    for v in videos:
        lab, rec = viterbi_decode(v, trans, init)
        labs.append(lab)
        recs.append(rec)
    return (torch.from_numpy(np.concatenate(labs).astype(np.int32)) if labs else torch.zeros(0, dtype=torch.int32),
            torch.tensor(recs, dtype=torch.int64).reshape(-1, 2))


def _check(videos, C_, trans, init, costs, pad=0, misalign=False):
    """labels and records of the device equal the oracle's; every feasible path, recomputed on the host, costs what its record says"""
    x, off = _to_device(videos, C_, pad, misalign)
    labels, records = viterbi_decode_device(x, off, trans, init, costs=costs)
    want_l, want_r = _oracle(videos, trans, init)
    got_l, got_r = labels.cpu(), records.cpu()
    assert got_l.dtype == torch.int32 and got_r.dtype == torch.int64 and got_r.shape == want_r.shape
    if not torch.equal(got_r, want_r):
        bad = (got_r != want_r).any(1).nonzero().flatten().tolist()
        raise AssertionError(f"records of videos {bad[:5]} of {len(videos)}: device {got_r[bad[:5]].tolist()} host {want_r[bad[:5]].tolist()}")
    if not torch.equal(got_l, want_l):
        bad = (got_l != want_l).nonzero().flatten().tolist()
        raise AssertionError(f"{len(bad)} labels differ, first at frames {bad[:5]}: device {got_l[bad[:5]].tolist()} host {want_l[bad[:5]].tolist()}")
    o = 0
    for v, rec in zip(videos, got_r.tolist()):
        lab = got_l[o:o + len(v)].numpy()
        o += len(v)
        if rec[1] >= 0:
            assert path_cost(v, trans, init, lab) == rec[0] and lab[-1] == rec[1]
        else:
            assert (lab == -1).all()
    return got_l, got_r


@pytest.mark.parametrize("costs_mode", [True, False])
def test_hand_cases(costs_mode):
    for name, case in sorted(HAND_CASES.items()):
        C_ = case["C"]
        v = np.asarray(case["costs"], np.int32).reshape(-1, C_)
        if not costs_mode:
            if name == "clamped_words":
                continue                                          # cost words out of range: the costs entry's
            v = np.exp2(-v.astype(np.float64) / 256.0).astype(np.float32)
            if not np.array_equal(emission_costs(v), np.clip(np.asarray(case["costs"]).reshape(-1, C_), 0, DECODE_CAP)):
                continue                                          # this case's costs are no images of the quantiser
        x, off = _to_device([v], C_)
        labels, records = viterbi_decode_device(x, off, np.asarray(case["trans"]), case["init"], costs=costs_mode)
        assert labels.cpu().tolist() == case["labels"] and tuple(records.cpu()[0].tolist()) == case["record"], name


# C: 1, 2, 12, 86, 128 (every slice length of the kernel); V: 300 is more than one workgroup per CU, 1100 more than the grid (it strides)
RANDOM_SETS = [
    # C, V, max_len, density, init given, out-of-range words, row pad, misaligned
    (1, 3, 140, 0.0, False, False, 0, False), (1, 64, 300, 0.5, True, True, 3, True),
    (2, 1, 5000, 0.0, True, False, 1, True), (2, 300, 140, 0.5, False, True, 0, False), (2, 1100, 40, 0.95, True, False, 2, False),
    (12, 3, 5000, 0.0, False, True, 4, False), (12, 64, 300, 0.95, True, False, 0, True), (12, 1100, 40, 0.5, False, False, 1, False),
    (86, 1, 5000, 0.5, True, False, 10, False), (86, 64, 300, 0.0, False, True, 0, True), (86, 300, 140, 0.95, True, False, 2, False),
    (128, 3, 5000, 0.95, False, False, 0, False), (128, 64, 300, 0.5, True, True, 5, True), (128, 300, 140, 0.0, True, False, 0, False)]


def _random_set(C_, V, max_len, density, given_init, oor, costs_mode):
    rng = np.random.default_rng(C_ * 100000 + V * 10 + int(costs_mode))
    trans, init = random_model(rng, C_, density, given_init, oor)
    lens = [max_len] + random_lengths(rng, V - 1, min(max_len, 300)) if max_len == 5000 else random_lengths(rng, V, max_len)
    videos = [random_costs(rng, T, C_, oor) if costs_mode else random_probs(rng, T, C_) for T in lens]
    return videos, trans, init


@pytest.mark.parametrize("costs_mode", [True, False])
@pytest.mark.parametrize("C_,V,max_len,density,given_init,oor,pad,misalign", RANDOM_SETS)
def test_random_sets(C_, V, max_len, density, given_init, oor, pad, misalign, costs_mode):
    videos, trans, init = _random_set(C_, V, max_len, density, given_init, oor, costs_mode)
    _, rec = _check(videos, C_, trans, init, costs_mode, pad, misalign)
    if density >= 0.95 and C_ > 1 and V >= 64:
        assert (rec[:, 1] < 0).any()                             # many videos have no allowed path at all


def test_ties_take_the_lowest_index():
    # constant emissions, constant transitions: every path costs the same; the lowest predecessor at every step, the lowest end state
    for C_ in (2, 12, 86, 128):
        lens = [1, 2, DECODE_PREFETCH, DECODE_BLOCK + 1, 3 * DECODE_BLOCK + 5]
        videos = [np.full((T, C_), 9, np.int32) for T in lens]
        lab, rec = _check(videos, C_, np.full((C_, C_), 4, np.int32), None, True)
        assert not lab.any() and rec.tolist() == [[9 * T + 4 * (T - 1), 0] for T in lens]
    # duplicated columns: class k of 86 is a copy of class k % 5 in the emissions and in the model
    rng = np.random.default_rng(4)
    base_t, _ = random_model(rng, 5, 0.3, False)
    idx = np.arange(86) % 5
    trans = base_t[np.ix_(idx, idx)]
    videos = [random_costs(rng, T, 5)[:, idx] for T in (700, 64, 65)]
    lab, _ = _check(videos, 86, trans, None, True)
    assert int(lab.max()) < 5
    lab, _ = _check([np.exp2(-v / 256.0).astype(np.float32) for v in videos], 86, trans, None, False)
    assert int(lab.max()) < 5


def test_accumulator_passes_2_to_the_31():
    """T = 70000, C = 2, only self-loops, emissions CAP on state 0 and CAP - 1 on state 1: exactly 70000 * 32766 = 2 293 620 000 on
    state 1 (past 2^31), the two states 70000 apart at the end."""
    T = 70000
    costs = np.tile(np.array([[DECODE_CAP, DECODE_CAP - 1]], np.int32), (T, 1))
    x, off = _to_device([costs], 2)
    labels, records = viterbi_decode_device(x, off, np.array([[0, -1], [-1, 0]], np.int32), None, costs=True)
    assert records.cpu().tolist() == [[T * 32766, 1]] and T * 32766 > 2 ** 31
    assert bool((labels == 1).all())


def test_a_state_far_above_the_minimum_is_not_saturated():
    """T = 40000, C = 3, only self-loops: whatever state a path starts in it stays in.  For the first 19999 frames state 0 costs
    nothing and state 2 costs CAP per frame, so 2 climbs to 19999 CAP = 655 307 233 above the step's minimum - past the spread the
    kernel's 32-bit relative keys hold (2^24 - 64 * 65534) from frame 385 on, so from there the stretches run on the exact 64-bit keys
    with state 2 as a FAR value.  Then the emissions reverse for the remaining 20001 frames: state 0 pays CAP, state 2 nothing, and
    the path through state 2 ends cheapest, 19999 CAP against 20001 CAP (state 1 pays CAP throughout: 40000 CAP).  The result IS the
    value that was far: a kernel that saturated it (say at minimum + 2^24) would report another cost or another end state."""
    T, F, half = 40000, -1, 19999
    costs = np.empty((T, 3), np.int32)
    costs[:half] = (0, DECODE_CAP, DECODE_CAP)
    costs[half:] = (DECODE_CAP, DECODE_CAP, 0)
    trans = np.array([[0, F, F], [F, 0, F], [F, F, 0]], np.int32)
    short = costs[half - 300:half + 200]                     # state 0 wins here: 200 CAP against 300 CAP, never far
    lab, rec = _check([costs, short], 3, trans, None, True)
    assert rec.tolist() == [[half * DECODE_CAP, 2], [200 * DECODE_CAP, 0]]
    assert bool((lab[:T] == 2).all()) and bool((lab[T:] == 0).all())
    # the same through the probabilities entry: p = 1 costs 0, p = 0 costs CAP
    lab, rec = _check([(costs == 0).astype(np.float32)], 3, trans, None, False)
    assert rec.tolist() == [[half * DECODE_CAP, 2]] and bool((lab == 2).all())
    # three frames in which two states die: 0 may only go to 1 and 1 nowhere, so 2 is the only state with an allowed continuation
    dying = np.array([[F, 0, F], [F, F, F], [F, F, DECODE_CAP]], np.int32)
    flat = np.tile(np.array([[0, 0, DECODE_CAP]], np.int32), (3, 1))
    lab, rec = _check([flat, flat[:2]], 3, dying, None, True)
    assert rec.tolist() == [[5 * DECODE_CAP, 2], [0, 1]] and lab.tolist() == [2, 2, 2, 0, 1]


def _two_components(rng, T, turn, first_far=29000, then_far=29000):
    """costs [T, 12]: classes 6..11 pay `first_far` more per frame before frame `turn`, classes 0..5 `then_far` more from it on"""
    x = random_costs(rng, T, 12)
    x[:turn, 6:] += first_far
    x[turn:, :6] += then_far
    return x


def test_a_far_component_that_wins_in_the_end():
    """C = 12, two components that never mix (block-diagonal random transitions).  The second pays 29000 more per frame at first, so
    it runs away from the step's minimum by 2^24 in under 600 frames and the stretches go over to the exact 64-bit keys with its six
    states as far values; then the first component pays 29000 more per frame for a longer time, the spread closes again (back to 32-bit
    keys) and the path through the SECOND component ends cheapest.  Labels and records must be the oracle's: they are values that were
    far, carried through 64-bit stretches and through both changes of width.  Short videos beside them never leave 32 bits."""
    rng = np.random.default_rng(21)
    trans, _ = random_model(rng, 12, 0.2, False)
    trans[:6, 6:] = -1
    trans[6:, :6] = -1
    plan = [(3000, 1400), (2900, 1363), (300, 140), (2 * DECODE_BLOCK + 1, 60), (1500, 700)]
    videos = [_two_components(rng, T, turn) for T, turn in plan]
    _, rec = _check(videos, 12, trans, None, True)
    assert (rec[:, 1] >= 6).all()                             # every video ends in the component that was far
    assert int(rec[0, 0]) > 1400 * 29000 > 2 ** 24
    # without the reversal the cheap component wins and the far one only has to do no harm, whichever width a stretch runs in
    videos = [_two_components(rng, T, T) for T, _ in plan]
    _, rec = _check(videos, 12, trans, None, True)
    assert (rec[:, 1] < 6).all() and (rec[:, 1] >= 0).all()
    # only the far component may start: its exact costs are the result (the cheap one is infinite, so nothing is far any more)
    _, rec = _check(videos, 12, trans, np.array([-1] * 6 + [0] * 6, np.int32), True)
    assert (rec[:, 1] >= 6).all() and int(rec[0, 0]) > 3000 * 29000
    # a state that dies and a video that becomes infeasible in the middle of a long run: state 0 may only stay, 1 may go nowhere
    dead_end = np.array([[0, 5], [-1, -1]], np.int32)
    _check([random_costs(rng, T, 2) for T in (700, 2, 1)], 2, dead_end, np.array([-1, 0], np.int32), True)


def test_quantiser_on_the_device():
    rng = np.random.default_rng(11)
    w = rng.integers(0, 2 ** 32, 1 << 20, dtype=np.uint64).astype(np.uint32)                    # every class of word: both signs, NaNs, denormals
    special = np.array([0, 0x80000000, 1, 0x007FFFFF, 0x00800000, 0x3F800000, 0x3F7FFFFF, 0x3F000000, 0x7F800000, 0xFF800000, 0x7FC00000,
                        0x7F800001, 0xFFFFFFFF, 0x3FC00000, 0x00808000], np.uint32)
    w[:special.size] = special
    w[special.size:300000] &= 0x3FFFFFFF                                                          # and many ordinary words below 2.0
    p = w.view(np.float32).reshape(-1, 64)
    want = torch.from_numpy(emission_costs(p))
    got = emission_costs_device(torch.from_numpy(p).to(DEV))
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), want)
    wide = torch.from_numpy(np.concatenate((p, np.full((p.shape[0], 3), 0.5, np.float32)), 1)).to(DEV)      # ld > n_classes
    assert torch.equal(emission_costs_device(wide[:, :64]).cpu(), want)
    assert int(want.max()) == DECODE_CAP and int(want.min()) == 0


def test_probabilities_and_device_made_costs_decode_alike():
    rng = np.random.default_rng(12)
    trans, init = random_model(rng, 86, 0.3, True)
    lens = [0, 900, 1, DECODE_BLOCK, 2000]
    videos = [random_probs(rng, T, 86) for T in lens]
    x, off = _to_device(videos, 86, pad=2)
    la, ra = viterbi_decode_device(x, off, trans, init)
    lb, rb = viterbi_decode_device(emission_costs_device(x), off, trans, init, costs=True)
    assert torch.equal(la, lb) and torch.equal(ra, rb) and bool((ra[1:, 1] >= 0).any())


def test_defer_offsets_and_argument_checks():
    rng = np.random.default_rng(13)
    costs = random_costs(rng, 1000, 12)
    trans = uniform_transitions(12, 700)
    x, _ = _to_device([costs], 12)
    # offsets words outside [0, n_frames] are clamped before they index memory; a descending pair is an empty video
    off = torch.tensor([-5, 400, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    fn = viterbi_decode_device(x, off, trans, None, costs=True, defer=True)
    assert callable(fn)
    lab, rec = fn()
    (l0, r0), (l1, r1) = viterbi_decode(costs[:400], trans), viterbi_decode(costs[400:], trans)
    assert np.array_equal(lab, np.concatenate((l0, l1))) and rec.tolist() == [list(r0), list(r1)]
    off = torch.tensor([300, 200, 1000, -2 ** 31], dtype=torch.int32, device=DEV)        # empty, [200, 1000), empty
    lab, rec = viterbi_decode_device(x, off, trans, None, costs=True)
    l1, r1 = viterbi_decode(costs[200:], trans)
    assert rec.cpu().tolist() == [[0, -1], list(r1), [0, -1]] and np.array_equal(lab.cpu().numpy()[200:], l1)
    # no frames at all
    z = torch.zeros((0, 12), dtype=torch.int32, device=DEV)
    lab, rec = viterbi_decode_device(z, torch.zeros(4, dtype=torch.int32, device=DEV), trans, None, costs=True)
    assert lab.numel() == 0 and rec.cpu().tolist() == [[0, -1]] * 3
    with pytest.raises(PregoError, match="CUDA"):
        viterbi_decode_device(x.cpu(), off, trans)
    with pytest.raises(PregoError, match="float32"):
        viterbi_decode_device(x, off, trans)
    with pytest.raises(PregoError, match="classes"):
        viterbi_decode_device(torch.zeros((4, 129), device=DEV), off, np.zeros((129, 129), np.int32))


def _p(t):
    return C.c_void_p(t.data_ptr())


def test_every_refusal_leaves_the_outputs_untouched():
    lib = _lib.load()
    n, V, C_, ld = 700, 3, 12, 16
    EINVAL, EWORKSPACE = -1, -3                                     # PREGO_EINVAL, PREGO_EWORKSPACE
    rng = np.random.default_rng(14)
    host = random_probs(rng, n, ld)
    probs = torch.from_numpy(host).to(DEV)
    costs = torch.from_numpy(emission_costs(host)).to(DEV)
    off = torch.tensor([0, 100, 100, n], dtype=torch.int32, device=DEV)
    trans = torch.from_numpy(uniform_transitions(C_, 600)).to(DEV)
    init = torch.zeros(C_, dtype=torch.int32, device=DEV)
    need = lib.prego_viterbi_workspace_bytes(n, V, C_)
    assert need >= n * C_ and lib.prego_viterbi_workspace_bytes(0, V, C_) == 0 and lib.prego_viterbi_workspace_bytes(n, V, 129) == 0
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=DEV)
    labels = torch.full((n + 4,), -77, dtype=torch.int32, device=DEV)
    rec = torch.full((V * 2 + 2,), -77, dtype=torch.int64, device=DEV)
    assert rec.data_ptr() % 16 == 0

    def ptr(t):
        return C.c_void_p(t) if isinstance(t, int) else (_p(t) if t is not None else None)

    def call(entry=lib.prego_viterbi_decode, src=probs, ld_=ld, off_=off, V_=V, n_=n, C__=C_, trans_=trans, init_=init, labels_=labels,
             rec_=rec, ws_=ws, ws_bytes=need):
        return entry(ptr(src), ld_, ptr(off_), V_, n_, C__, ptr(trans_), ptr(init_), ptr(labels_), ptr(rec_), ptr(ws_), ws_bytes, None)
    for entry, src in ((lib.prego_viterbi_decode, probs), (lib.prego_viterbi_decode_costs, costs)):
        e = dict(entry=entry, src=src)
        refused = [call(entry=entry, src=None), call(off_=None, **e), call(trans_=None, **e), call(labels_=None, **e), call(rec_=None, **e),
                   call(ws_=None, **e), call(V_=0, **e), call(V_=-3, **e), call(n_=-1, **e), call(n_=2 ** 31, **e), call(C__=0, **e),
                   call(C__=129, **e), call(ld_=C_ - 1, **e), call(rec_=rec.data_ptr() + 8, **e),
                   # an output that overlaps an input: labels in the scores, records in trans, the workspace over the offsets, labels in init
                   call(labels_=src.data_ptr() + 64, **e), call(rec_=trans.data_ptr(), **e), call(ws_=off.data_ptr(), **e),
                   call(labels_=init.data_ptr(), n_=4, off_=off, **e)]
        assert refused == [EINVAL] * len(refused), refused
        assert b"viterbi_decode" in lib.prego_last_error()
        short = call(ws_bytes=need - 1, **e)
        assert short == EWORKSPACE and b"prego_viterbi_workspace_bytes" in lib.prego_last_error()
    ec = torch.full((n * C_ + 2,), -77, dtype=torch.int32, device=DEV)
    refused = [lib.prego_emission_costs(None, ld, n, C_, _p(ec), None), lib.prego_emission_costs(_p(probs), ld, n, C_, None, None),
               lib.prego_emission_costs(_p(probs), ld, -1, C_, _p(ec), None), lib.prego_emission_costs(_p(probs), ld, n, 0, _p(ec), None),
               lib.prego_emission_costs(_p(probs), C_ - 1, n, C_, _p(ec), None),
               lib.prego_emission_costs(_p(probs), ld, n, C_, C.c_void_p(probs.data_ptr() + 16), None)]
    assert refused == [EINVAL] * len(refused) and b"emission_costs" in lib.prego_last_error()
    torch.cuda.synchronize()
    assert bool((labels == -77).all()) and bool((rec == -77).all()) and bool((ws == 0x5A).all()) and bool((ec == -77).all())
    assert bool((init == 0).all()) and torch.equal(trans.cpu(), torch.from_numpy(uniform_transitions(C_, 600)))
    # and the same arguments unrefused run, both entries alike, inside their outputs
    videos = [host[:100, :C_], host[:0, :C_], host[100:, :C_]]
    want_l, want_r = _oracle(videos, uniform_transitions(C_, 600), None)
    for entry, src in ((lib.prego_viterbi_decode, probs), (lib.prego_viterbi_decode_costs, costs)):
        labels.fill_(-77)
        rec.fill_(-77)
        assert call(entry=entry, src=src) == 0
        torch.cuda.synchronize()
        assert torch.equal(labels[:n].cpu(), want_l) and torch.equal(rec[:V * 2].cpu().reshape(V, 2), want_r)
        assert bool((labels[n:] == -77).all()) and bool((rec[V * 2:] == -77).all())
    assert lib.prego_emission_costs(_p(probs), ld, n, C_, _p(ec), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(ec[:n * C_].cpu().reshape(n, C_), costs[:, :C_].cpu()) and bool((ec[n * C_:] == -77).all())
    assert call(n_=0, ws_=None, ws_bytes=0) == 0                     # no frames: legal without a workspace
    torch.cuda.synchronize()
    assert rec[:V * 2].cpu().tolist() == [0, -1] * V and bool((rec[V * 2:] == -77).all())


def test_no_allocation_and_no_host_wait_in_the_entries():
    dbg = _lib.load_debug()
    rng = np.random.default_rng(15)
    lens = [2000, 0, 300, 64, 1]
    videos = [random_probs(rng, T, 86) for T in lens]
    trans, init = random_model(rng, 86, 0.2, True)
    x, off = _to_device(videos, 86)
    x = x.contiguous()
    n = x.shape[0]
    td, idv = torch.from_numpy(trans).to(DEV), torch.from_numpy(init).to(DEV)
    ws = torch.empty(dbg.prego_viterbi_workspace_bytes(n, len(lens), 86), dtype=torch.uint8, device=DEV)
    labels = torch.empty(n, dtype=torch.int32, device=DEV)
    rec = torch.empty((len(lens), 2), dtype=torch.int64, device=DEV)
    ec = torch.empty((n, 86), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()

    def counts():
        a, w = C.c_int64(), C.c_int64()
        assert dbg.prego_debug_alloc_count(C.byref(a), C.byref(w)) == 0
        return a.value, w.value
    n0 = counts()
    assert dbg.prego_emission_costs(_p(x), 86, n, 86, _p(ec), None) == 0
    assert dbg.prego_viterbi_decode(_p(x), 86, _p(off), len(lens), n, 86, _p(td), _p(idv), _p(labels), _p(rec), _p(ws), ws.numel(), None) == 0
    assert counts() == n0
    torch.cuda.synchronize()
    want_l, want_r = _oracle(videos, trans, init)
    assert torch.equal(labels.cpu(), want_l) and torch.equal(rec.cpu(), want_r)
    assert dbg.prego_viterbi_decode_costs(_p(ec), 86, _p(off), len(lens), n, 86, _p(td), _p(idv), _p(labels), _p(rec), _p(ws), ws.numel(), None) == 0
    assert counts() == n0
    torch.cuda.synchronize()
    assert torch.equal(labels.cpu(), want_l) and torch.equal(rec.cpu(), want_r)


# ---- Evaluate ----
def _eval_items(lens, multi=False):
    from prego_amd import weights as W
    items = []
    for i, T in enumerate(lens):
        rgb = torch.from_numpy(W.tsn_features((T, 2048), 21, f"dec.rgb.{i}"))[None].pin_memory()
        tgt = torch.zeros(1, T, 12)
        tgt[0, torch.arange(T), (torch.arange(T) // 41 + i) % 12] = 1
        if multi and i == 2:
            tgt[0, 100:200, 7] = 1
        items.append((rgb, torch.zeros(1, 1, 2048).expand(1, T, 2048), tgt.pin_memory(), (f"v{i}",), torch.tensor([0]), torch.tensor([T])))
    return items


def _run_eval(tmp_path, tag, **over):
    from prego_amd import weights as W
    from prego_amd.config import epic_tent_cfg
    from prego_amd.registry import build_eval, build_model
    import prego_amd.evaluate, prego_amd.model  # noqa: F401
    vl = os.path.join(tmp_path, "video_list.json")
    json.dump({"EPIC-TENT-O": {"class_index": [f"c{i}" for i in range(12)]}}, open(vl, "w"))
    out_dir = tmp_path / tag
    cfg = epic_tent_cfg(eval="dummy.pth", video_list_path=vl, compute_dtype="fp16", eval_output_dir=str(out_dir), **over)
    model = build_model(cfg, DEV)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.miniroad_state_dict(cfg, 20, head_gain=8.0).items()})
    return build_eval(cfg), model, out_dir


class _Lines(logging.Handler):
    def __init__(self):
        super().__init__()
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def test_evaluate_decode(tmp_path, monkeypatch):
    lens = [900, 1, 2500, 333, 64]
    items = _eval_items(lens)
    log = logging.getLogger("t.decode")
    log.setLevel(logging.INFO)
    h = _Lines()
    log.addHandler(h)
    # the scores of the pass, downloaded where Evaluate hands them to the decoder
    import prego_amd.evaluate as E
    seen = []

    def spy(scores, offsets, trans, init=None, **kw):
        seen.append((scores.cpu().numpy(), offsets.cpu().tolist()))
        return viterbi_decode_device(scores, offsets, trans, init, **kw)
    monkeypatch.setattr(E, "viterbi_decode_device", spy)
    ev, model, out_dir = _run_eval(tmp_path, "on", eval_decode=True, eval_segmental=True, eval_decode_switch_cost=1500)
    mAP = ev(model, items, log, DEV)
    js = json.load(open(out_dir / "output_miniROAD.json"))
    (all_scores, cuts), = seen
    assert cuts == np.concatenate(([0], np.cumsum(lens))).tolist() and all_scores.shape == (sum(lens), 12)
    same = all_scores.argmax(1) == np.concatenate([js[f"v{i}"]["pred"] for i in range(len(lens))])
    assert same.mean() > 0.999                                       # they ARE the pass's scores (up to an exact tie between two classes)
    Gt = [js[f"v{i}"]["gt"] for i in range(len(lens))]
    trans = uniform_transitions(12, 1500)
    want = [viterbi_decode(all_scores[cuts[i]:cuts[i + 1]], trans) for i in range(len(lens))]
    dec = ev.last_decode
    assert list(dec["labels"]) == [f"v{i}" for i in range(len(lens))]
    for i, (lab, rec) in enumerate(want):
        got = dec["labels"][f"v{i}"]
        assert got.dtype == torch.int32 and torch.equal(got, torch.from_numpy(lab)), i
    assert torch.equal(dec["records"], torch.tensor([list(r) for _l, r in want], dtype=torch.int64))
    assert dec["segmental"] == segmental_scores([l for l, _r in want], Gt)
    assert sum("decoded (switch 1500, stay 0)" in ln for ln in h.lines) == 5          # MoF, Edit, three F1: one new line each
    # the transitions given: the same matrix, the same decode
    ev2, model2, _ = _run_eval(tmp_path, "given", eval_decode=True, eval_decode_transitions=(trans, None))
    ev2(model2, items, log, DEV)
    assert all(torch.equal(ev2.last_decode["labels"][k], v) for k, v in dec["labels"].items())
    # the key off: no decode, and nothing else about the pass differs
    h.lines.clear()
    ev0, model0, out0 = _run_eval(tmp_path, "off", eval_segmental=True)
    mAP0 = ev0(model0, items, log, DEV)
    log.removeHandler(h)
    assert getattr(ev0, "last_decode", None) is None and not any("decoded" in ln for ln in h.lines)
    assert mAP0 == mAP and json.load(open(out0 / "output_miniROAD.json")) == js and ev0.last_segmental == ev.last_segmental
    assert [p for p, _ in ev0.phase_log] == [p for p, _ in ev.phase_log if p != "decode_done"]


def test_evaluate_decode_refusals(tmp_path, monkeypatch):
    log = logging.getLogger("t")
    items = _eval_items([300, 40, 500], multi=True)
    ev, model, _ = _run_eval(tmp_path, "dense", eval_decode=True)
    with pytest.raises(PregoError, match="eval_decode.*one class id per frame"):
        ev(model, items, log, DEV)
    ev.all_class_names = [f"c{i}" for i in range(129)]
    with pytest.raises(PregoError, match="eval_decode.*129 classes"):
        ev(model, items, log, DEV)
    ev, model, _ = _run_eval(tmp_path, "vit", eval_decode=True)
    ev.cfg["model"] = "Transformer"
    with pytest.raises(PregoError, match="eval_decode.*raw logits"):
        ev(model, items, log, DEV)
    ev, model, _ = _run_eval(tmp_path, "ranks", eval_decode=True)
    import prego_amd.evaluate as E
    for name, val in (("is_available", True), ("is_initialized", True), ("get_world_size", 2), ("get_rank", 0)):
        monkeypatch.setattr(E.dist, name, lambda *a, _v=val, **k: _v)
    with pytest.raises(PregoError, match="eval_decode.*2 ranks"):
        ev(model, items, log, DEV)
