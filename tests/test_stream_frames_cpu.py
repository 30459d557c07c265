"""CPU side of the multi-frame streaming step (prego_miniroad_step_frames / _anticipation, prego_miniroad_step_pool_frames;
csrc/stream_frames.hip): the host model of the pool's K-frame commit - `OnlineRecord.push_frames`, `aggregate_online(bursts=...)`, which
tests/test_gpu_stream_pool_frames.py holds the device rule against - equals `aggregate()` whatever the burst sizes are; the automaton
reference driven in bursts with the state carried equals its frame-by-frame run, which is what tests/test_gpu_step_frames.py relies on when
it compares bursts against slices of ONE reference; and the entry points are declared and bound."""
import gzip
import json
import os
import random
import re

import pytest

torch = pytest.importorskip("torch")

from prego_amd.aggregate import OnlineRecord, aggregate, aggregate_online      # noqa: E402
from tests.helpers import gru_automaton as A                                   # noqa: E402
from tests.helpers import step_wide_cases as SW                                # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
_G8 = {}


def _g8():
    """the four shortest G8 videos' per-frame ids and what aggregate() makes of them, computed once"""
    if not _G8:
        with gzip.open(os.path.join(G, "g8_output_miniROAD.json.gz"), "rt") as f:
            data = json.load(f)
        for vid in sorted(data, key=lambda k: len(data[k]["pred"]))[:4]:
            ids = data[vid]["pred"]
            a = aggregate({"v": {"pred": ids, "gt": [0] * len(ids)}})["v"]
            _G8[vid] = (ids, {"pred": a["pred"], "changes_pred": a["changes_pred"]})
        assert sorted(len(v[0]) for v in _G8.values()) == [3702, 5157, 6971, 9015]
    return _G8


@pytest.mark.parametrize("K", list(range(1, 33)))
def test_bursts_of_every_size_equal_aggregate_on_the_g8_videos(K):
    for vid, (ids, want) in _g8().items():
        assert aggregate_online(ids, 200, n_classes=12, bursts=K) == want, (vid, K)


def test_a_ragged_sequence_of_bursts_equals_aggregate():
    rng = random.Random(13)
    for vid, (ids, want) in _g8().items():
        sizes = [rng.randint(1, 32) for _ in range(len(ids))]
        assert len(set(sizes)) == 32
        assert aggregate_online(ids, 200, n_classes=12, bursts=sizes) == want, vid
        # the record itself, word for word, after every burst: a burst leaves what its ids leave one at a time
        a, b, at = OnlineRecord(7, 12, 1 << 20), OnlineRecord(7, 12, 1 << 20), 0
        for k in sizes:
            if at >= len(ids):
                break
            a.push_frames(ids[at:at + k])
            for i in ids[at:at + k]:
                b.push(i)
            at += k
            assert vars(a) == vars(b)
        assert a.frames == len(ids) and len(a.event_id) > 1
    with pytest.raises(ValueError, match="burst sizes"):
        aggregate_online([1, 2], 200, bursts=0)


def test_small_windows_inside_a_burst():
    ids = [2, 2, 0, 1, 1, 1, 0, 0, 3, 3, 3]
    for window in (1, 2, 3, 4):
        want = aggregate({"v": {"pred": ids, "gt": [0] * len(ids)}}, window_size=window)["v"]
        for K in (1, 2, 3, 5, 7, 11, 32):                       # multiples of the window and not; a burst that spans several windows
            got = aggregate_online(ids, window, bursts=K)
            assert got == {"pred": want["pred"], "changes_pred": want["changes_pred"]}, (window, K)
    r = OnlineRecord(window=3, n_classes=4, max_events=2)
    r.push_frames([1, 1, 0, 2, 2, 2, 0, 0])                      # two finished windows and the start of a third
    assert r.result() == {"pred": [1, 2], "changes_pred": [3, 6], "frames": 8} and r.overflow == 0
    r.push_frames([0, 3, 3, 3])                                  # a third and a fourth event inside one burst: both dropped
    assert r.overflow == 1 and r.result()["pred"] == [1, 2] and r.frames == 12


@pytest.mark.parametrize("cid", ["L4-C12", "L1-C12"])
def test_bursts_of_the_automaton_equal_its_frame_by_frame_run(cid):
    """the reference of tests/test_gpu_step_frames.py is ONE run over T frames; a burst is compared with its slice.  Here: the automaton
    restarted at every burst boundary from the state it left gives those slices, for the burst patterns the GPU test drives"""
    case, sd, n, T, feats, res = SW.reference(cid)
    _, meta = A.build_state_dict(case)
    L, C = case.ant_len, case.n_classes
    full = [t.view(n, T, *t.shape[1:]) for t in (res.logits, res.argmax, res.h[0], res.ant_logits, res.ant_argmax)]
    for sizes in ((3, 3, 2), (8,), (1, 2, 5), (2,) * 4):
        assert sum(sizes) == T
        h, at = None, 0
        for K in sizes:
            part = [(r[at:at + K], f) for r, f in feats]
            got = A.run(sd, meta, case, part, h0=h)
            for name, g, w in zip(("logits", "argmax", "state", "anticipation logits", "anticipation argmax"),
                                  (got.logits, got.argmax, got.h[0], got.ant_logits, got.ant_argmax), full):
                assert torch.equal(g.view(n, K, *g.shape[1:]), w[:, at:at + K]), (sizes, at, name)
            assert torch.equal(got.h_last, full[2][:, at + K - 1].to(torch.float32))
            h, at = got.h_last, at + K
    assert L >= 1 and C == 12


def _args(hdr, name):
    m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/prego_amd.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_entry_points_are_declared_and_bound():
    from prego_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "prego_amd.h")).read()
    want = {"prego_miniroad_step_frames_workspace_bytes": 3, "prego_miniroad_step_frames": 12, "prego_miniroad_step_frames_anticipation": 14,
            "prego_miniroad_step_pool_frames_workspace_bytes": 3, "prego_miniroad_step_pool_frames": 15}
    for name, n_args in want.items():
        assert len(_args(hdr, name)) == n_args, name
        assert name in _lib.SYMBOLS
    a = _args(hdr, "prego_miniroad_step_frames")
    assert a[1].endswith("n_streams") and a[2].endswith("n_frames") and a[9].endswith("workspace") and a[11].endswith("stream")
    a = _args(hdr, "prego_miniroad_step_frames_anticipation")
    assert a[8].endswith("ant_out") and a[9].endswith("ant_argmax") and a[11].endswith("workspace")
    a = _args(hdr, "prego_miniroad_step_pool_frames")
    assert a[2].endswith("n_active") and a[3].endswith("n_frames") and a[4].endswith("slots") and a[12].endswith("workspace")
    assert "#define PREGO_ABI_VERSION 7" in hdr
    src = open(os.path.join(ROOT, "prego_amd", "_lib.py")).read()
    for name in want:
        assert f"lib.{name}.argtypes" in src, f"{name} has no prototype in _lib"


def test_python_surface():
    import prego_amd.model as M
    from prego_amd.engine import MiniRoadEngine
    from prego_amd.stream_pool import StreamPool
    assert callable(MiniRoadEngine.step_frames) and callable(M.MROAD.step_frames) and callable(M.MROADA.step_frames)
    assert M.MROADA.step_frames is not M.MROAD.step_frames
    assert callable(StreamPool.push_frames) and callable(OnlineRecord.push_frames)
