"""CPU: the parts of Evaluate's batching that need no device - the by-length split of a batch (`split_by_length`), the frame ranges a
video's features are copied in (`_pieces_of`), and the order of the pass loop's phases with the stand-in model of
tests/test_distributed_cpu.py.  The split's expectations are worked out by hand from its rule."""
import json
import logging
import os

import numpy as np
import pytest
import torch

from tests.test_distributed_cpu import _FakeModel

TAIL = ["collect_last", "check", "json_written"]


def _cfg(tmp_path, name, **extra):
    from prego_amd.config import epic_tent_cfg
    vl = os.path.join(tmp_path, "vl.json")
    json.dump({"EPIC-TENT-O": {"class_index": [f"c{i}" for i in range(12)]}}, open(vl, "w"))
    return epic_tent_cfg(eval="x.pth", video_list_path=vl, eval_output_dir=os.path.join(tmp_path, name), **extra)


# ---- the by-length split ---------------------------------------------------------------------------------------------------------
def test_fewer_than_16_videos_stay_one_part_in_loader_order():
    from prego_amd.evaluate import split_by_length
    assert split_by_length([], 4, None) == [[]]
    assert split_by_length([7], 4, None) == [[0]]
    assert split_by_length([5, 90, 1, 40, 90, 3, 8, 2, 60, 10, 20, 30, 4, 6, 9], 4, 0.5) == [list(range(15))]


def test_16_videos_split_into_the_longest_first_and_the_rest():
    from prego_amd.evaluate import split_by_length
    frames = [10, 80, 30, 100, 5, 60, 20, 90, 1, 70, 40, 50, 15, 25, 35, 45]                  # 676 frames
    by_length = [3, 7, 1, 9, 5, 11, 15, 10, 14, 2, 13, 6, 12, 0, 4, 8]
    assert sorted(by_length) == list(range(16)) and [frames[i] for i in by_length] == sorted(frames, reverse=True)
    # 0.5 x 676 = 338: 100 + 90 + 80 = 270 fits, + 70 = 340 does not
    assert split_by_length(frames, 4, 0.5) == [by_length[:3], by_length[3:]]
    # 0.2 x 676 = 135.2: 100 fits, + 90 does not
    assert split_by_length(frames, 4, 0.2) == [by_length[:1], by_length[1:]]
    # a prefix that ends exactly on the budget still belongs to the first part: 0.25 x 760 = 190 = 100 + 90
    assert split_by_length(frames[:8] + [85] + frames[9:], 4, 0.25)[0] == [3, 7]
    # equal lengths keep the loader's order among themselves
    assert split_by_length([9] * 16, 4, 0.5) == [list(range(8)), list(range(8, 16))]


def test_the_first_part_always_leaves_a_video_behind():
    from prego_amd.evaluate import split_by_length
    assert split_by_length([4] * 16, 4, 1.0) == [list(range(15)), [15]]
    assert split_by_length([4] * 16, 4, 5.0) == [list(range(15)), [15]]


def test_an_empty_prefix_is_one_part():
    from prego_amd.evaluate import split_by_length
    frames = [1000] + [10] * 15                           # 0.5 x 1150 = 575 < the longest video
    assert split_by_length(frames, 4, 0.5) == [list(range(16))]
    frames = [10] * 15 + [1000]                           # one part, in the order the rule sorted it: by length
    assert split_by_length(frames, 4, 0.5) == [[15] + list(range(15))]
    assert split_by_length([0] * 16, 4, 0.0) == [list(range(15)), [15]]        # no frames: nothing is over a budget of 0


def test_the_default_fraction_follows_the_element_size():
    from prego_amd.evaluate import split_by_length
    frames = [10] * 20                                    # 200 frames: half of them is 10 videos, a fifth is 4
    assert split_by_length(frames, 4, None) == split_by_length(frames, 4, 0.5) == [list(range(10)), list(range(10, 20))]
    assert split_by_length(frames, 8, None) == split_by_length(frames, 4, 0.5)
    assert split_by_length(frames, 2, None) == split_by_length(frames, 2, 0.2) == [list(range(4)), list(range(4, 20))]
    assert split_by_length(frames, 1, None) == split_by_length(frames, 2, 0.2)


# ---- _pieces_of ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,Q", [(8, 3), (8, 8), (5, 2), (4, 9)])
def test_pieces_tile_a_video_with_short_pieces_at_its_tail(tmp_path, P, Q):
    from prego_amd.evaluate import Evaluate
    ev = Evaluate(_cfg(str(tmp_path), "o"))
    ev.PIECE_FRAMES, ev.TAIL_PIECE_FRAMES = P, Q
    q = min(Q, P)                                         # a tail piece is never longer than a piece
    for T in (0, 1, Q, P + Q, P + Q + 1, 3 * P + 5):
        pieces = ev._pieces_of(T)
        assert [a for a, _ in pieces] == [0] * bool(pieces) + [b for _, b in pieces[:-1]]      # each piece starts where the last one ended
        assert (pieces[-1][1] if pieces else 0) == T and all(a < b for a, b in pieces)
        n_full = len([a for a in range(0, T, P) if T - a > P + q])      # whole pieces as long as more than a piece + a tail piece is left
        assert pieces[:n_full] == [(k * P, (k + 1) * P) for k in range(n_full)]
        tail = pieces[n_full:]
        assert all(b - a == q for a, b in tail[:-1]) and all(b - a <= q for a, b in tail)
    assert Evaluate.PIECE_FRAMES == 8192 and Evaluate.TAIL_PIECE_FRAMES == 2048 and Evaluate.EVENT_BYTES == 64 << 20


def test_eval_piece_frames_sets_the_piece_length(tmp_path):
    from prego_amd.evaluate import Evaluate
    ev = Evaluate(_cfg(str(tmp_path), "o", eval_piece_frames=4096))
    assert ev._pieces_of(4096 + 2048 + 1) == [(0, 4096), (4096, 6144), (6144, 6145)]
    assert ev._pieces_of(4096 + 2048) == [(0, 2048), (2048, 4096), (4096, 6144)]


# ---- the pass loop with the stand-in model ---------------------------------------------------------------------------------------
def _stand_in_pass(tmp_path, name, **extra):
    from prego_amd import weights as W
    from prego_amd.evaluate import Evaluate
    from oracle.oracle_torch import TorchPort
    cfg = _cfg(tmp_path, name, **extra)
    model = _FakeModel(TorchPort(W.miniroad_state_dict(cfg, 20, head_gain=8.0), 1024))
    assert model.max_clips == 4
    items = []
    for i, T in enumerate([30, 11, 25, 18, 9]):
        tgt = np.zeros((T, 12), np.float32)
        tgt[np.arange(T), (np.arange(T) // 5 + i) % 12] = 1
        items.append((torch.from_numpy(W.tsn_features((T, 2048), 9, f"eb.{i}"))[None], torch.zeros(1, T, 2048), torch.from_numpy(tgt)[None],
                      (f"v{i}",), torch.tensor([0]), torch.tensor([T])))
    ev = Evaluate(cfg)
    mAP = float(ev(model, items, logging.getLogger("t"), "cpu"))
    return [p for p, _ in ev.phase_log], open(os.path.join(tmp_path, name, "output_miniROAD.json"), "rb").read(), mAP


def test_phases_of_a_pass_and_of_a_pass_of_one_video_batches(tmp_path):
    phases, text, mAP = _stand_in_pass(str(tmp_path), "clips")
    assert phases == ["loader", "launch", "collect"] * 2 + TAIL          # four videos fill the model's clips; the fifth goes behind the loop
    phases1, text1, mAP1 = _stand_in_pass(str(tmp_path), "one", eval_frames_per_batch=1)
    assert phases1 == ["loader", "launch", "collect"] * 6 + TAIL         # five batches in the loop, and the empty one behind it
    assert text1 == text and mAP1 == mAP
    assert list(json.loads(text)) == [f"v{i}" for i in range(5)] and 0.0 < mAP <= 1.0
