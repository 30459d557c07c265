"""CPU: the host model of the segmental metrics (prego_amd/segmental.py: MoF, segmental Edit, segmental F1 at three overlaps) against
hand-computed cases, against an independent restatement in the usual sequential fp64 form (full-matrix Levenshtein, argmax over IoU x
label equality, a `hits` list) on seeded random videos, and against the Epic-tent-O fixture (tests/golden/g8_output_miniROAD.json.gz,
tests/golden/segmental_epic_tent.json)."""
import gzip
import json
import os

import numpy as np
import pytest

from prego_amd.segmental import (DEFAULT_OVERLAPS, edit_distance, segmental_records, segmental_report, segmental_scores, segments,
                                 voted_frames)
from tests.helpers.segmental_cases import HAND_CASES, random_videos

G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_cases(name):
    case = HAND_CASES[name]
    rec = segmental_records(case["pred"], case["gt"], case.get("bg", ()))
    assert rec.dtype == np.int32 and rec.tolist() == case["records"], name


def test_segments_and_edit_distance():
    assert segments([3, 3, 0, 0, 3, 5], bg=(0,)).tolist() == [[3, 0, 2], [3, 4, 5], [5, 5, 6]]      # two runs of 3 around background stay two
    assert segments([3, 3, 0, 0, 3, 5]).tolist() == [[3, 0, 2], [0, 2, 4], [3, 4, 5], [5, 5, 6]]
    assert segments([]).shape == (0, 3) and segments([7], bg=(7,)).shape == (0, 3)
    assert segments([-1, -1, 200, 200]).tolist() == [[-1, 0, 2], [200, 2, 4]]
    with pytest.raises(ValueError):
        segments([1], bg=(128,))
    assert edit_distance([], []) == 0 and edit_distance([1, 2, 3], []) == 3 and edit_distance([], [4]) == 1
    assert edit_distance([1, 2, 3], [1, 2, 3]) == 0 and edit_distance([1, 2, 3], [1, 3]) == 1 and edit_distance([1, 2], [2, 1]) == 2
    assert edit_distance(list(b"kitten"), list(b"sitting")) == 3 and edit_distance(list(b"sitting"), list(b"kitten")) == 3


# ---- the independent restatement: sequential, fp64 ----
def _ref_segments(x, bg):
    out, i = [], 0
    while i < len(x):
        j = i
        while j < len(x) and x[j] == x[i]:
            j += 1
        if not (0 <= x[i] < 128 and x[i] in bg):
            out.append((int(x[i]), i, j))
        i = j
    return out


def _ref_levenshtein(p, y):
    D = np.zeros((len(p) + 1, len(y) + 1))
    D[:, 0] = np.arange(len(p) + 1)
    D[0, :] = np.arange(len(y) + 1)
    for i in range(1, len(p) + 1):
        for j in range(1, len(y) + 1):
            D[i, j] = D[i - 1, j - 1] if p[i - 1] == y[j - 1] else min(D[i - 1, j], D[i, j - 1], D[i - 1, j - 1]) + 1
    return int(D[-1, -1])


def _ref_tp(ps, gs, overlap):
    tp, hits = 0, [False] * len(gs)
    if not gs:
        return 0
    g_lab = np.array([g[0] for g in gs])
    g_s = np.array([g[1] for g in gs], dtype=np.float64)
    g_e = np.array([g[2] for g in gs], dtype=np.float64)
    for lab, s, e in ps:
        inter = np.minimum(e, g_e) - np.maximum(s, g_s)
        union = np.maximum(e, g_e) - np.minimum(s, g_s)
        iou = (inter / union) * (g_lab == lab)
        idx = int(np.argmax(iou))
        if iou[idx] >= overlap and not hits[idx]:
            tp += 1
            hits[idx] = True
    return tp


def _ref_records(P, Gt, bg, overlaps):
    rec = []
    for p, g in zip(P, Gt):
        ps, gs = _ref_segments(list(p), set(bg)), _ref_segments(list(g), set(bg))
        rec.append([int(sum(int(a == b) for a, b in zip(p, g))), len(p), len(ps), len(gs), _ref_levenshtein([s[0] for s in ps], [s[0] for s in gs])] +
                   [_ref_tp(ps, gs, num / den) for num, den in overlaps])
    return rec


def _ref_report(rec):
    rec = np.asarray(rec, dtype=np.float64).reshape(-1, 8)
    tot = rec.sum(0)
    rep = {"MoF": 100 * tot[0] / tot[1] if tot[1] else 0.0,
           "Edit": float(np.mean([100 * (1 - r[4] / max(r[2], r[3], 1)) for r in rec]))}
    for k, name in enumerate(("F1@10", "F1@25", "F1@50")):
        M, N, TP = tot[2], tot[3], tot[5 + k]
        if M + N == 0 or TP == 0:
            rep[name] = 0.0
        else:
            prec, recall = TP / M, TP / N
            rep[name] = 100 * 2 * prec * recall / (prec + recall)
    return rep


@pytest.mark.parametrize("seed", range(6))
def test_sequential_fp64_restatement(seed):
    """60 seeded videos per seed (360 in all), short enough for the full-matrix DP: records equal, reports within 1e-12"""
    rng = np.random.default_rng(100 + seed)
    P, Gt, bg = random_videos(rng, 60, max_len=160, alphabet=(1, 3, 12, 86, 128)[seed % 5], out_of_range=seed % 2 == 1,
                              mask=("none", "some", "all")[seed % 3])
    rec = segmental_records(P, Gt, bg)
    assert rec.tolist() == _ref_records(P, Gt, bg, DEFAULT_OVERLAPS)
    rep, want = segmental_report(rec), _ref_report(rec)
    for key, val in want.items():
        assert abs(rep[key] - val) <= 1e-12, (key, rep[key], val)
    assert rep["videos"] == 60 and len(rep["per_video"]) == 60


def test_report_edges_and_overlap_names():
    assert segmental_report(np.zeros((0, 8), np.int32))["MoF"] == 0.0
    rep = segmental_report(np.zeros((2, 8), np.int32))
    assert rep["MoF"] == 0.0 and rep["Edit"] == 100.0 and rep["F1@10"] == rep["F1@25"] == rep["F1@50"] == 0.0
    rep = segmental_report([[3, 4, 2, 2, 1, 2, 1, 0]], overlaps=((1, 3), (3, 4), (1, 1)))
    assert rep["MoF"] == 75.0 and rep["Edit"] == 50.0 and rep["F1@1/3"] == 100.0 and rep["F1@75"] == 50.0 and rep["F1@100"] == 0.0
    for bad in (((0, 4), (1, 4), (1, 2)), ((5, 4), (1, 4), (1, 2)), ((1, 40000), (1, 4), (1, 2)), ((1, 2), (1, 4))):
        with pytest.raises(ValueError):
            segmental_records([[1]], [[1]], overlaps=bad)


def test_transcripts_edit_only():
    d = json.load(open(os.path.join(G, "procedure_assembly101o.json")))
    seqs = d["sequences"]
    rep = segmental_scores([s["pred"] for s in seqs], [s["gt"] for s in seqs], transcripts=True)
    assert rep["videos"] == 182 and set(rep) == {"Edit", "videos", "per_video"}
    want = [100.0 * (1.0 - _ref_levenshtein(s["pred"], s["gt"]) / max(len(s["pred"]), len(s["gt"]), 1)) for s in seqs]
    assert abs(rep["Edit"] - float(np.mean(want))) <= 1e-12
    assert [v["dist"] for v in rep["per_video"][:20]] == [_ref_levenshtein(s["pred"], s["gt"]) for s in seqs[:20]]
    rep = segmental_scores([[1, 2, 2, 0, 3]], [[1, 2, 3]], bg=(0,), transcripts=True)         # entries are segments: the two 2s stay two
    assert rep["per_video"][0] == {"m": 4, "n": 3, "dist": 1, "Edit": 75.0}


# ---- the Epic-tent-O fixture ----
VOTED_DIST = [19, 12, 11, 6, 10, 5, 4, 16, 6, 7, 3, 5, 1, 5, 16]       # plain Levenshtein of the voted sequences (window 200, no background)
VOTED_M = [25, 18, 25, 8, 5, 7, 5, 23, 12, 12, 8, 12, 4, 2, 13]
GT_N = [9, 10, 18, 8, 14, 11, 4, 14, 16, 9, 9, 13, 3, 7, 23]


def test_epic_tent_fixture():
    g = json.load(gzip.open(os.path.join(G, "g8_output_miniROAD.json.gz")))
    P, Gt = [np.asarray(v["pred"]) for v in g.values()], [np.asarray(v["gt"]) for v in g.values()]
    raw = segmental_records(P, Gt)
    voted = segmental_records([voted_frames(p, 200) for p in P], Gt)
    assert voted[:, 4].tolist() == VOTED_DIST and voted[:, 2].tolist() == VOTED_M
    assert voted[:, 3].tolist() == GT_N and raw[:, 3].tolist() == GT_N
    assert raw[:, 2].min() == 18 and raw[:, 2].max() == 330
    assert raw[:, 1].tolist() == [len(p) for p in P]
    gold = json.load(open(os.path.join(G, "segmental_epic_tent.json")))
    assert gold["videos"] == list(g.keys()) and gold["window"] == 200
    assert raw.tolist() == gold["frames"] and voted.tolist() == gold["vote"]
