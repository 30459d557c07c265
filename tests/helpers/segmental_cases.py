"""Inputs shared by tests/test_segmental_cpu.py and tests/test_gpu_segmental.py: the hand-computed cases of the segmental metrics
(records worked out on paper from the definitions in include/prego_amd.h: correct | frames | m | n | dist | tp@1/10 | tp@1/4 | tp@1/2)
and the seeded random video sets."""
import numpy as np

# name -> {"pred": [video, ..], "gt": [video, ..], "bg": ids, "records": [[8 ints] per video]}
HAND_CASES = {
    # one pred segment of label 1 over the whole video, a gt segment of label 1 on frame 0 only: inter 1, union = the video's length
    "iou_exactly_at_each_threshold": {
        "pred": [[1] * 10, [1] * 4, [1] * 2],
        "gt": [[1] + [2] * 9, [1] + [2] * 3, [1, 2]],
        "records": [[1, 10, 1, 2, 1, 1, 0, 0], [1, 4, 1, 2, 1, 1, 1, 0], [1, 2, 1, 2, 1, 1, 1, 1]]},
    "iou_one_below_each_threshold": {           # 1/11 < 1/10; 1/5 < 1/4; 1/3 < 1/2
        "pred": [[1] * 11, [1] * 5, [1] * 3],
        "gt": [[1] + [2] * 10, [1] + [2] * 4, [1, 2, 2]],
        "records": [[1, 11, 1, 2, 1, 0, 0, 0], [1, 5, 1, 2, 1, 1, 0, 0], [1, 3, 1, 2, 1, 1, 1, 0]]},
    # pred (1,0,3) (2,3,4) (1,4,6) against gt (1,0,6): IoU 3/6 and 2/6, both best = the one gt segment: one true positive, not two
    "two_pred_segments_share_their_best": {
        "pred": [[1, 1, 1, 2, 1, 1]], "gt": [[1] * 6], "records": [[5, 6, 3, 1, 2, 1, 1, 1]]},
    # pred (1,0,5) against gt (1,0,2) (2,2,3) (1,3,5): 2/5 twice, the earlier wins; 2/5 reaches 1/10 and 1/4
    "iou_tie_between_two_gt_segments": {
        "pred": [[1] * 5], "gt": [[1, 1, 2, 1, 1]], "records": [[4, 5, 1, 3, 2, 1, 1, 0]]},
    # pred (1,0,6) overlaps gt (2,1,6) in 5 frames but its label is 2: the candidate is gt (1,0,1), IoU 1/6
    "better_overlap_of_another_label": {
        "pred": [[1] * 6], "gt": [[1, 2, 2, 2, 2, 2]], "records": [[1, 6, 1, 2, 1, 1, 0, 0]]},
    # pred (3,0,2) (3,4,6) - the background run between them is dropped, they stay two - against gt (3,0,6): 2/6 each
    "background_between_two_runs_of_one_label": {
        "pred": [[3, 3, 0, 0, 3, 3]], "gt": [[3] * 6], "bg": (0,), "records": [[4, 6, 2, 1, 1, 1, 1, 0]]},
    "all_background_video": {                   # background frames count in correct and frames; no segment on either side / on one side
        "pred": [[0, 0, 0], [0, 0]], "gt": [[0, 0, 0], [0, 5]], "bg": (0,),
        "records": [[3, 3, 0, 0, 0, 0, 0, 0], [1, 2, 0, 1, 1, 0, 0, 0]]},
    "empty_videos": {
        "pred": [[], [1, 1], []], "gt": [[], [1, 1], []],
        "records": [[0] * 8, [2, 2, 1, 1, 0, 1, 1, 1], [0] * 8]},
    # video 0 ends with label 1 and video 1 starts with it: two segments.  Video 1: pred (1,0,2) (2,2,3), gt (1,0,1) (2,1,3), IoU 1/2 twice
    "equal_labels_across_a_video_boundary": {
        "pred": [[1, 1], [1, 1, 2]], "gt": [[1, 1], [1, 2, 2]],
        "records": [[2, 2, 1, 1, 0, 1, 1, 1], [2, 3, 2, 2, 0, 2, 2, 2]]},
    # ids outside [0, 128) are ordinary labels: the mask bits 127 (-1 & 127) and 72 (200 - 128) do not touch them.  IoU 1/2 and 2/3
    "labels_minus_one_and_200": {
        "pred": [[-1, -1, 200, 200]], "gt": [[-1, 200, 200, 200]], "bg": (72, 127), "records": [[3, 4, 2, 2, 0, 2, 2, 2]]},
}


def run_sequence(rng, length, ids, mean_run):
    """`length` ids in runs of geometric length (mean `mean_run`; 1: every frame drawn alone)"""
    if length == 0:
        return np.zeros(0, np.int32)
    ids = np.asarray(ids)
    if mean_run <= 1:
        return ids[rng.integers(0, len(ids), size=length)].astype(np.int32)
    lens = rng.geometric(1.0 / mean_run, size=length)          # every run has a frame or more: enough of them
    vals = ids[rng.integers(0, len(ids), size=lens.size)]
    return np.repeat(vals, lens)[:length].astype(np.int32)


def random_videos(rng, n_videos, max_len=5000, alphabet=12, out_of_range=False, mask="none", lengths=None):
    """-> (pred videos, gt videos, bg): lengths 0 .. max_len with empty videos first and last (from three videos on) and inside (from five on), per video a
    run-length mix drawn from one-frame runs / short / long runs; pred = gt with stretches redrawn, so that segments overlap in every
    way.  alphabet: ids 0 .. alphabet - 1, out_of_range: plus -1, -7, 128, 200, 2^31 - 1.  mask: 'none' | 'some' | 'all' of the ids in
    [0, 128) are background."""
    ids = list(range(alphabet)) + ([-1, -7, 128, 200, 2 ** 31 - 1] if out_of_range else [])
    if lengths is None:
        lengths = [int(x) for x in rng.integers(0, max_len + 1, size=n_videos)]
        if n_videos >= 3:
            lengths[0] = lengths[-1] = 0
        if n_videos >= 5:
            lengths[n_videos // 2] = 0
    P, G = [], []
    for n in lengths:
        g = run_sequence(rng, n, ids, (1, 7, 150)[int(rng.integers(0, 3))])
        p = g.copy()
        noise = run_sequence(rng, n, ids, (1, 7, 150)[int(rng.integers(0, 3))])
        redo = run_sequence(rng, n, [0, 1], (3, 40)[int(rng.integers(0, 2))]).astype(bool)
        p[redo] = noise[redo]
        if n > 3:
            k = int(rng.integers(0, 3))
            p = np.concatenate((p[k:], p[:k]))              # a shift: boundaries that differ by a few frames
        P.append(np.ascontiguousarray(p, dtype=np.int32))
        G.append(g)
    bg = {"none": (), "some": tuple(range(0, min(alphabet, 128), 3)), "all": tuple(range(min(alphabet, 128)))}[mask]
    return P, G, bg


def concat(videos):
    """-> (int32 [frames], int32 offsets [videos + 1])"""
    off = np.concatenate(([0], np.cumsum([len(v) for v in videos]))).astype(np.int32)
    flat = np.concatenate([np.asarray(v, dtype=np.int32).reshape(-1) for v in videos] + [np.zeros(0, np.int32)])
    return flat, off
