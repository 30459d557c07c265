"""The automaton cases of the wide streaming step (tests/test_step_wide_cpu.py proves on the CPU what tests/test_gpu_step_wide.py relies on):
the (ant_len, n_classes, case seed, feature seed) of tests/helpers/ant_step_cases.py with n streams of T frames instead of 16."""
import torch

from tests.helpers import ant_step_cases as S
from tests.helpers import gru_automaton as A

# id (a case of ant_step_cases.CASES): (streams per call, frames per stream)
CASES = {
    "L1-C12": (17, 8),             # one full tile plus a tail of one
    "L4-C12": (37, 8),             # two tiles plus a tail of five
    "L8-C12": (64, 6),             # four full tiles
    "L32-C12": (33, 6),            # the largest anticipation_length
    "L8-C86": (144, 6),            # nine tiles, six class tiles
    "L3-C22": (256, 6),            # the maximum, the halved tile of the hidden product, two class tiles
}


def trunk_ties(res):
    """frames whose maximal logit is held by more than one class"""
    return int(((res.logits == res.logits.max(dim=-1, keepdim=True).values).sum(dim=-1) > 1).sum())


def reference(cid, device="cpu"):
    """(case, sd, n, T, feats, Result) with conditions() checked; the feature bits are drawn on the CPU whatever `device` computes the
    reference, so that the CPU proof is about the inputs the GPU test uses"""
    L, C, seed, _, fseed, _ = S.CASES[cid]
    n, T = CASES[cid]
    case = A.Case(ant_len=L, seed=seed, n_classes=C, **A.RGB)
    sd, meta = A.build_state_dict(case)
    feats = A.build_features(case, [T] * n, fseed, "cpu", sigma=meta["sigma"])
    feats = [tuple(None if t is None else t.to(device) for t in rf) for rf in feats]
    res = A.run(sd, meta, case, feats, device=device)
    A.conditions(sd, case, res)
    return case, sd, n, T, feats, res
