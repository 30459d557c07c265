"""The automaton cases of the MiniROADA streaming tests (tests/test_anticipation_step_cpu.py proves on the CPU what
tests/test_gpu_anticipation_step.py relies on): built from the public parts of tests/helpers/gru_automaton.py, 16 streams of T frames."""
import torch

from tests.helpers import gru_automaton as A

# id: (ant_len, n_classes, case seed, frames per stream, feature seed, stream counts the GPU test runs)
CASES = {
    "L1-C12": (1, 12, 51, 40, 16, (1, 3, 4, 5, 16)),
    "L4-C12": (4, 12, 54, 40, 16, (1, 3, 4, 5, 16)),
    "L8-C12": (8, 12, 58, 40, 16, (1, 3, 4, 5, 16)),
    "L8-C86": (8, 86, 61, 24, 17, (1, 16)),               # six class tiles
    "L3-C22": (3, 22, 62, 24, 17, (1, 16)),               # odd L, two class tiles, the halved tile of the hidden product
    "L32-C12": (32, 12, 63, 24, 17, (1, 16)),             # the largest anticipation_length
}
N_STREAMS = 16


def ant_ties(res):
    """(frame, step) pairs whose anticipation maximum is held by more than one class"""
    return int(((res.ant_logits == res.ant_logits.max(dim=-1, keepdim=True).values).sum(dim=-1) > 1).sum())


def reference(cid, device="cpu"):
    """(case, sd, T, feats, Result) with conditions() checked and at least one tie for the anticipation maximum; the feature bits are
    drawn on the CPU whatever `device` computes the reference, so that the CPU proof is about the inputs the GPU test uses"""
    L, C, seed, T, fseed, _ = CASES[cid]
    case = A.Case(ant_len=L, seed=seed, n_classes=C, **A.RGB)
    sd, meta = A.build_state_dict(case)
    feats = A.build_features(case, [T] * N_STREAMS, fseed, "cpu", sigma=meta["sigma"])
    feats = [tuple(None if t is None else t.to(device) for t in rf) for rf in feats]
    res = A.run(sd, meta, case, feats, device=device)
    A.conditions(sd, case, res)
    assert ant_ties(res) > 0, f"{cid}: no tie for the anticipation maximum in the reference"
    return case, sd, T, feats, res
