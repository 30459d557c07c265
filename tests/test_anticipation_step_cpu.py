"""CPU side of MiniROADA streaming (prego_miniroad_step_anticipation, csrc/stream_ant.hip): the automaton cases of
tests/test_gpu_anticipation_step.py stay inside conditions() and have exact ties for the anticipation maximum, and the entry point is
declared and bound."""
import os
import re

import pytest

torch = pytest.importorskip("torch")

from tests.helpers import ant_step_cases as S               # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (frame, step) pairs with a tie, counted once on the CPU when the cases were chosen: a change of the helper that moves them shows here
TIES = {"L1-C12": 20, "L4-C12": 924, "L8-C12": 278, "L8-C86": 253, "L3-C22": 102, "L32-C12": 3873}


@pytest.mark.parametrize("cid", list(S.CASES))
def test_case_is_exact_and_has_ties(cid):
    case, sd, T, feats, res = S.reference(cid)               # conditions() and ties > 0 inside
    L, C = S.CASES[cid][0], S.CASES[cid][1]
    assert res.ant_logits.shape == (S.N_STREAMS * T, L, C) and res.ant_argmax.shape == (S.N_STREAMS * T, L)
    assert S.ant_ties(res) == TIES[cid]
    assert res.stats["max_A"] <= 10                          # A_l stays a small integer: exact in bf16 and fp16
    assert float(res.ant_logits.abs().max()) < 2 ** 24       # exact in fp32 in any summation order


def test_entry_point_is_declared_and_bound():
    from prego_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "prego_amd.h")).read()
    m = re.search(r"int\s+prego_miniroad_step_anticipation\s*\(([^;]*)\)\s*;", hdr)
    assert m, "prego_miniroad_step_anticipation is not declared in include/prego_amd.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 11 and args[7].endswith("ant_out") and args[8].endswith("ant_argmax")
    assert "prego_miniroad_step_anticipation" in _lib.SYMBOLS
    assert "prego_miniroad_step" in _lib.SYMBOLS
