"""CPU side of the wide streaming step (prego_miniroad_step_wide / _anticipation, csrc/stream_wide.hip): the automaton cases of
tests/test_gpu_step_wide.py stay inside conditions(), have exact ties for the trunk and for the anticipation maximum and pairwise-distinct
streams (a stream written to another stream's row cannot pass), and the entry points are declared and bound."""
import os
import re

import pytest

torch = pytest.importorskip("torch")

from tests.helpers import ant_step_cases as S               # noqa: E402
from tests.helpers import step_wide_cases as SW             # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (frames with a tie for the trunk maximum, (frame, step) pairs with a tie for the anticipation maximum), counted once on the CPU when the
# cases were chosen: a change of the helpers that moves them shows here
TIES = {"L1-C12": (17, 7), "L4-C12": (127, 439), "L8-C12": (115, 175), "L32-C12": (70, 2016), "L8-C86": (173, 468), "L3-C22": (218, 432)}


@pytest.mark.parametrize("cid", list(SW.CASES))
def test_case_is_exact_has_ties_and_distinct_streams(cid):
    case, sd, n, T, feats, res = SW.reference(cid)           # conditions() inside
    L, C = case.ant_len, case.n_classes
    assert (n, T) == SW.CASES[cid] and 16 < n <= 256
    assert res.logits.shape == (n * T, C) and res.ant_logits.shape == (n * T, L, C) and res.ant_argmax.shape == (n * T, L)
    assert (SW.trunk_ties(res), S.ant_ties(res)) == TIES[cid]
    assert SW.trunk_ties(res) > 0 and S.ant_ties(res) > 0
    assert res.stats["max_A"] <= 10                          # A_l stays a small integer: exact in bf16 and fp16
    assert float(res.ant_logits.abs().max()) < 2 ** 24       # exact in fp32 in any summation order
    last = res.logits.view(n, T, C)[:, -1]
    same = (last[:, None, :] == last[None, :, :]).all(-1)
    assert int(same.sum()) == n, "two streams end on the same logits"


def _args(hdr, name):
    m = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/prego_amd.h"
    return [a.strip() for a in m.group(1).split(",")]


def test_entry_points_are_declared_and_bound():
    from prego_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "prego_amd.h")).read()
    assert len(_args(hdr, "prego_miniroad_step_wide_workspace_bytes")) == 2
    a = _args(hdr, "prego_miniroad_step_wide")
    assert len(a) == 11 and a[8].endswith("workspace") and a[9].endswith("workspace_bytes")
    a = _args(hdr, "prego_miniroad_step_wide_anticipation")
    assert len(a) == 13 and a[7].endswith("ant_out") and a[8].endswith("ant_argmax") and a[10].endswith("workspace")
    for name in ("prego_miniroad_step_wide_workspace_bytes", "prego_miniroad_step_wide", "prego_miniroad_step_wide_anticipation"):
        assert name in _lib.SYMBOLS
    assert "#define PREGO_ABI_VERSION 7" in hdr


def test_python_surface():
    import prego_amd.model as M
    from prego_amd.engine import MiniRoadEngine
    assert callable(MiniRoadEngine.step_wide) and callable(M.MROAD.step_wide) and callable(M.MROADA.step_wide)
    assert M.MROADA.step_wide is not M.MROAD.step_wide
