"""What the nine streaming entries answer to a wrong call, held to the texts recorded before they shared prego_amd/_stream_call.py: the
table of tests/helpers/stream_refusal_cases.py runs once and must equal tests/golden/stream_refusals.json (scripts/gen_stream_refusals.py)
case for case - exception type and message, which also pins the order of the refusals (the cases wrong in two ways) and the policies the
entries do not share (a CUDA counts tensor, one int for the counts, `step`'s wording)."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.helpers import stream_refusal_cases as R      # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "stream_refusals.json")


def test_every_refusal_is_the_recorded_one():
    want = [tuple(row) for row in json.load(open(GOLDEN))]
    got = [tuple(row) for row in R.record()]
    assert [g[0] for g in got] == [w[0] for w in want], "the case table and the golden file list different cases: record the file again at the parent"
    wrong = [f"{g[0]}:\n    recorded {w[1]}: {w[2]}\n    now      {g[1]}: {g[2]}" for g, w in zip(got, want) if g != w]
    assert not wrong, f"{len(wrong)} of {len(want)} cases answer differently:\n" + "\n".join(wrong)
    kinds = {w[1] for w in want}
    assert kinds == {"PregoError", "TypeError", "ok"} and sum(1 for w in want if w[0].split("/")[2].startswith("two:")) >= 6
    assert not any("0x" in w[2] or "(nil)" in w[2] for w in want)                # no pointer in a pinned text
