#!/usr/bin/env python3
"""Records what the nine streaming entries answer to the wrong calls of tests/helpers/stream_refusal_cases.py:

    python scripts/gen_stream_refusals.py [OUT]        # default tests/golden/stream_refusals.json

Run it on a built checkout of the commit whose texts are to be pinned (the file in the tree was written at the parent of the commit
that introduced prego_amd/_stream_call.py); tests/test_gpu_stream_refusals.py then requires every later tree to give the same list."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import stream_refusal_cases as R      # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "stream_refusals.json")
    got = R.record()
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(row) for row in got) + "\n]\n")
    print(f"{len(got)} cases -> {out}; " + ", ".join(f"{k}: {sum(1 for r in got if r[1] == k)}" for k in sorted({r[1] for r in got})))
