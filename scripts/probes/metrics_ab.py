"""Bit-for-bit A/B of the metric entries (csrc/metrics.hip, the metric part of csrc/host_misc.cpp): the tree's library against
prego_amd/lib_ab/libold.so (bash scripts/build_old.sh metrics.hip host_misc.cpp: those two sources as of git HEAD), both opened in one
process.  Per shape, tie-free and with three score levels: prego_perframe_ap / _cap (dense targets) and prego_perframe_ap_labels /
_cap_labels, prego_perstage_ap_labels / _cap_labels (ids) - the raw bytes of every output array and the four *_workspace_bytes results;
then the return codes and prego_last_error texts of an n = 0 call, a NULL-argument call and a call with the workspace one byte short.
Every comparison must be equal.  One JSON line: comparisons, mismatches.  usage: python scripts/probes/metrics_ab.py [--old LIB] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np                                           # noqa: E402
import torch                                                 # noqa: E402

from prego_amd import _lib                                   # noqa: E402

SHAPES = [(1, 3), (63, 5), (4097, 12), (8193, 86), (9001, 130), (5000, 3), (90_000, 70), (140_000, 2)]
BIG = {(90_000, 70), (140_000, 2)}       # dense: one class positive on every frame (ap_count's fallback); ids: also one run over all
KINDS = ["perframe_ap", "perframe_cap", "perstage_ap", "perstage_cap"]


def scores_of(rng, n, ncls, levels):
    """levels = 0: a permutation of distinct values per column; else every column quantised to that many values"""
    if levels:
        return (rng.integers(0, levels, (n, ncls)) / np.float32(levels - 1)).astype(np.float32)
    base = (np.arange(n, dtype=np.float32) - n // 2) / np.float32(max(n, 2))
    return np.stack([rng.permutation(base) for _ in range(ncls)], axis=1)


def run_ids(rng, n, ncls):
    """runs of 1..300 frames; ids -1 and ncls: negatives of every class"""
    lens = rng.integers(1, 301, n)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), n)) + 1]
    return np.repeat(rng.integers(-1, ncls + 1, lens.shape[0]), lens)[:n].astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=os.path.join(ROOT, "prego_amd", "lib_ab", "libold.so"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_ab: no GPU")
    libs = {"new": _lib.load(), "old": _lib._open(args.old, debug=False)}
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_cmp, bad = 0, []

    def same(what, a, b):
        nonlocal n_cmp
        n_cmp += 1
        if a != b:
            bad.append(what if len(repr(a)) > 200 else f"{what}: {a!r} != {b!r}")

    def call(lib, kind, by_ids, scores, truth, n, ncls, ws, ws_bytes):
        """-> (rc, the output arrays' bytes, the error text of a refusal)"""
        stage = kind.startswith("perstage")
        rows = max(ncls, 1)                                   # never an empty tensor: its pointer would be NULL
        outs = [torch.full(((10, rows) if stage else (rows,)), -7.0, dtype=torch.float64, device="cuda") for _ in range(2 if stage else 3)]
        fn = getattr(lib, f"prego_{kind}" + ("_labels" if by_ids else ""))
        rc = fn(p(scores), p(truth), n, ncls, *[p(o) for o in outs], p(ws), ws_bytes, stream)
        torch.cuda.synchronize()
        return rc, [o.cpu().numpy().tobytes() for o in outs], (lib.prego_last_error() if rc else b"")

    def both(what, kind, by_ids, scores, truth, n, ncls, short=0, no_ws=False):
        res = {}
        for name, lib in libs.items():
            need = getattr(lib, f"prego_{kind}_workspace_bytes")(n, ncls)
            refused = n <= 0 or n >= 1 << 31 or ncls <= 0         # no entry touches the workspace then: 16 bytes stand in for it
            ws = None if no_ws else torch.full((16 if refused else need,), 0x5A, dtype=torch.uint8, device="cuda")
            res[name] = (need,) + call(lib, kind, by_ids, scores, truth, n, ncls, ws, 16 if refused else need - short)
        for i, part in enumerate(("workspace_bytes", "rc", "outputs", "error")):
            same(f"{what} {kind}{'_labels' if by_ids else ''} {part}", res["new"][i], res["old"][i])

    for n, ncls in SHAPES:
        for levels in (0, 3):
            rng = np.random.default_rng(7 * n + ncls + levels)
            sc = scores_of(rng, n, ncls, levels)
            id_cases = {"runs": run_ids(rng, n, ncls)}
            if (n, ncls) in BIG:
                dense = (rng.random((n, ncls)) < 0.01).astype(np.float32)
                dense[:, ncls - 1] = 1.0
                id_cases["one run"] = np.full(n, ncls - 1, np.int32)
            else:
                ids = id_cases["runs"]
                dense = np.zeros((n, ncls), np.float32)
                ok = (ids >= 0) & (ids < ncls)
                dense[np.arange(n)[ok], ids[ok]] = 1
            sc_d, dense_d = torch.from_numpy(sc).cuda(), torch.from_numpy(dense).cuda()
            what = f"({n}, {ncls}) levels {levels}"
            for kind in KINDS[:2]:
                both(what + " dense", kind, False, sc_d, dense_d, n, ncls)
            for case, ids in id_cases.items():
                ids_d = torch.from_numpy(ids).cuda()
                for kind in KINDS:
                    both(f"{what} ids {case}", kind, True, sc_d, ids_d, n, ncls)
    # refusals and the empty set: codes, texts and what is left in the outputs
    n, ncls = 100, 4
    sc_d = torch.rand(n, ncls, device="cuda")
    ids_d = torch.randint(0, ncls, (n,), dtype=torch.int32, device="cuda")
    dense_d = torch.nn.functional.one_hot(ids_d.long(), ncls).float()
    for kind in KINDS:
        for by_ids in ((True,) if kind.startswith("perstage") else (False, True)):
            truth = ids_d if by_ids else dense_d
            both("n = 0", kind, by_ids, sc_d, truth, 0, ncls, no_ws=True)
            both("n = 0 with a workspace", kind, by_ids, sc_d, truth, 0, ncls)
            both("NULL scores", kind, by_ids, None, truth, n, ncls)
            both("NULL truth", kind, by_ids, sc_d, None, n, ncls)
            both("NULL workspace", kind, by_ids, sc_d, truth, n, ncls, no_ws=True)
            both("workspace one byte short", kind, by_ids, sc_d, truth, n, ncls, short=1)
            both("n_classes 0", kind, by_ids, sc_d, truth, n, 0)
            both("n_frames 2^31", kind, by_ids, sc_d, truth, 1 << 31, ncls)
    line = json.dumps({"probe": "metrics_ab", "old": os.path.relpath(args.old, ROOT), "comparisons": n_cmp, "mismatches": len(bad),
                       "first_mismatches": bad[:10]})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
