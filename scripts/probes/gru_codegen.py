#!/usr/bin/env python3
"""Generated-code comparison of the GRU recurrence files between two trees (profiles/gru_ab/codegen.md is its output).

    hipcc -O3 -std=c++17 -S --cuda-device-only --offload-arch=gfx950 prego_amd/csrc/<file>.hip -o <dir>/<file>.s     (both trees)
    python scripts/probes/gru_codegen.py <parent asm dir> <tree asm dir> > table.md

Per kernel on both sides: registers, scratch, spills, the counts of MFMA / vector-memory / LDS / barrier / vmcnt-wait instructions,
instruction lines, and whether the instruction stream is the parent's up to register names.  Kernels on one side only are listed.
For the multi-tile kernels: the vector-memory instructions between the end of each gather prefetch (a run of global_load_lds_dwordx4)
and the next `s_waitcnt vmcnt(5)` in layout order."""
import collections
import difflib
import re
import shutil
import subprocess
import sys

FILES = ("gru_recurrence", "gru_recurrence_x2", "gru_bptt")
COUNTS = (("mfma", r"v_mfma"), ("vm load", r"(buffer|global)_load_(?!lds)"), ("vm store", r"(buffer|global)_store"), ("lds-dma", r"global_load_lds"),
          ("ds_read", r"ds_read"), ("ds_write", r"ds_write"), ("s_barrier", r"s_barrier"), ("vmcnt", r"s_waitcnt.*vmcnt"))
REG = re.compile(r"\b(?:[vsa]\d+|[vsa]\[\d+:\d+\]|vcc(?:_lo|_hi)?|exec(?:_lo|_hi)?|m0|ttmp\d+)\b")
LABEL = re.compile(r"\.LBB\d+_")                              # a block label carries the kernel's index in its file
VM = re.compile(r"^(buffer|global)_(load|store|atomic)")


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(path):
    """{symbol: {"ins": [instruction lines], "meta": {key: int}}} of the kernels of one assembly file; registers, scratch and spills
    come from the amdhsa.kernels metadata at the end of the file"""
    text = open(path).read().split("\n")
    ks, cur = {}, None
    for ln in text:
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            cur = ks.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if ln.startswith(".Lfunc_end") or ln.startswith("\t.section") or ln.startswith("\t.amdhsa_kernel"):
            cur = None
            continue
        s = ln.split(";")[0].strip()
        if s and s[0] != "." and not s.endswith(":"):
            cur.append(s)
    out, block = {}, {}
    for ln in text[text.index("amdhsa.kernels:"):] + ["  - .end"]:
        if re.match(r"^  - \.", ln) or ln.startswith("amdhsa.target"):
            if "symbol" in block:
                out[block["symbol"]] = {"ins": ks[block["symbol"]], "meta": block}
            block = {}
        m = re.match(r"^\s+(?:- )?\.(\w+):\s+(\S+)", ln)
        if m and m.group(1) == "symbol":
            block["symbol"] = m.group(2)[:-3]
        elif m and m.group(1) in ("agpr_count", "vgpr_count", "sgpr_count", "private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count"):
            block[m.group(1)] = int(m.group(2))
    return out


def norm(ins):
    return [REG.sub("R", i) for i in ins]


def count(ins, pat):
    r = re.compile(pat)
    return sum(1 for i in ins if r.match(i))


def short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\((GruArgs|BpttArgs)(, float const\*)?\)$", "", name)
    return name.replace("unsigned short", "bf16_t").replace("_Float16", "f16_t").replace("(bool)", "").replace("true", "T").replace("false", "F")


def prefetch_windows(ins):
    """layout-order scan: the instructions between the last global_load_lds_dwordx4 in front of a vmcnt(5) wait and that wait"""
    out, i, n = [], 0, len(ins)
    while i < n:
        if ins[i].startswith("global_load_lds_dwordx4"):
            w, k = [], i + 1
            while k < n and not re.match(r"s_waitcnt.*vmcnt\(5\)", ins[k]):
                if ins[k].startswith("global_load_lds_dwordx4"):
                    w = []                                 # still inside the run, or a later run: start behind its end
                else:
                    w.append(ins[k])
                k += 1
            if k < n:
                out.append(w)
            i = k + 1
        else:
            i += 1
    return out


def window_by_path(w):
    """what a window issues on one path: the gi DMAs, the publish store (one instruction per arm of the `local` branch: the arms
    share the exchange buffer's resource, one of them carries sc1), the relu(h) store (the other resource), and loads that sit in an
    arm with its own vmcnt(0) behind them (the cursor's restart)"""
    vm = [(j, x) for j, x in enumerate(w) if VM.match(x)]
    if not vm:
        return "0: the wait follows the DMA run of the arm that did not prefetch (that arm waits vmcnt(0))"
    gi = sum(1 for _, x in vm if x.startswith("global_load_lds_dword "))
    stores = [x for _, x in vm if x.startswith("buffer_store")]
    rsrc = lambda x: re.search(r"s\[\d+:\d+\]", x).group(0)
    hx = {rsrc(x) for x in stores if x.endswith(" sc1")}
    arms, relu = [x for x in stores if rsrc(x) in hx], [x for x in stores if rsrc(x) not in hx]
    loads = [j for j, x in vm if x.startswith("global_load_dword")]
    drained = all(any(re.match(r"s_waitcnt.*vmcnt\(0\)", y) for y in w[j + 1:]) for j in loads)
    rest = len(vm) - gi - len(stores) - len(loads)
    return (f"{gi} gi DMA + 1 publish ({len(arms)} arms of one branch) + {len(relu)} relu(h) store = {gi + 1 + len(relu)} on every path"
            + (f"; {len(loads)} load in an arm that {'drains the queue itself (vmcnt(0) behind it, in front of the vmcnt(5))' if drained else 'DOES NOT drain'}" if loads else "")
            + (f"; {rest} UNCLASSIFIED" if rest else ""))


def main(old_dir, new_dir):
    for f in FILES:
        old, new = kernels(f"{old_dir}/{f}.s"), kernels(f"{new_dir}/{f}.s")
        names = demangle(sorted(set(old) | set(new)))
        print(f"\n### {f}.hip: {len(old)} kernels in the parent, {len(new)} in the tree\n")
        print("| kernel | VGPR | AGPR | SGPR | scratch | spills s/v | " + " | ".join(c for c, _ in COUNTS) + " | lines | stream |")
        print("|---|---|---|---|---|---|" + "---|" * len(COUNTS) + "---|---|")
        verdicts = collections.Counter()
        for k in sorted(set(old) & set(new), key=lambda k: names[k]):
            o, n = old[k], new[k]

            def both(a, b):
                return str(a) if a == b else f"**{a} -> {b}**"
            cells = [both(o["meta"][x], n["meta"][x]) for x in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size")]
            cells.append(both("%d/%d" % (o["meta"]["sgpr_spill_count"], o["meta"]["vgpr_spill_count"]),
                              "%d/%d" % (n["meta"]["sgpr_spill_count"], n["meta"]["vgpr_spill_count"])))
            cells += [both(count(o["ins"], p), count(n["ins"], p)) for _, p in COUNTS]
            cells.append(both(len(o["ins"]), len(n["ins"])))
            o["ins"], n["ins"] = [LABEL.sub(".LBB_", i) for i in o["ins"]], [LABEL.sub(".LBB_", i) for i in n["ins"]]
            if o["ins"] == n["ins"]:
                v = "identical"
            elif norm(o["ins"]) == norm(n["ins"]):
                v = "identical up to register names"
            else:
                sm = difflib.SequenceMatcher(None, [i.split()[0] for i in o["ins"]], [i.split()[0] for i in n["ins"]], autojunk=False)
                moved = sum(max(i2 - i1, j2 - j1) for tag, i1, i2, j1, j2 in sm.get_opcodes() if tag != "equal")
                v = f"differs: {moved} of {len(o['ins'])} instructions moved or changed"
            verdicts[v.split(":")[0]] += 1
            print(f"| `{short(names[k])}` | " + " | ".join(cells) + f" | {v} |")
        print("\n" + ", ".join(f"{n} {v}" for v, n in verdicts.items()) + ".")
        gone, came = sorted(set(old) - set(new), key=lambda k: names[k]), sorted(set(new) - set(old), key=lambda k: names[k])
        if gone:
            print(f"\nRemoved ({len(gone)}):\n")
            for k in gone:
                print(f"- `{short(names[k])}`")
        if came:
            print(f"\nNew ({len(came)}):\n")
            for k in came:
                print(f"- `{short(names[k])}`")
        mt = [k for k in sorted(new, key=lambda k: names[k]) if "mt_kernel" in names[k]]
        if mt:
            print("\nMulti-tile kernels, vector-memory instructions between the end of a gather prefetch and the next `s_waitcnt vmcnt(5)`, "
                  "per window in layout order and split by path (the tree; the parent's windows are compared instruction by instruction):\n")
            for k in mt:
                wn, wo = prefetch_windows(new[k]["ins"]), prefetch_windows(old[k]["ins"]) if k in old else None
                same = "windows identical to the parent's" if wo is not None and [norm(w) for w in wo] == [norm(w) for w in wn] else "WINDOWS DIFFER from the parent's"
                print(f"- `{short(names[k])}` ({same}):")
                for w in wn:
                    print(f"  - {window_by_path(w)}")

if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
