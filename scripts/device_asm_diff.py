#!/usr/bin/env python3
"""Device-code gate for kernel refactors: is the gfx950 assembly of two source trees the same, kernel by kernel?

    scripts/device_asm_diff.py TREE_A TREE_B [-j N] [--keep DIR] [file.hip ...]

For every .hip file of csrc/Makefile's SRCS (or the ones named) each tree is compiled with ITS Makefile's FLAGS (and
the per-file additions such as extend_hbm.o's scheduler flag) as `hipcc ... --cuda-device-only -S`.  The assembly is cut
into one piece per symbol (the function body, its .amdhsa_kernel descriptor with the register / LDS counts, its
entry in the code object's metadata), the compiler's per-function label numbers are dropped and the pieces are
compared by symbol: the order in which a translation unit emits its instantiations does not count, their set and
mangled names do.  What belongs to no function (device variables, the metadata's header) is compared as one piece,
`<file scope>`, without the per-build __hip_cuid_<hash> symbol.

Prints the files and symbols that differ; exit status 0 when there are none.  Needs hipcc, no GPU.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join("single-file-vulkan-pathtracing_amd", "csrc")
HEAD = re.compile(r"^\s*\.(globl|weak|protected|hidden|p2align|section|text)\b")
FUNC = re.compile(r"^\s*\.type\s+([^,\s]+),@function")
OBJ = re.compile(r"^\s*(\.type\s+[^,\s]+,@object|\.section\s+\.AMDGPU\.gpr_maximums)")


def makefile_recipe(tree):
    """(hipcc, [flags], [sources], {source: [extra flags]}) as csrc/Makefile states them."""
    text = open(os.path.join(tree, CSRC, "Makefile")).read()
    var = {m.group(1): m.group(2).strip() for m in re.finditer(r"^(\w+)\s*[:?]?=\s*(.*)$", text, re.M)}
    expand = lambda s: re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), s)
    extra = {m.group(1) + ".hip": expand(m.group(2)).split() for m in re.finditer(r"^(\w+)\.o:\s*FLAGS\s*\+=\s*(.*)$", text, re.M)}
    return os.environ.get("HIPCC", expand(var["HIPCC"])), expand(var["FLAGS"]).split(), var["SRCS"].split(), extra


def compile_asm(tree, src, out):
    hipcc, flags, _, extra = makefile_recipe(tree)
    cmd = [hipcc, *flags, *extra.get(src, []), "--cuda-device-only", "-S", src, "-o", out]
    r = subprocess.run(cmd, cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{tree}: {src} does not compile\n{r.stderr}")


def pieces(path):
    """{symbol: normalised text}; '<file scope>' holds what belongs to no function."""
    lines = [l.rstrip() for l in open(path) if "__hip_cuid_" not in l]
    # labels carry the function's number in the file (.LBB6_8, .Lfunc_end6, "Header=BB6_8" in the loop comments): keep the block number only
    # (and a label's length moves the comment behind it)
    lines = [re.sub(r"(\.L|\b)(BB|func_begin|func_end|tmp)\d+(_\d+)?\b", lambda m: m.group(1) + m.group(2) + (m.group(3) or ""), l) for l in lines]
    lines = [re.sub(r"\s+;", " ;", l) for l in lines]
    meta = next((i for i, l in enumerate(lines) if l.strip() == ".amdgpu_metadata"), len(lines))
    out, cur = {"<file scope>": []}, "<file scope>"
    starts = {}
    for i in range(meta):
        m = FUNC.match(lines[i])
        if m:
            j = i
            while j > 0 and HEAD.match(lines[j - 1]):
                j -= 1
            starts[j] = m.group(1)
        elif OBJ.match(lines[i]):  # a variable, or the trailer of the file: no longer the function before it
            j = i
            while j > 0 and HEAD.match(lines[j - 1]):
                j -= 1
            starts[j] = "<file scope>"
    for i in range(meta):
        if i in starts:
            cur = starts[i]
            out.setdefault(cur, [])
        out[cur].append(lines[i])
    # the metadata: one YAML list entry per kernel, keyed by its .name
    entry, in_kernels = [], False
    def flush():
        if not entry:
            return
        name = next((re.match(r"\s*\.name:\s*(\S+)", l).group(1) for l in entry if re.match(r"\s*\.name:\s*\S+", l) and l.startswith("    .name")), None)
        out.setdefault(name if name in out else "<file scope>", []).extend(entry)
        entry.clear()
    for l in lines[meta:]:
        if l.startswith("amdhsa.kernels:"):
            in_kernels = True
            out["<file scope>"].append(l)
        elif in_kernels and l.startswith("  - "):
            flush()
            entry.append(l)
        elif in_kernels and l.startswith("    "):
            entry.append(l)
        else:
            flush()
            in_kernels = False
            out["<file scope>"].append(l)
    flush()
    return {k: "\n".join(v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("files", nargs="*", help="default: every file of SRCS")
    ap.add_argument("-j", "--jobs", type=int, default=8)
    ap.add_argument("--keep", metavar="DIR", help="keep the .s files here (DIR/a, DIR/b) instead of a temporary directory")
    ap.add_argument("--show", type=int, default=0, metavar="N", help="print the first N lines of each differing symbol's unified diff")
    ap.add_argument("--reuse-a", action="store_true", help="with --keep: do not compile again what DIR/a already holds")
    a = ap.parse_args()
    trees = {"a": os.path.abspath(a.tree_a), "b": os.path.abspath(a.tree_b)}
    srcs_a, srcs_b = makefile_recipe(trees["a"])[2], makefile_recipe(trees["b"])[2]
    files = a.files or sorted(set(srcs_a) | set(srcs_b))
    tmp = None if a.keep else tempfile.TemporaryDirectory()
    root = a.keep or tmp.name
    jobs = []
    for side, tree in trees.items():
        os.makedirs(os.path.join(root, side), exist_ok=True)
        for f in files:
            if a.reuse_a and side == "a" and os.path.exists(os.path.join(root, side, f[:-4] + ".s")):
                continue
            if os.path.exists(os.path.join(tree, CSRC, f)):
                jobs.append((tree, f, os.path.join(root, side, f[:-4] + ".s")))
    with ThreadPoolExecutor(max(1, a.jobs)) as ex:
        list(ex.map(lambda j: compile_asm(*j), jobs))
    bad = 0
    for f in files:
        sa, sb = (os.path.join(root, side, f[:-4] + ".s") for side in ("a", "b"))
        if not (os.path.exists(sa) and os.path.exists(sb)):
            print(f"{f}: only in tree {'A' if os.path.exists(sa) else 'B'}")
            bad += 1
            continue
        pa, pb = pieces(sa), pieces(sb)
        diff = [(k, "only in A" if k not in pb else "only in B" if k not in pa else
                 f"differs ({sum(x != y for x, y in zip(pa[k].split(chr(10)), pb[k].split(chr(10)))) + abs(pa[k].count(chr(10)) - pb[k].count(chr(10)))} lines)")
                for k in sorted(set(pa) | set(pb)) if pa.get(k) != pb.get(k)]
        n_kern = sum(1 for k in pa if k != "<file scope>")
        print(f"{f}: {n_kern} symbols, " + ("identical" if not diff else f"{len(diff)} differ"))
        for k, why in diff:
            print(f"    {k}: {why}")
            if a.show and k in pa and k in pb:
                for l in list(difflib.unified_diff(pa[k].split("\n"), pb[k].split("\n"), "A", "B", n=1, lineterm=""))[:a.show]:
                    print("        " + l)
        bad += len(diff)
    print("device code identical" if not bad else f"{bad} differences")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
