#!/usr/bin/env python3
"""The v_mov_b32 of a fused kernel, per BLOCK of its loop, with the source line each of them comes from -- and the registers of every fused kernel.

    python scripts/isa_moves.py [--kernel k_fusedILi0ELb1E] [--csrc DIR] [--extra "-DX ..."] [--json FILE --tag parent|tree]
    python scripts/isa_moves.py --regs [--csrc DIR]

scripts/isa_regions.py says how many instructions a block of the loop is; it does not say which of them the result needs.  A move computes
nothing: it is a zero-fill, a copy the source forces on the register allocator, or a constant.  This script reads the SAME compile as
isa_regions.py (fused.hip to gfx950 assembly with the flags of csrc/Makefile plus -gline-tables-only, its opcode sequence checked against the plain
listing), gives every instruction the block isa_regions.classify gives it, and lists the v_mov_b32 with the file and line of their `.loc` and
whether they are inside the persistent loop.  It looks for nothing but opcodes and `.loc`.

--csrc: another copy of csrc/ (the parent commit's, for a before / after); --regs: VGPRs, scratch and spilled registers of every kernel of
fused.hip and fused_guided.hip, from the listings' metadata; --json: the move table, the per-block VALU / SALU counts and the registers, stored
under --tag in FILE (profiles/fused_moves_isa_blocks.json).
"""
import argparse
import collections
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_regions as ir  # noqa: E402


def located(body, files):
    """-> [(opcode, file, line)] of the kernel's instructions, in the order isa_regions.classify walks them"""
    out, loc = [], None
    for l in body:
        t = l.strip()
        m = re.match(r"^\.loc\s+(\d+)\s+(\d+)", t)
        if m:
            loc = (files.get(int(m.group(1)), "?"), int(m.group(2)))
            continue
        if re.match(r"^(\.LBB\d+_\d+):", t) or re.match(r"^; %bb\.\d+:", t) or not t or t.startswith((";", ".")):
            continue
        out.append((t.split()[0], *(loc or ("?", 0))))
    return out


def registers(csrc, extra):
    """-> {kernel: {vgprs, scratch, sgpr_spills, vgpr_spills}} of fused.hip and fused_guided.hip"""
    regs = {}
    for src in ("fused.hip", "fused_guided.hip"):
        out = f"/tmp/isa_moves_{src}.s"
        subprocess.check_call(["/opt/rocm/bin/hipcc", *ir.FLAGS, *extra, "-S", "--cuda-device-only", os.path.join(csrc, src), "-o", out], stderr=subprocess.DEVNULL)
        name = None
        for l in open(out):
            m = re.match(r"^\s+\.(name|vgpr_count|sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size):\s+(\S+)", l)
            if not m:
                continue
            if m.group(1) == "name":
                k = re.search(r"(k_fused\w*?)I(.*?)EEv", m.group(2))
                name = f"{k.group(1)}<{k.group(2)}>".replace("Li", "").replace("Lb", "").replace("E", ",").rstrip(",>") + ">" if k else None
                if name:
                    regs[name] = {}
            elif name:
                regs[name][{"vgpr_count": "vgprs", "sgpr_spill_count": "sgpr_spills", "vgpr_spill_count": "vgpr_spills",
                            "private_segment_fixed_size": "scratch"}[m.group(1)]] = int(m.group(2))
    return regs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", default="k_fusedILi0ELb1E")
    ap.add_argument("--csrc", default=ir.CSRC)
    ap.add_argument("--extra", default="")
    ap.add_argument("--regs", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--tag", default="tree")
    a = ap.parse_args()
    ir.CSRC = os.path.abspath(a.csrc)
    extra = a.extra.split()
    regs = registers(ir.CSRC, extra) if (a.regs or a.json) else {}
    if a.regs:
        print(f"{'kernel':28s} {'VGPRs':>5s} {'scratch':>7s} {'SGPR spills':>11s} {'VGPR spills':>11s}")
        for k in sorted(regs):
            r = regs[k]
            print(f"{k:28s} {r['vgprs']:5d} {r['scratch']:7d} {r['sgpr_spills']:11d} {r['vgpr_spills']:11d}")
        if not a.json:
            return
    plain = ir.kernel_body(ir.compile_s(extra, False), a.kernel)
    dbg_lines = ir.compile_s(extra, True)
    dbg = ir.kernel_body(dbg_lines, a.kernel)
    if ir.opcodes(plain) != ir.opcodes(dbg):
        sys.exit("the -gline-tables-only listing's opcode sequence differs from the plain one: cannot attribute")
    files = {}
    for l in dbg_lines:
        m = re.match(r'^\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]+)"', l)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(2))
    totals, bbs = ir.classify(dbg, files, ir.marker_regions(os.path.join(ir.CSRC, "fused_kernel.h")), ir.pair_leaf_regions(os.path.join(ir.CSRC, "pair_leaf.h")),
                              ir.slow_divide_lines(os.path.join(ir.CSRC, "pt_math.h")))
    locs = located(dbg, files)
    # (the staging loops in front of the persistent loop are loops to LLVM too: what classify calls PROLOGUE is outside)
    flat = [(b or maj, in_loop and (b or maj) != "PROLOGUE") for (_, maj, _, _), (_, ins, in_loop) in zip(bbs, ir.classify.last_bbs) for _, b, _ in ins]
    if [op for _, ins, _ in ir.classify.last_bbs for op, _, _ in ins] != [op for op, _, _ in locs]:
        sys.exit("isa_moves: the two walks of the listing disagree")
    moves = collections.defaultdict(collections.Counter)   # (block, in_loop) -> Counter("file:line")
    n_valu = n_mov = 0
    for (op, f, line), (blk, in_loop) in zip(locs, flat):
        n_valu += op.startswith("v_")
        if op.startswith("v_mov_b32"):
            n_mov += 1
            moves[(str(blk), in_loop)][f"{f}:{line}" if line else "(no line)"] += 1
    in_loop_n = sum(sum(c.values()) for (b, il), c in moves.items() if il)
    print(f"{a.kernel}: {n_valu} VALU instructions, {n_mov} of them v_mov_b32: {n_mov - in_loop_n} before or behind the loop, {in_loop_n} inside it")
    for il, head in ((True, "inside the persistent loop"), (False, "outside the loop (once per wave)")):
        print(f"-- {head}")
        for (b, l2), c in sorted(moves.items(), key=lambda kv: -sum(kv[1].values())):
            if l2 == il:
                print(f"  {b:10s} {sum(c.values()):3d}   " + ", ".join(f"{k} x{v}" if v > 1 else k for k, v in sorted(c.items())))
    if a.json:
        doc = json.load(open(a.json)) if os.path.exists(a.json) else {}
        entry = doc.setdefault(a.tag, {})
        entry.setdefault("kernels", {})[a.kernel] = {
            "valu": n_valu, "v_mov_b32": n_mov, "v_mov_b32_in_loop": in_loop_n,
            "moves_in_loop": {b: dict(c) for (b, il), c in sorted(moves.items()) if il},
            "blocks": {str(b): {"valu": totals[b]["valu"], "salu": totals[b]["salu"]} for b in ["PROLOGUE", *ir.BLOCKS] if b in totals}}
        entry["registers"] = regs
        json.dump(doc, open(a.json, "w"), indent=1)
        print("wrote", a.json, "tag", a.tag)


if __name__ == "__main__":
    main()
