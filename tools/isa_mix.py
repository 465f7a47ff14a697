#!/usr/bin/env python3
"""Instruction mix of one kernel (or one loop of it) in hipcc's -S output; needs no GPU.

    hipcc ... --cuda-device-only -S encode_launch.hip -o k3_t8.s
    tools/isa_mix.py k3_t8.s _ZN5pqhip15k_encode_mfma16ILi8ELi20EhEEvNS_10EncodeArgsE --loop auto
    tools/isa_mix.py k3_t8.s k_encode_mfma16ILi8ELi20Eh --lines 640:1900

The kernel is named by its symbol (or a unique substring of it).  Without --loop / --lines the whole kernel body is
counted.  --loop LABEL counts from that label (e.g. .LBB11_25) to the last branch back to it; --loop auto takes the
loop with the most matrix instructions.  --lines A:B counts lines A..B of the file (1-based, inclusive) that lie in
the kernel.  Inline-asm lines count like any other instruction.

Printed: instructions per class (matrix, other vector, scalar, LDS, global / buffer memory, waits, s_nop), the
s_nop wait states, the s_nop that directly follow a matrix instruction (an MFMA whose result is read next), and every
mnemonic with its count.
"""
import argparse
import collections
import re
import sys


def kernel_lines(lines, sym):
    """(first, last) 0-based line indices of the body of the function whose symbol matches `sym`."""
    starts = [i for i, l in enumerate(lines) if re.match(r"^[A-Za-z_.$][\w.$]*:", l) and not l.startswith(".")]
    hits = [i for i in starts if lines[i].split(":")[0] == sym] or [i for i in starts if sym in lines[i].split(":")[0]]
    if len(hits) != 1:
        names = [lines[i].split(":")[0] for i in hits]
        sys.exit("isa_mix: symbol %r matches %d functions%s" % (sym, len(hits), (": " + ", ".join(names)) if names else ""))
    first = hits[0]
    last = len(lines) - 1
    for i in range(first + 1, len(lines)):
        if lines[i].lstrip().startswith("s_endpgm") or lines[i].startswith(".Lfunc_end"):
            last = i
            break
    return first, last


def instr(line):
    """mnemonic of an instruction line, or None for labels, directives, comments and blanks"""
    s = line.split(";")[0].strip()
    if not s or s.endswith(":") or s.startswith("."):
        return None
    return s.split()[0]


def klass(mn):
    if mn.startswith("v_mfma") or mn.startswith("v_smfmac"):
        return "matrix"
    if mn == "s_nop":
        return "s_nop"
    if mn.startswith("s_waitcnt"):
        return "wait"
    if mn.startswith("ds_"):
        return "lds"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if mn.startswith("s_load") or mn.startswith("s_buffer_load"):
        return "smem"
    if mn.startswith("v_"):
        return "vector"
    if mn.startswith("s_"):
        return "scalar"
    return "other"


def find_loop(lines, first, last, label):
    labels = {}
    for i in range(first, last + 1):
        m = re.match(r"^(\.LBB\w+):", lines[i])
        if m:
            labels[m.group(1)] = i
    loops = []
    for lab, li in labels.items():
        back = [i for i in range(li + 1, last + 1) if re.match(r"^\s*s_(cbranch_\w+|branch)\s+%s\s*$" % re.escape(lab), lines[i].split(";")[0])]
        if back:
            loops.append((lab, li, back[-1]))
    if label == "auto":
        if not loops:
            sys.exit("isa_mix: no loop in the kernel")
        mf = lambda lp: sum(1 for i in range(lp[1], lp[2] + 1) if (instr(lines[i]) or "").startswith("v_mfma"))
        return max(loops, key=mf)
    for lp in loops:
        if lp[0] == label:
            return lp
    sys.exit("isa_mix: %s is not a loop header in this kernel (loops: %s)" % (label, ", ".join(l[0] for l in loops)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm", help="hipcc -S output (.s)")
    ap.add_argument("symbol", help="kernel symbol or a unique substring of it")
    g = ap.add_mutually_exclusive_group()
    g.add_argument("--loop", help="loop header label (.LBBx_y), or 'auto' for the loop with the most MFMAs")
    g.add_argument("--lines", help="A:B, 1-based inclusive line range of the file")
    ap.add_argument("--top", type=int, default=0, help="print only the N most frequent mnemonics (default: all)")
    args = ap.parse_args()

    lines = open(args.asm).read().split("\n")
    first, last = kernel_lines(lines, args.symbol)
    lo, hi, what = first, last, "whole kernel"
    if args.loop:
        lab, lo, hi = find_loop(lines, first, last, args.loop)
        what = "loop %s" % lab
    elif args.lines:
        a, b = (int(v) for v in args.lines.split(":"))
        lo, hi = max(first, a - 1), min(last, b - 1)
        what = "lines %d..%d" % (lo + 1, hi + 1)

    mix = collections.Counter()
    cls = collections.Counter()
    nop_states = 0
    nop_after_mfma = 0
    nop_after_mfma_states = 0
    prev = None
    for i in range(lo, hi + 1):
        mn = instr(lines[i])
        if mn is None:
            continue
        mix[mn] += 1
        c = klass(mn)
        cls[c] += 1
        if mn == "s_nop":
            n = int(lines[i].split(";")[0].split()[1], 0) + 1
            nop_states += n
            if prev is not None and prev.startswith("v_mfma"):
                nop_after_mfma += 1
                nop_after_mfma_states += n
        prev = mn

    print("%s, %s: lines %d..%d of %s" % (lines[first].split(":")[0], what, lo + 1, hi + 1, args.asm))
    total = sum(mix.values())
    print("instructions %d: matrix %d, other vector %d, scalar %d, LDS %d, vmem %d, smem %d, waits %d, s_nop %d"
          % (total, cls["matrix"], cls["vector"], cls["scalar"], cls["lds"], cls["vmem"], cls["smem"], cls["wait"], cls["s_nop"]))
    print("s_nop wait states %d; s_nop right after a matrix instruction: %d (%d wait states)"
          % (nop_states, nop_after_mfma, nop_after_mfma_states))
    items = mix.most_common(args.top or None)
    w = max(len(k) for k, _ in items) if items else 0
    for k, v in items:
        print("  %-*s %5d" % (w, k, v))


if __name__ == "__main__":
    main()
