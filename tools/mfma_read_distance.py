#!/usr/bin/env python3
"""Wait states between every matrix instruction of a kernel and the first later use of its result registers, in
hipcc's -S output; needs no GPU.

    hipcc ... --cuda-device-only -S encode_launch.hip -o k3_t8.s
    tools/mfma_read_distance.py k3_t8.s _ZN5pqhip15k_encode_mfma16ILi8ELi20EhEEvNS_10EncodeArgsE [--need 12]

gfx9 has no interlock between a matrix instruction's write of its result and a vector instruction that reads it: the
compiler inserts the wait states (s_nop), but only in front of instructions it issues itself.  A kernel that feeds
accumulators straight into inline assembly has to keep the distance by its own schedule; this tool measures it.  For
every v_mfma the text is followed in program order (branches not taken, at most --window instructions) to the first
instruction that names one of its result registers; the distance is the number of instructions in between, an
s_nop N counting N + 1 and everything else 1 (an under-estimate: a matrix instruction holds the issue for longer).
Uses inside inline assembly (between ASMSTART and ASMEND) and by the compiler's own instructions are reported apart;
the exit status is 1 when a use inside inline assembly is nearer than --need."""
import argparse
import re
import sys

from isa_mix import instr, kernel_lines


def regs(text):
    """set of VGPR numbers named in an instruction's operands"""
    out = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", text):
        out.update(range(int(a), int(b) + 1))
    out.update(int(a) for a in re.findall(r"\bv(\d+)\b", text))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("asm")
    ap.add_argument("symbol")
    ap.add_argument("--need", type=int, default=12, help="wait states an inline-assembly use must keep (default 12: what the compiler keeps for an 8-pass result on gfx950, passes + 4)")
    ap.add_argument("--window", type=int, default=120)
    args = ap.parse_args()
    lines = open(args.asm).read().split("\n")
    first, last = kernel_lines(lines, args.symbol)
    prog = []                                                    # (mnemonic, operand text, in inline assembly)
    in_asm = False
    for i in range(first, last + 1):
        if "#ASMSTART" in lines[i]:
            in_asm = True
        elif "#ASMEND" in lines[i]:
            in_asm = False
        mn = instr(lines[i])
        if mn is not None:
            prog.append((mn, lines[i].split(";")[0], in_asm, i + 1))
    worst = {True: None, False: None}
    n_mfma = 0
    near = 0
    for k, (mn, text, _, line) in enumerate(prog):
        if not mn.startswith("v_mfma"):
            continue
        n_mfma += 1
        dst = regs(text.split(",")[0])
        dist = 0
        for mn2, text2, asm2, line2 in prog[k + 1:k + 1 + args.window]:
            if regs(text2) & dst:
                if worst[asm2] is None or dist < worst[asm2][0]:
                    worst[asm2] = (dist, line, line2)
                if asm2 and dist < args.need:
                    near += 1
                break
            dist += (int(text2.split()[1], 0) + 1) if mn2 == "s_nop" else 1
    print("%s: %d matrix instructions" % (lines[first].split(":")[0], n_mfma))
    for asm2, what in ((True, "inline assembly"), (False, "the compiler's instructions")):
        w = worst[asm2]
        print("  nearest use by %s: %s" % (what, "none in the window" if w is None else
                                          "%d wait states (matrix instruction at line %d, use at line %d)" % w))
    print("  uses by inline assembly nearer than %d: %d" % (args.need, near))
    return 1 if near else 0


if __name__ == "__main__":
    sys.exit(main())
