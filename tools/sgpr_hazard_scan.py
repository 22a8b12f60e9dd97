#!/usr/bin/env python3
"""Wait states between a vector instruction that writes a scalar register and a vector instruction that reads it.

usage: tools/sgpr_hazard_scan.py [engine.s]        (make -C ppqsflhe_amd/csrc asm writes engine.s)

gfx90a and later want two wait states between a VALU instruction that writes an SGPR or vcc (a carry-out, a compare, a
v_readfirstlane) and a VALU instruction that reads that register (a carry-in, a select, a scalar operand).  hipcc pads
its own instructions with s_nop; it does not look inside an inline-asm string, and modarith.hpp takes the carry-out of
v_mad_u64_u32 and feeds v_addc_co_u32 from asm statements (mad_u64_cy, add_cy, mac128).  This script walks every
kernel of an assembly listing, counts the wait states (instructions issued in between, s_nop N counting N + 1) for each
such pair and prints the pairs with fewer than two; exit status 1 if there are any.  On a listing without inline asm it
reports nothing, which is the check of the rule itself against the compiler's own padding.
"""
import re
import sys

SREG = re.compile(r"(\bvcc\b|\bs\[(\d+):(\d+)\]|\bs(\d+)\b)")
CARRY_OUT = ("v_mad_u64_u32", "v_mad_i64_i32", "v_add_co", "v_addc_co", "v_sub_co", "v_subb_co", "v_subrev_co",
             "v_subbrev_co", "v_div_scale")
IMPLICIT_VCC_IN = ("v_addc_co", "v_subb_co", "v_subbrev_co", "v_cndmask")
NOT_A_WRITE = ("s_waitcnt", "s_cbranch", "s_branch", "s_barrier", "s_endpgm", "s_nop", "s_cmp", "s_bitcmp")
VCC = {106, 107}


def regs(text):
    out = set()
    for m in SREG.finditer(text):
        if m.group(1) == "vcc":
            out |= VCC
        elif m.group(2):
            out |= set(range(int(m.group(2)), int(m.group(3)) + 1))
        else:
            out.add(int(m.group(4)))
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else "ppqsflhe_amd/csrc/engine.s"
    label = re.compile(r"^(_Z\w+):")
    kern, hist, pos, in_asm = None, [], 0, False
    found = pairs = 0
    for line in open(path):
        m = label.match(line)
        if m:
            kern, hist, pos = m.group(1), [], 0
            continue
        s = line.strip()
        if s.startswith(";;#ASMSTART"):
            in_asm = True
            continue
        if s.startswith(";;#ASMEND"):
            in_asm = False
            continue
        if not s or s.startswith((".", ";")) or s.endswith(":"):
            continue
        s = s.split(";")[0].strip()
        if not s:
            continue
        op = s.split()[0]
        ops = [o.strip() for o in s[len(op):].split(",")]
        if op == "s_nop":
            pos += int(ops[0]) + 1
            continue
        if op.startswith("v_"):
            written, srcs = set(), ops[1:]
            if op.startswith(CARRY_OUT):
                written, srcs = regs(ops[1]), ops[2:]
            elif op.startswith(("v_cmp", "v_readfirstlane", "v_readlane")):
                written, srcs = regs(ops[0]), ops[1:]
            read = set()
            for o in srcs:
                read |= regs(o)
            if "_e32" in op and op.startswith(IMPLICIT_VCC_IN):
                read |= VCC
            for p, w, text, asm in hist[-3:]:
                if w & read:
                    pairs += 1
                    if pos - p - 1 < 2:
                        found += 1
                        print(f"{kern}: {pos - p - 1} wait state(s): [{text}] -> [{s}]" + (" (inline asm)" if asm or in_asm else ""))
            hist.append((pos, written, s, in_asm))
        elif op.startswith("s_") and not op.startswith(NOT_A_WRITE) and ops:
            w = regs(ops[0])  # a scalar instruction's own write ends the hazard on that register
            hist = [(p, ww - w, t, a) for p, ww, t, a in hist]
        pos += 1
    print(f"{found} pair(s) with fewer than two wait states ({pairs} write -> read pairs within three instructions)")
    return 1 if found else 0


if __name__ == "__main__":
    sys.exit(main())
