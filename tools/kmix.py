#!/usr/bin/env python3
"""Static instruction mix of chosen kernels in two assembly listings, side by side (parent -> new).

usage: tools/kmix.py <parent engine.s> <new engine.s> <name-filter> [name-filter ...]
Per kernel: VGPRs, scratch bytes per lane, waves per SIMD (512 VGPRs, granule 8), the VALU instruction count and the
opcodes the integer arithmetic is made of.  Loops count once (see tools/kres.py).
"""
import re
import subprocess
import sys

OPS = ["v_mad_u64_u32", "v_mov_b32", "v_lshl_add_u64", "v_lshrrev_b64", "v_cndmask_b32", "v_mul_lo_u32", "v_addc_co_u32",
       "v_alignbit_b32", "s_nop"]


def load(path):
    body, meta, entries, cur = {}, {}, [], None
    label = re.compile(r"^(_Z\w+):")
    for line in open(path):
        m = label.match(line)
        if m:
            cur = m.group(1)
            body[cur] = dict.fromkeys(OPS + ["valu"], 0)
            continue
        s = line.strip()
        if line.startswith("  - ."):
            entries.append({})
            s = s[2:]
        if entries and cur is None and s.startswith("."):
            k, _, v = s.partition(":")
            if k == ".name":
                entries[-1][k] = v.strip()
            elif k in (".vgpr_count", ".private_segment_fixed_size"):
                entries[-1][k] = int(v)
        if cur is None or not s or s.startswith((".", ";")):
            if s.startswith((".end_amdhsa_kernel", ".Lfunc_end")):
                cur = None
            continue
        op = s.split()[0]
        if op.startswith("v_"):
            body[cur]["valu"] += 1
        for o in OPS:
            if op == o or op.startswith(o + "_e"):
                body[cur][o] += 1
    for e in entries:
        if e.get(".name") in body:
            meta[e[".name"]] = e
    return body, meta


def main():
    a_body, a_meta = load(sys.argv[1])
    b_body, b_meta = load(sys.argv[2])
    filters = sys.argv[3:]
    names = [n for n in a_meta if n in b_meta]
    pretty = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    rows = []
    for n, p in zip(names, pretty):
        p = re.sub(r"\(.*$", "", re.sub(r"^void ", "", p))
        if any(f in p for f in filters):
            rows.append((p, n))
    cols = ["vgpr", "scr", "w", "valu"] + [o[2:] for o in OPS]
    print(f"{'kernel (parent -> new)':44s} " + " ".join(f"{c:>11s}" for c in cols))
    for p, n in sorted(rows):
        def waves(v):
            return min(8, 512 // ((v + 7) // 8 * 8)) if v else 8
        va, vb = a_meta[n].get(".vgpr_count", 0), b_meta[n].get(".vgpr_count", 0)
        pairs = [(va, vb), (a_meta[n].get(".private_segment_fixed_size", 0), b_meta[n].get(".private_segment_fixed_size", 0)),
                 (waves(va), waves(vb)), (a_body[n]["valu"], b_body[n]["valu"])] + [(a_body[n][o], b_body[n][o]) for o in OPS]
        print(f"{p[:44]:44s} " + " ".join(f"{x:>5d}>{y:<5d}" for x, y in pairs))


if __name__ == "__main__":
    main()
