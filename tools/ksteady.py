#!/usr/bin/env python3
"""Per-kernel time per step over the warm steps of two rocprofv3 --kernel-trace runs of bench.py, joined by kernel.

usage: tools/ksteady.py <base_dir> <new_dir> <steps_in_run> [first_warm_step]
The mk:: dispatches of a run (k_pack_rowb excluded: context creation) in start order are cut into `steps` equal groups, as
tools/kstats.py does; per step a kernel's calls are added up.  Columns: average, fastest and slowest step of each run over
steps first_warm_step .. steps - 1 (default 6), their ratio, and the verdict: new's slowest step below base's fastest,
above base's slowest, or inside.  Kernels of one run only are listed with the other side empty.
"""
import csv
import glob
import re
import sys


def short(name):
    m = re.search(r"(mk::[A-Za-z0-9_]+(?:<[^>(]*>)?)", name)
    return m.group(1) if m else name[:60]


def per_step(d, steps, first):
    files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    if not files:
        sys.exit("no *kernel_trace.csv under " + d)
    ev = []
    for r in csv.DictReader(open(files[0])):
        if "mk::" in r["Kernel_Name"] and "k_pack_rowb" not in r["Kernel_Name"]:
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    ev.sort()
    if not ev or len(ev) % steps:
        sys.exit(f"{d}: {len(ev)} mk:: dispatches do not divide into {steps} equal steps")
    per = len(ev) // steps
    out, walls = {}, []
    for i in range(first, steps):
        g = ev[i * per:(i + 1) * per]
        walls.append((max(e for _, e, _ in g) - g[0][0]) / 1e3)
        t, n = {}, {}
        for s, e, k in g:
            t[k] = t.get(k, 0.0) + (e - s) / 1e3
            n[k] = n.get(k, 0) + 1
        for k in t:
            out.setdefault(k, (n[k], []))[1].append(t[k])
    return out, walls, per


def main():
    base_dir, new_dir, steps = sys.argv[1], sys.argv[2], int(sys.argv[3])
    first = int(sys.argv[4]) if len(sys.argv) > 4 else 6
    base, bw, bper = per_step(base_dir, steps, first)
    new, nw, nper = per_step(new_dir, steps, first)
    for tag, w, per in (("base", bw, bper), ("new ", nw, nper)):
        print(f"# {tag}: {per} mk:: kernels per step; wall per step over steps {first}..{steps - 1}: avg {sum(w) / len(w):.1f} us, "
              f"min {min(w):.1f}, max {max(w):.1f}")
    print(f"{'kernel':46s} {'calls':>9s} | {'base avg_us':>11s} {'min_us':>8s} {'max_us':>8s} | {'new avg_us':>11s} {'min_us':>8s} "
          f"{'max_us':>8s} | {'new/base':>8s}  verdict")
    keys = sorted(set(base) | set(new), key=lambda k: -max(sum(x[k][1]) / len(x[k][1]) if k in x else 0.0 for x in (base, new)))
    tot = {"base": 0.0, "new": 0.0}
    for k in keys:
        b, n = base.get(k), new.get(k)
        cells = []
        for x in (b, n):
            cells.append(f"{sum(x[1]) / len(x[1]):11.2f} {min(x[1]):8.2f} {max(x[1]):8.2f}" if x else f"{'':11s} {'':8s} {'':8s}")
        calls = "/".join(str(x[0]) if x else "-" for x in (b, n))
        ratio = verdict = ""
        if b and n:
            ratio = f"{(sum(n[1]) / len(n[1])) / (sum(b[1]) / len(b[1])):8.3f}"
            verdict = "below base min" if max(n[1]) < min(b[1]) else "above base max" if min(n[1]) > max(b[1]) else "inside"
        tot["base"] += sum(b[1]) / len(b[1]) if b else 0.0
        tot["new"] += sum(n[1]) / len(n[1]) if n else 0.0
        print(f"{k:46s} {calls:>9s} | {cells[0]} | {cells[1]} | {ratio:>8s}  {verdict}")
    print(f"# sum of the averages: base {tot['base']:.1f} us, new {tot['new']:.1f} us")


if __name__ == "__main__":
    main()
