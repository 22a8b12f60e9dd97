#!/usr/bin/env python3
"""A/B of the distribution leg: the full fan-out at the aggregate's level (arm A, mkckks_reencrypt_fanout_batch at nl_in)
against the compact fan-out written at k limbs (arm B, mkckks_reencrypt_fanout_compact_batch at k = 1 and k = 2).

usage: tools/bench_compact_back.py [--shape n16|n17|all] [--blocks 7] [--block-seconds 0.5]
       tools/bench_compact_back.py --profile-arm-b --shape n16 [--limbs 1]   # a few arm-B passes only, to run under
                                                        # rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python ...
       tools/bench_compact_back.py --stats <rocprof_out_dir>                # arm B's kernel time by kernel

Shapes: n16 = Context(16, 10, 50, 60, dnum=3), nl_in = 11, B = 16, n_keys = 7 (the back leg of the headline workload);
        n17 = Context(17, 18, 50, 60, dnum=3), nl_in = 19, B = 8, n_keys = 7.
All arms run in one process on the same device arrays with every key already in HBM, warmed, in alternating blocks
(A, B1, B2, A, B1, B2, ...) of at least --block-seconds each; wall time between device synchronisations.  Before anything
is timed arm B is compared word for word with the composition on the device (packed copy of the prefix -> reencrypt_fanout
at k + 1 -> rescale); a mismatch or a missing device ends the run with a non-zero status.
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_fanout import SHAPES, make_inputs  # noqa: E402

KS = (1, 2)


def composition(g, d_evks, ct, n_keys, k):
    B, nl = ct.shape[0], k + 1
    d_pre = g.to_device(np.ascontiguousarray(ct[:, :, :nl]))
    d_ks = g.empty((n_keys, B, 2, nl, g.N))
    g.reencrypt_fanout(d_pre, d_evks, d_ks, n_keys, B, nl)
    d_out = g.empty((n_keys * B, 2, k, g.N))
    g.rescale(d_ks, d_out, n_keys * B, nl)
    return d_out.to_host().reshape(n_keys, B, 2, k, g.N)


def run_ab(shape, blocks, block_s, out):
    from ppqsflhe_amd import Context
    args, nl, B, n_keys = SHAPES[shape]
    g = Context(*args[:4], dnum=args[4], device=0)  # raises without a device: no fallback
    ct, evks = make_inputs(g, nl, B, n_keys, 2024)
    d_ct, d_evks = g.to_device(ct), g.to_device(evks)
    d_a = g.empty((n_keys, B, 2, nl, g.N))
    d_b = {k: g.empty((n_keys, B, 2, k, g.N)) for k in KS}
    arms = {"A": lambda: g.reencrypt_fanout(d_ct, d_evks, d_a, n_keys, B, nl)}
    for k in KS:
        arms[f"B{k}"] = (lambda k: lambda: g.reencrypt_fanout_compact(d_ct, d_evks, d_b[k], n_keys, B, nl, k))(k)
    for fn in arms.values():
        fn()
    g.sync()
    for k in KS:
        if not np.array_equal(d_b[k].to_host(), composition(g, d_evks, ct, n_keys, k)):
            sys.exit(f"{shape} k={k}: the compact fan-out differs from prefix copy -> reencrypt_fanout -> rescale")
    for _ in range(2):
        for fn in arms.values():
            fn()
    g.sync()

    def block(fn):
        reps, t0 = 0, time.perf_counter()
        while True:
            fn()
            g.sync()
            reps += 1
            dt = time.perf_counter() - t0
            if dt >= block_s:
                return dt / reps * 1e3

    t = {name: [] for name in arms}
    for _ in range(blocks):
        for name, fn in arms.items():
            t[name].append(block(fn))
    ma = statistics.median(t["A"])
    print(f"{shape} nl_in={nl} B={B} n_keys={n_keys}: arm B == composition on all words at k = {', '.join(map(str, KS))}", file=out)
    per_client = lambda limbs: B * (48 + 16 * limbs * g.N)  # noqa: E731  (blob = 48-byte header + 2 x limbs x N words)
    print(f"  arm A  (reencrypt_fanout at {nl} limbs):          median {ma:.3f} ms  min {min(t['A']):.3f}  max {max(t['A']):.3f}  "
          f"({n_keys * B / ma * 1e3:.0f} ct/s)  {per_client(nl) / 1048576:.2f} MiB written per client", file=out)
    for k in KS:
        tb = t[f"B{k}"]
        mb = statistics.median(tb)
        print(f"  arm B{k} (reencrypt_fanout_compact to {k} limb{'s' if k > 1 else ' '}): median {mb:.3f} ms  min {min(tb):.3f}  max {max(tb):.3f}  "
              f"({n_keys * B / mb * 1e3:.0f} ct/s)  {per_client(k) / 1048576:.2f} MiB written per client", file=out)
        print(f"         A / B{k} = {ma / mb:.2f} x  (A - B{k} = {ma - mb:.3f} ms, arm A spread {max(t['A']) - min(t['A']):.3f} ms, "
              f"arm B{k} spread {max(tb) - min(tb):.3f} ms; payload {nl / k:.1f} x smaller)", file=out)
    print(f"  {blocks} alternating blocks per arm of >= {block_s} s", file=out)
    out.flush()
    g.close()


def profile_arm_b(shape, k):
    from ppqsflhe_amd import Context
    args, nl, B, n_keys = SHAPES[shape]
    g = Context(*args[:4], dnum=args[4], device=0)
    ct, evks = make_inputs(g, nl, B, n_keys, 2024)
    d_ct, d_evks, d_b = g.to_device(ct), g.to_device(evks), g.empty((n_keys, B, 2, k, g.N))
    for _ in range(5):
        g.reencrypt_fanout_compact(d_ct, d_evks, d_b, n_keys, B, nl, k)
    g.sync()
    g.close()


def stats(prof_dir, out):
    files = glob.glob(prof_dir + "/**/*kernel_stats.csv", recursive=True)
    if not files:
        sys.exit("no *kernel_stats.csv under " + prof_dir)
    rows, tot = [], 0.0
    for r in csv.DictReader(open(files[0])):
        name, ns = r["Name"], float(r["TotalDurationNs"])
        if "mk::" not in name or "k_pack_rowb" in name:
            continue
        tot += ns
        rows.append((ns, int(r["Calls"]), name))
    print("arm B kernel time by kernel (rocprofv3 --kernel-trace --stats; share, calls, mean us per call):", file=out)
    for ns, calls, name in sorted(rows, reverse=True):
        print(f"  {100 * ns / tot:6.2f} %  {calls:4d}  {ns / calls / 1e3:8.1f}  {name[name.index('mk::'):][:96]}", file=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-seconds", type=float, default=0.5)
    ap.add_argument("--profile-arm-b", action="store_true")
    ap.add_argument("--limbs", type=int, default=1)
    ap.add_argument("--stats", default=None)
    a = ap.parse_args()
    if a.stats:
        stats(a.stats, sys.stdout)
        return
    for sh in (list(SHAPES) if a.shape == "all" else [a.shape]):
        if a.profile_arm_b:
            profile_arm_b(sh, a.limbs)
        else:
            run_ab(sh, max(7, a.blocks), max(0.5, a.block_seconds), sys.stdout)


if __name__ == "__main__":
    main()
