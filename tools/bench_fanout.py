#!/usr/bin/env python3
"""A/B of the distribution leg: a loop of n_keys single-key re-encryptions (arm A) against one fan-out call (arm B).

usage: tools/bench_fanout.py [--shape n16|n17|all] [--groups 1,2,4,7] [--blocks 7] [--block-seconds 0.5]
       tools/bench_fanout.py --profile-arm-a --shape n16      # a few arm-A passes only, to run under
                                                              # rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python ...
       tools/bench_fanout.py --share <rocprof_out_dir> --shape n16   # f = key-independent share of arm A's kernel time

Shapes: n16 = Context(16, 10, 50, 60, dnum=3), nl = 11, B = 16, n_keys = 7 (the back leg of the headline workload);
        n17 = Context(17, 18, 50, 60, dnum=3), nl = 19, B = 8, n_keys = 7.
Both arms run in one process on the same device arrays with every key already in HBM, warmed, in alternating blocks
(A, B, A, B, ...) of at least --block-seconds each; wall time between device synchronisations.  B is compared with A
word for word before anything is timed; a mismatch or a missing device ends the run with a non-zero status.
MKCKKS_FANOUT_GROUP is read when a context is created, so every group gets a context of its own.
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

SHAPES = {"n16": ((16, 10, 50, 60, 3), 11, 16, 7), "n17": ((17, 18, 50, 60, 3), 19, 8, 7)}


def make_inputs(g, nl, B, n_keys, seed):
    rng = np.random.default_rng(seed)

    def polys(ids, lead):
        out = np.empty(lead + (len(ids), g.N), dtype=np.uint64)
        for j, l in enumerate(ids):
            out[..., j, :] = rng.integers(0, int(g.moduli[l]), size=lead + (g.N,), dtype=np.uint64)
        return out

    ct = polys(list(range(nl)) * 2, (B,)).reshape(B, 2, nl, g.N)
    evks = polys(list(range(g.D)) * (2 * g.beta), (n_keys,)).reshape(n_keys, g.beta, 2, g.D, g.N)
    return ct, evks


def hbm_bytes(g, nl, B, n_keys, fanout):
    """Algorithmic HBM traffic (bytes) of one pass, from the shapes: every array a kernel reads or writes counted once
    per launch that touches it (no cache reuse assumed between launches; the eval key once per launch)."""
    n, K, alpha = g.N, g.K, g.alpha
    ext, nparts = nl + K, -(-nl // alpha)
    w = 8 * n
    own = nl                          # limbs that are some digit's own (not converted)
    conv_limbs = nparts * ext - own   # converted limbs of all digits of one ciphertext
    # key-independent half, per ciphertext: INTT of c1 (2 passes: read + write each), conversions (read coef per digit,
    # write converted limbs), the row-pass read of the converted limbs
    shared = (4 * nl + nparts * nl + conv_limbs + conv_limbs) * w
    # key-dependent half, per (ciphertext, key): c1 own limbs read, til written (Q limbs) + pc written (P limbs), ModDown:
    # pc read + coefficient write (inverse column), conversion read K + write nl per component, tail reads til_Q + conv + c0
    # and writes the output
    per_key = (nl + 2 * nl + 2 * K + 2 * (2 * K) + 2 * (K + nl) + 2 * (nl + nl) + nl + 2 * nl) * w
    evk_read = nparts * 2 * ext * w   # the key limbs one pass over a chunk reads
    chunks = -(-B // 16)
    if fanout:  # the group changes the workspace, not the traffic: every key is still read once per chunk
        return B * shared + B * n_keys * per_key + chunks * n_keys * evk_read
    return n_keys * (B * shared + B * per_key + chunks * evk_read)


def run_ab(shape, groups, blocks, block_s, out):
    from ppqsflhe_amd import Context
    args, nl, B, n_keys = SHAPES[shape]
    results = {}
    for grp in groups:
        os.environ["MKCKKS_FANOUT_GROUP"] = str(grp)
        g = Context(*args[:4], dnum=args[4], device=0)  # raises without a device: no fallback
        ct, evks = make_inputs(g, nl, B, n_keys, 2024)
        d_ct, d_evks = g.to_device(ct), g.to_device(evks)
        d_a, d_b = g.empty((n_keys, B, 2, nl, g.N)), g.empty((n_keys, B, 2, nl, g.N))
        evk_words, ct_words = g.beta * 2 * g.D * g.N, 2 * nl * g.N

        def arm_a():
            for k in range(n_keys):
                g.reencrypt(d_ct, d_evks.view(k * evk_words, (g.beta, 2, g.D, g.N)), d_a.view(k * B * ct_words, (B, 2, nl, g.N)), B, nl)

        def arm_b():
            g.reencrypt_fanout(d_ct, d_evks, d_b, n_keys, B, nl)

        arm_a()
        arm_b()
        g.sync()
        if not np.array_equal(d_a.to_host(), d_b.to_host()):
            sys.exit(f"{shape} group {grp}: fan-out differs from the loop of single-key calls")
        for _ in range(2):
            arm_a()
            arm_b()
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

        ta, tb = [], []
        for _ in range(blocks):
            ta.append(block(arm_a))
            tb.append(block(arm_b))
        results[grp] = (ta, tb)
        ma, mb = statistics.median(ta), statistics.median(tb)
        print(f"{shape} nl={nl} B={B} n_keys={n_keys} MKCKKS_FANOUT_GROUP={grp}: verified B == A on all words", file=out)
        print(f"  arm A (loop of {n_keys} reencrypt): median {ma:.3f} ms  min {min(ta):.3f}  max {max(ta):.3f}  "
              f"({n_keys * B / ma * 1e3:.0f} ct/s)  algorithmic HBM {hbm_bytes(g, nl, B, n_keys, False) / 1e9:.3f} GB", file=out)
        print(f"  arm B (one reencrypt_fanout):      median {mb:.3f} ms  min {min(tb):.3f}  max {max(tb):.3f}  "
              f"({n_keys * B / mb * 1e3:.0f} ct/s)  algorithmic HBM {hbm_bytes(g, nl, B, n_keys, True) / 1e9:.3f} GB", file=out)
        print(f"  ratio B/A {mb / ma:.4f}  saving {100 * (1 - mb / ma):.1f} %  (arm A spread {max(ta) - min(ta):.3f} ms, "
              f"A - B = {ma - mb:.3f} ms, {blocks} blocks per arm of >= {block_s} s)", file=out)
        out.flush()
        g.close()
    best = min(results, key=lambda k: statistics.median(results[k][1]))
    print(f"{shape}: best MKCKKS_FANOUT_GROUP of {sorted(results)} = {best}", file=out)


def profile_arm_a(shape):
    from ppqsflhe_amd import Context
    args, nl, B, n_keys = SHAPES[shape]
    g = Context(*args[:4], dnum=args[4], device=0)
    ct, evks = make_inputs(g, nl, B, n_keys, 2024)
    d_ct, d_evks, d_a = g.to_device(ct), g.to_device(evks), g.empty((B, 2, nl, g.N))
    evk_words = g.beta * 2 * g.D * g.N
    for _ in range(3):
        for k in range(n_keys):
            g.reencrypt(d_ct, d_evks.view(k * evk_words, (g.beta, 2, g.D, g.N)), d_a, B, nl)
    g.sync()
    g.close()


def share(prof_dir, shape, out):
    """f: the share of arm A's kernel time in the key-independent kernels.  INTT of c1 = the inverse row pass (only c1 takes
    it: ModDown's inverse row pass is fused into the P-limb kernel) + the c1 part of the inverse column pass, apportioned
    by limb count (nl of c1 against 2 K of ModDown per ciphertext); ModUp's conversions = every k_conv_col* instance
    apportioned the same way (nparts conversions into ext - own limbs for ModUp against 2 conversions into nl limbs for
    ModDown).  The forward row passes of the converted digits are fused into the inner-product kernels of arm A and are
    NOT in this figure: f is a lower bound."""
    args, nl, B, n_keys = SHAPES[shape]
    files = glob.glob(prof_dir + "/**/*kernel_stats.csv", recursive=True)
    if not files:
        sys.exit("no *kernel_stats.csv under " + prof_dir)
    from ppqsflhe_amd import Context
    h = Context(*args[:4], dnum=args[4], device=-1)  # host-only: the limb structure
    K, alpha = h.K, h.alpha
    h.close()
    ext, nparts = nl + K, -(-nl // alpha)
    tot = inv_row = inv_col = conv = 0.0
    rows = []
    for r in csv.DictReader(open(files[0])):
        name, ns = r["Name"], float(r["TotalDurationNs"])
        if "mk::" not in name or "k_pack_rowb" in name:
            continue
        tot += ns
        rows.append((ns, name))
        if "k_ntt_row" in name and ("true" in name.split("k_ntt_row")[1][:24]):
            inv_row += ns
        elif "k_ntt_col_r" in name and ("true" in name.split("k_ntt_col_r")[1][:24]):
            inv_col += ns
        elif "k_conv_col" in name:
            conv += ns
    c1_col = inv_col * nl / (nl + 2 * K)
    modup_out, moddown_out = nparts * ext - nl, 2 * nl
    conv_up = conv * modup_out / (modup_out + moddown_out)
    f = (inv_row + c1_col + conv_up) / tot
    print(f"{shape}: arm A kernel time by kernel (rocprofv3 --kernel-trace --stats):", file=out)
    for ns, name in sorted(rows, reverse=True):
        short = name[name.index("mk::"):][:90]
        print(f"  {100 * ns / tot:6.2f} %  {short}", file=out)
    print(f"{shape}: f (lower bound: INTT of c1 {100 * (inv_row + c1_col) / tot:.1f} % + ModUp conversions "
          f"{100 * conv_up / tot:.1f} %, forward row passes not separable) = {f:.3f}; predicted B/A = 1 - f * "
          f"{n_keys - 1}/{n_keys} = {1 - f * (n_keys - 1) / n_keys:.3f}", file=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all")
    ap.add_argument("--groups", default="1,2,4,7")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-seconds", type=float, default=0.5)
    ap.add_argument("--profile-arm-a", action="store_true")
    ap.add_argument("--share", default=None)
    a = ap.parse_args()
    shapes = list(SHAPES) if a.shape == "all" else [a.shape]
    for sh in shapes:
        if a.share:
            share(a.share, sh, sys.stdout)
        elif a.profile_arm_a:
            profile_arm_a(sh)
        else:
            run_ab(sh, [int(x) for x in a.groups.split(",")], max(7, a.blocks), max(0.5, a.block_seconds), sys.stdout)


if __name__ == "__main__":
    main()
