#!/usr/bin/env python3
"""A/B of the re-randomisation before a key switch (HRA-secure re-encryption).

Arm A uses only the entry points the library had before mkckks_rerandomize_batch: mkckks_encrypt_batch with pt := a packed
copy of the c0 components and int32 errors, then mkckks_eval_add_batch with (0, c1).  Arm B is mkckks_rerandomize_batch
on the same v, e0, e1 (as int64).  Arm F is the key switch that follows on the same inputs (mkckks_reencrypt_fanout_batch
over 7 keys; at the compact prefix mkckks_reencrypt_fanout_compact_batch to 1 limb): arm B is reported as a share of it.

usage: tools/bench_rerandomize.py [--blocks 7] [--block-seconds 0.5] [--out profiles/rerandomize_ab.txt]
       tools/bench_rerandomize.py --profile-arm-b [--limbs 11]     # a few arm-B passes only, to run under
                                                        # rocprofv3 --kernel-trace --stats -- python ...

Shapes: the back leg of the headline workload, Context(16, 10, 50, 60, dnum=3), 16 ciphertexts of 11 limbs: nl = 11 (the
whole aggregate) and nl = 2 (the prefix serverRound --back-limbs 1 re-randomises, read in place out of the 11 limbs by arm B,
from a packed copy by arm A).  Errors: sigma = 2^20 (fits arm A's int32).  One process, all arrays resident, warmed,
alternating blocks (A, B, F, A, B, F, ...) of at least --block-seconds each, wall time between device synchronisations.
The two arms are compared word for word before anything is timed; a mismatch or a missing device ends the run with a
non-zero status.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_fanout import SHAPES, make_inputs  # noqa: E402

SIGMA_BITS = 20
N_KEYS = 7


def setup(g, nl_in, B):
    ct, evks = make_inputs(g, nl_in, B, N_KEYS, 2025)
    rng = np.random.default_rng(7)
    pk = np.empty((2, g.D, g.N), dtype=np.uint64)
    for l in range(g.D):
        pk[:, l] = rng.integers(0, int(g.moduli[l]), size=(2, g.N), dtype=np.uint64)
    key = rng.bytes(32)
    d_v, d_e0, d_e1 = g.empty((B, g.N), np.int8), g.empty((B, g.N), np.int64), g.empty((B, g.N), np.int64)
    g.sample_ternary(d_v, B * g.N, key, 0)
    g.sample_gauss_wide(d_e0, B * g.N, 2.0 ** SIGMA_BITS, key, 1)
    g.sample_gauss_wide(d_e1, B * g.N, 2.0 ** SIGMA_BITS, key, 2)
    e0, e1 = d_e0.to_host(), d_e1.to_host()
    assert max(np.abs(e0).max(), np.abs(e1).max()) < 2 ** 31
    return dict(ct=ct, d_ct=g.to_device(ct), d_evks=g.to_device(evks), d_pk=g.to_device(pk), d_v=d_v, d_e0=d_e0, d_e1=d_e1,
                d_e0_32=g.to_device(e0.astype(np.int32)), d_e1_32=g.to_device(e1.astype(np.int32)))


def arms_for(g, s, nl_in, nl, B):
    ct = s["ct"]
    c1_only = np.zeros((B, 2, nl, g.N), dtype=np.uint64)
    c1_only[:, 1] = ct[:, 1, :nl]
    d_pt, d_c1 = g.to_device(np.ascontiguousarray(ct[:, 0, :nl])), g.to_device(c1_only)
    d_a, d_b = g.empty((B, 2, nl, g.N)), g.empty((B, 2, nl, g.N))

    def arm_a():
        g.encrypt(s["d_pk"], d_pt, s["d_v"], s["d_e0_32"], s["d_e1_32"], d_a, B, nl)
        g.eval_add(d_a, d_c1, d_a, B, nl)

    def arm_b():
        g.rerandomize(s["d_ct"], s["d_pk"], s["d_v"], s["d_e0"], s["d_e1"], d_b, B, nl_in, nl)

    if nl == nl_in:
        d_f = g.empty((N_KEYS, B, 2, nl, g.N))
        arm_f = lambda: g.reencrypt_fanout(d_b, s["d_evks"], d_f, N_KEYS, B, nl)  # noqa: E731
        f_name = f"reencrypt_fanout, {N_KEYS} keys at {nl} limbs"
    else:
        d_f = g.empty((N_KEYS, B, 2, nl - 1, g.N))
        arm_f = lambda: g.reencrypt_fanout_compact(d_b, s["d_evks"], d_f, N_KEYS, B, nl, nl - 1)  # noqa: E731
        f_name = f"reencrypt_fanout_compact, {N_KEYS} keys, {nl} -> {nl - 1} limb"
    return {"A": arm_a, "B": arm_b, "F": arm_f}, d_a, d_b, f_name


def run_ab(blocks, block_s, out):
    from ppqsflhe_amd import Context
    args, nl_in, B, _ = SHAPES["n16"]
    g = Context(*args[:4], dnum=args[4], device=0)  # raises without a device: no fallback
    s = setup(g, nl_in, B)
    print(f"re-randomisation A/B: N = 2^{args[0]}, {B} ciphertexts of {nl_in} limbs, sigma = 2^{SIGMA_BITS}; arm A = encrypt_batch "
          f"(pt := c0) + eval_add_batch (0, c1), arm B = rerandomize_batch, arm F = the key switch that follows", file=out)
    for nl in (nl_in, 2):
        arms, d_a, d_b, f_name = arms_for(g, s, nl_in, nl, B)
        for fn in arms.values():
            fn()
        g.sync()
        if not np.array_equal(d_a.to_host(), d_b.to_host()):
            sys.exit(f"nl={nl}: mkckks_rerandomize_batch differs from encrypt_batch + eval_add_batch")
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
        ma, mb, mf = (statistics.median(t[k]) for k in "ABF")
        print(f"nl = {nl}{' (prefix of ' + str(nl_in) + ')' if nl != nl_in else ''}: arm B == arm A on all words", file=out)
        print(f"  arm A (encrypt + eval_add):  median {ma:.3f} ms  min {min(t['A']):.3f}  max {max(t['A']):.3f}  "
              f"({ma / B * 1e3:.1f} us per ciphertext)", file=out)
        print(f"  arm B (rerandomize):         median {mb:.3f} ms  min {min(t['B']):.3f}  max {max(t['B']):.3f}  "
              f"({mb / B * 1e3:.1f} us per ciphertext)", file=out)
        print(f"         A / B = {ma / mb:.2f} x  (A - B = {ma - mb:.3f} ms; spread A {max(t['A']) - min(t['A']):.3f} ms, "
              f"B {max(t['B']) - min(t['B']):.3f} ms)", file=out)
        print(f"  arm F ({f_name}): median {mf:.3f} ms; arm B = {100 * mb / mf:.1f} % of it", file=out)
    print(f"  {blocks} alternating blocks per arm of >= {block_s} s", file=out)
    out.flush()
    g.close()


def profile_arm_b(nl):
    from ppqsflhe_amd import Context
    args, nl_in, B, _ = SHAPES["n16"]
    g = Context(*args[:4], dnum=args[4], device=0)
    s = setup(g, nl_in, B)
    arms, _, _, _ = arms_for(g, s, nl_in, nl, B)
    for _ in range(5):
        arms["B"]()
    g.sync()
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile-arm-b", action="store_true")
    ap.add_argument("--limbs", type=int, default=11)
    a = ap.parse_args()
    if a.profile_arm_b:
        profile_arm_b(a.limbs)
        return
    out = open(a.out, "w") if a.out else sys.stdout
    run_ab(max(7, a.blocks), max(0.5, a.block_seconds), out)


if __name__ == "__main__":
    main()
