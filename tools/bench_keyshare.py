#!/usr/bin/env python3
"""A/B of the t-of-n key sharing: mkckks_share_key against its composition from the public entry points, and the per-round
extra of a threshold decryption with key shares.

Arm A (composition): t - 1 mkckks_sample_uniform calls write r_1 .. r_{t-1} to HBM behind a resident copy of sk, then n
mkckks_combine_key_shares calls (m = t, weights (p + 1)^k mod q_i) read all t operands once per party.  Arm B (fused):
one mkckks_share_key -- the coefficient polynomials never reach HBM.  Word count per coefficient and limb: fused 1 read +
n writes; composition (t - 1) writes + n t reads + n writes.

Per-round extra: one mkckks_combine_key_shares with m = 1 over 11 limbs (lambda * sigma_j, arm C) beside the
mkckks_partial_decrypt_batch of 16 ciphertexts of 11 limbs that it precedes (arm P).

usage: tools/bench_keyshare.py [--blocks 7] [--block-seconds 0.5] [--out profiles/keyshare_ab.txt]

Context(16, 10, 50, 60, dnum=3), nl = 12, (n, t) = (8, 5) and (16, 9).  One process, one card, all arrays resident, warmed,
alternating blocks of at least --block-seconds each; a block is timed with HIP events on the stream the kernels run on and
reports milliseconds per pass.  The two sharing arms are compared word for word before anything is timed; a mismatch or a
missing device ends the run with a non-zero status.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools.bench_fanout import make_inputs  # noqa: E402

ARGS = (16, 10, 50, 60, 3)
NL = 12
SHAPES = [(8, 5), (16, 9)]  # (n_parties, threshold)
ROUND_NL, ROUND_B = 11, 16


def sharing_arms(g, sk, n, t, key):
    N = g.N
    d_sk = g.to_device(sk)
    d_ops = g.empty((t, NL, N))
    d_ops.view(0, (NL, N)).upload(sk[:NL])
    d_a, d_b = g.empty((n, NL, N)), g.empty((n, NL, N))
    outs = [d_a.view(p * NL * N, (NL, N)) for p in range(n)]
    rks = [d_ops.view(k * NL * N, (1, NL, N)) for k in range(1, t)]
    ws = [np.array([[pow(p + 1, k, int(g.moduli[i])) for i in range(NL)] for k in range(t)], dtype=np.uint64) for p in range(n)]

    def arm_a():
        for k in range(1, t):
            g.sample_uniform(rks[k - 1], 1, NL, False, key, k - 1)
        for p in range(n):
            g.combine_key_shares(d_ops, ws[p], outs[p], t, NL)

    def arm_b():
        g.share_key(d_sk, d_b, NL, n, t, key, 0)

    return {"A": arm_a, "B": arm_b}, d_a, d_b


def round_arms(g, sk):
    ct, _ = make_inputs(g, ROUND_NL, ROUND_B, 0, 2026)
    rng = np.random.default_rng(9)
    d_e = g.empty((ROUND_B, g.N), np.int64)
    g.sample_gauss_wide(d_e, ROUND_B * g.N, 2.0 ** 20, rng.bytes(32), 0)
    d_ct, d_sigma = g.to_device(ct), g.to_device(sk[:ROUND_NL])
    d_key, d_share = g.empty((ROUND_NL, g.N)), g.empty((ROUND_B, ROUND_NL, g.N))
    lam = g.lagrange_at_zero((2, 5, 7, 11, 16))[1:2, :ROUND_NL].copy()

    def arm_c():
        g.combine_key_shares(d_sigma, lam, d_key, 1, ROUND_NL)

    def arm_p():
        g.partial_decrypt(d_ct, d_key, d_e, d_share, ROUND_B, ROUND_NL, ROUND_NL, True)

    return {"C": arm_c, "P": arm_p}


def run_ab(blocks, block_s, out):
    from ppqsflhe_amd import Context
    g = Context(*ARGS[:4], dnum=ARGS[4], device=0)  # raises without a device: no fallback
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    print(f"key sharing A/B on {torch.cuda.get_device_name(0)}: N = 2^{ARGS[0]}, nl = {NL}; arm A = (t - 1) x sample_uniform + "
          f"n x combine_key_shares (m = t, weights (p + 1)^k), arm B = share_key", file=out)

    def sync():
        torch.cuda.synchronize()

    def block(fn):
        reps, total = 0, 0.0
        while total < block_s * 1e3:
            n = 8 if reps else 2
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(n):
                fn()
            ev1.record()
            sync()
            total += ev0.elapsed_time(ev1)
            reps += n
        return total / reps

    def measure(arms):
        for _ in range(3):
            for fn in arms.values():
                fn()
        sync()
        t = {name: [] for name in arms}
        for _ in range(blocks):
            for name, fn in arms.items():
                t[name].append(block(fn))
        return t

    def line(label, ts):
        return f"  {label:40s} median {statistics.median(ts):.4f} ms  min {min(ts):.4f}  max {max(ts):.4f}"

    rng = np.random.default_rng(3)
    sk = np.empty((g.D, g.N), dtype=np.uint64)
    for l in range(g.D):
        sk[l] = rng.integers(0, int(g.moduli[l]), size=g.N, dtype=np.uint64)
    key = rng.bytes(32)
    for n, t in SHAPES:
        arms, d_a, d_b = sharing_arms(g, sk, n, t, key)
        for fn in arms.values():
            fn()
        sync()
        if not np.array_equal(d_a.to_host(), d_b.to_host()):
            sys.exit(f"n={n} t={t}: mkckks_share_key differs from sample_uniform + combine_key_shares")
        ts = measure(arms)
        ma, mb = statistics.median(ts["A"]), statistics.median(ts["B"])
        words_a, words_b = (t - 1) + n * t + n, 1 + n
        print(f"n = {n}, t = {t}: arm B == arm A on all words (bit-identical)", file=out)
        print(line(f"arm A ({t - 1} sample_uniform + {n} combine):", ts["A"]), file=out)
        print(line("arm B (share_key):", ts["B"]), file=out)
        print(f"         A / B = {ma / mb:.2f} x  (A - B = {ma - mb:.4f} ms; spread A {max(ts['A']) - min(ts['A']):.4f} ms, "
              f"B {max(ts['B']) - min(ts['B']):.4f} ms); words per coefficient and limb A {words_a}, B {words_b} "
              f"({words_a / words_b:.2f} x)", file=out)
    ts = measure(round_arms(g, sk))
    mc, mp = statistics.median(ts["C"]), statistics.median(ts["P"])
    print(f"per-round extra: {ROUND_B} ciphertexts of {ROUND_NL} limbs", file=out)
    print(line("arm C (combine_key_shares, m = 1):", ts["C"]), file=out)
    print(line("arm P (partial_decrypt_batch):", ts["P"]), file=out)
    print(f"         C / P = {mc / mp:.3f}  (the key share's Lagrange scaling adds {100 * mc / mp:.1f} % to a party's round)", file=out)
    print(f"  {blocks} alternating blocks per arm of >= {block_s} s, HIP-event time per pass", file=out)
    out.flush()
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout
    run_ab(max(7, a.blocks), max(0.5, a.block_seconds), out)


if __name__ == "__main__":
    main()
