#!/usr/bin/env python3
"""A/B of the slot rotation: mkckks_rotate_batch against the public calls it is made of, and k_automorph against a copy.

Arm R is mkckks_rotate_batch.  Arm C is the composition a caller without it would run: mkckks_automorphism_batch on the
batch (both components of every ciphertext are polynomials of one call) into a second buffer, then mkckks_reencrypt_batch
from there.  Arm P is mkckks_reencrypt_batch alone on the same ciphertexts: the floor, a rotation without its permutation.
Arm A is mkckks_automorphism_batch alone; its byte rate (bytes read + bytes written over the HIP-event time) stands beside
a device-to-device copy of the same bytes timed in the same process, on buffers larger than the Infinity Cache.
Arm S is a full-span mkckks_slot_sum_batch (log2(N/2) rotate-and-add steps).

usage: tools/bench_rotate.py [--blocks 7] [--block-seconds 0.5] [--out profiles/rotate_ab.txt]

Shapes: Context(16, 10, 50, 60, dnum=3), 16 ciphertexts of 11 limbs and of 2 limbs; Context(17, 2, 50, 60, dnum=2), 16
ciphertexts of 4 limbs.  One process, one card, all arrays resident, warmed, alternating blocks (R, C, P, A, R, ...) of at
least --block-seconds each; a block is timed with HIP events on the stream the kernels run on and reports milliseconds per
pass.  Arms R and C are compared word for word before anything is timed; a mismatch or a missing device ends the run with
a non-zero status.  Run it under a time limit of its own (timeout 600 is ample).
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

SHAPES = [((16, 10, 50, 60, 3), 11, 16, True), ((16, 10, 50, 60, 3), 2, 16, False), ((17, 2, 50, 60, 2), 4, 16, False)]
STREAM_CTS = 64  # ciphertexts of the byte-rate measurement: 2 x 738 MB at N = 2^16, 11 limbs


def run_ab(blocks, block_s, out):
    from ppqsflhe_amd import Context
    print(f"slot rotation A/B on {torch.cuda.get_device_name(0)}: arm R = rotate_batch, arm C = automorphism_batch + "
          f"reencrypt_batch, arm P = reencrypt_batch alone, arm A = automorphism_batch alone, arm S = full-span slot_sum_batch",
          file=out)

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

    def line(label, ts, extra=""):
        print(f"  {label:34s} median {statistics.median(ts):.4f} ms  min {min(ts):.4f}  max {max(ts):.4f}{extra}", file=out)

    ctx = {}
    for args, nl, B, with_sum in SHAPES:
        if args not in ctx:
            ctx[args] = Context(*args[:4], dnum=args[4], device=0)  # raises without a device: no fallback
            ctx[args].set_stream(torch.cuda.current_stream().cuda_stream)
        g = ctx[args]
        N = g.N
        gel = g.galois_element(3)
        ct, evks = make_inputs(g, nl, B, 1, 2027)
        d_ct, d_evk = g.to_device(ct), g.to_device(evks[0])
        d_r, d_c, d_tmp, d_p = (g.empty((B, 2, nl, N)) for _ in range(4))
        arms = {"R": lambda: g.rotate(d_ct, d_evk, d_r, B, nl, gel),
                "C": lambda: (g.automorphism(d_ct, d_tmp, 2 * B, nl, gel), g.reencrypt(d_tmp, d_evk, d_c, B, nl)),
                "P": lambda: g.reencrypt(d_ct, d_evk, d_p, B, nl),
                "A": lambda: g.automorphism(d_ct, d_tmp, 2 * B, nl, gel)}
        for fn in arms.values():
            fn()
        sync()
        if not np.array_equal(d_r.to_host(), d_c.to_host()):
            sys.exit(f"N={N} nl={nl}: mkckks_rotate_batch differs from automorphism_batch + reencrypt_batch")
        t = measure(arms)
        mr, mc, mp, ma = (statistics.median(t[k]) for k in "RCPA")
        nbytes = 2 * B * 2 * nl * N * 8
        print(f"N = 2^{args[0]}, {B} ciphertexts of {nl} limb(s), g = 5^3: arm R == arm C on all words (bit-identical)", file=out)
        line("arm R (rotate_batch):", t["R"], f"  ({mr / B * 1e3:.2f} us per ciphertext)")
        line("arm C (automorphism + reencrypt):", t["C"])
        line("arm P (reencrypt alone):", t["P"])
        line("arm A (automorphism alone):", t["A"], f"  ({nbytes / ma / 1e9:.2f} TB/s read + written, {nbytes / 1e6:.0f} MB)")
        print(f"         C / R = {mc / mr:.3f} x  (C - R = {mc - mr:.4f} ms; spread R {max(t['R']) - min(t['R']):.4f} ms, "
              f"C {max(t['C']) - min(t['C']):.4f} ms)", file=out)
        print(f"         R / P = {mr / mp:.3f} x  (R - P = {mr - mp:.4f} ms, automorphism alone {ma:.4f} ms; spread P "
              f"{max(t['P']) - min(t['P']):.4f} ms)", file=out)
        if with_sum:
            m = (N // 2).bit_length() - 1
            _, keys = make_inputs(g, 1, 1, m, 2028)
            d_keys, d_s = g.to_device(keys), g.empty((B, 2, nl, N))
            ts = measure({"S": lambda: g.slot_sum(d_ct, d_keys, d_s, B, nl, N // 2)})["S"]
            ms = statistics.median(ts)
            line(f"arm S (slot_sum, span {N // 2}):", ts, f"  ({m} steps, {ms / m:.4f} ms per step, {ms / m / mr:.3f} x arm R)")
            del d_keys, d_s
            # byte rate of k_automorph beside a copy, both on buffers beyond the Infinity Cache
            words = STREAM_CTS * 2 * nl * N
            t_in = torch.randint(0, 2 ** 40, (words,), dtype=torch.int64, device="cuda")
            t_out = torch.empty_like(t_in)
            tb = measure({"K": lambda: g.automorphism(t_in, t_out, STREAM_CTS * 2, nl, gel), "D": lambda: t_out.copy_(t_in)})
            mk_, md = statistics.median(tb["K"]), statistics.median(tb["D"])
            print(f"  byte rate, {STREAM_CTS} ciphertexts of {nl} limbs ({2 * words * 8 / 1e6:.0f} MB read + written per pass):", file=out)
            line("k_automorph:", tb["K"], f"  ({2 * words * 8 / mk_ / 1e9:.2f} TB/s)")
            line("device-to-device copy:", tb["D"], f"  ({2 * words * 8 / md / 1e9:.2f} TB/s; k_automorph / copy = {mk_ / md:.3f} x)")
            del t_in, t_out
    print(f"  {blocks} alternating blocks per arm of >= {block_s} s, HIP-event time per pass", file=out)
    out.flush()
    for g in ctx.values():
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
