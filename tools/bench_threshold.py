#!/usr/bin/env python3
"""A/B of the partial (threshold) decryption: mkckks_partial_decrypt_batch against the composition its header names.

Arm A uses only the entry points the library had before: mkckks_rerandomize_batch(v = 0, e0 = e, e1 = 0) out of place,
then mkckks_decrypt_batch (lead = 1); for lead = 0 the same on a resident copy whose component 0 is zero.  Arm B is
mkckks_partial_decrypt_batch on the same ciphertexts, key and errors.  Arm D is mkckks_decrypt_batch alone (k_fma + the
plain inverse transform, no error at all): arm A spends three forward transforms on its zero mask, so D is the floor of
any composition and shows what the smudging costs on top of a decryption.

usage: tools/bench_threshold.py [--blocks 7] [--block-seconds 0.5] [--out profiles/threshold_ab.txt]

Shapes: Context(16, 10, 50, 60, dnum=3); the aggregate as it leaves the server, 16 ciphertexts of 11 limbs; and the compact
shape, 256 ciphertexts of 1 limb.  Errors: sigma = 2^20.  One process, one card, all arrays resident, warmed, alternating
blocks (A, B, D, A, B, D, ...) of at least --block-seconds each; a block is timed with HIP events on the stream the kernels run
on and reports milliseconds per pass.  The two arms are compared word for word, for both values of lead, before anything is
timed; a mismatch or a missing device ends the run with a non-zero status.
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
SHAPES = [(11, 16), (1, 256)]  # (limbs, ciphertexts)
SIGMA_BITS = 20


def arms_for(g, nl, B, lead):
    ct, _ = make_inputs(g, nl, B, 0, 2026)
    rng = np.random.default_rng(9)
    sk = np.empty((g.D, g.N), dtype=np.uint64)
    for l in range(g.D):
        sk[l] = rng.integers(0, int(g.moduli[l]), size=g.N, dtype=np.uint64)
    d_e = g.empty((B, g.N), np.int64)
    g.sample_gauss_wide(d_e, B * g.N, 2.0 ** SIGMA_BITS, rng.bytes(32), 0)
    src = ct.copy()
    if not lead:
        src[:, 0] = 0
    d_ct, d_src, d_sk = g.to_device(ct), g.to_device(src), g.to_device(sk)
    d_work, d_a, d_b = g.empty((B, 2, nl, g.N)), g.empty((B, nl, g.N)), g.empty((B, nl, g.N))
    d_pk0 = g.to_device(np.zeros((2, g.D, g.N), dtype=np.uint64))
    d_v0, d_z = g.to_device(np.zeros((B, g.N), dtype=np.int8), np.int8), g.to_device(np.zeros((B, g.N), dtype=np.int64), np.int64)

    def arm_a():  # out of place: the source is never consumed
        g.rerandomize(d_src, d_pk0, d_v0, d_e, d_z, d_work, B, nl, nl)
        g.decrypt(d_work, d_sk, d_a, B, nl)

    def arm_b():
        g.partial_decrypt(d_ct, d_sk, d_e, d_b, B, nl, nl, lead)

    d_d = g.empty((B, nl, g.N))

    def arm_d():
        g.decrypt(d_ct, d_sk, d_d, B, nl)

    return {"A": arm_a, "B": arm_b, "D": arm_d}, d_a, d_b


def run_ab(blocks, block_s, out):
    from ppqsflhe_amd import Context
    g = Context(*ARGS[:4], dnum=ARGS[4], device=0)  # raises without a device: no fallback
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    print(f"partial decryption A/B on {torch.cuda.get_device_name(0)}: N = 2^{ARGS[0]}, sigma = 2^{SIGMA_BITS}; arm A = "
          f"rerandomize_batch(v = 0, e0 = e, e1 = 0) + decrypt_batch (component 0 zeroed for lead = 0), arm B = "
          f"partial_decrypt_batch, arm D = decrypt_batch alone (no error added)", file=out)

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

    for nl, B in SHAPES:
        for lead in (1, 0):
            arms, d_a, d_b = arms_for(g, nl, B, lead)
            for fn in arms.values():
                fn()
            sync()
            if not np.array_equal(d_a.to_host(), d_b.to_host()):
                sys.exit(f"nl={nl} lead={lead}: mkckks_partial_decrypt_batch differs from rerandomize_batch + decrypt_batch")
            for _ in range(3):
                for fn in arms.values():
                    fn()
            sync()
            t = {name: [] for name in arms}
            for _ in range(blocks):
                for name, fn in arms.items():
                    t[name].append(block(fn))
            ta = t["A"]
            ma, mb = statistics.median(ta), statistics.median(t["B"])
            print(f"{B} ciphertexts of {nl} limb(s), lead = {lead}: arm B == arm A on all words (bit-identical)", file=out)
            print(f"  arm A (rerandomize + decrypt):  median {ma:.4f} ms  min {min(ta):.4f}  max {max(ta):.4f}  "
                  f"({ma / B * 1e3:.2f} us per ciphertext)", file=out)
            print(f"  arm B (partial_decrypt):        median {mb:.4f} ms  min {min(t['B']):.4f}  max {max(t['B']):.4f}  "
                  f"({mb / B * 1e3:.2f} us per ciphertext)", file=out)
            print(f"         A / B = {ma / mb:.2f} x  (A - B = {ma - mb:.4f} ms; spread A {max(ta) - min(ta):.4f} ms, "
                  f"B {max(t['B']) - min(t['B']):.4f} ms)", file=out)
            md = statistics.median(t["D"])
            print(f"  arm D (decrypt alone):          median {md:.4f} ms  min {min(t['D']):.4f}  max {max(t['D']):.4f}  "
                  f"(D / B = {md / mb:.2f} x)", file=out)
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
