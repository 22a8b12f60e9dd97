#!/usr/bin/env python3
"""A/B of the collective key-switch share: mkckks_switch_share_batch against the composition its header names.

Arm A uses only the entry points the library had before: mkckks_partial_decrypt_batch with zero errors, mkckks_ntt_forward_batch
on its output, and mkckks_rerandomize_batch out of place on a resident ciphertext batch whose component 1 is zero and whose
component 0 is that output (one strided device-to-device copy, counted: the entry points do not share a layout).  Arm B is
mkckks_switch_share_batch on the same ciphertexts, keys and randomness.  Arm R is mkckks_rerandomize_batch alone on the
ciphertexts: the same lift and the same three forward transforms without c1 * s, the floor of both arms.

usage: tools/bench_kswitch.py [--blocks 7] [--block-seconds 0.5] [--out profiles/kswitch_ab.txt]

Shapes: Context(16, 10, 50, 60, dnum=3); the aggregate as it leaves the server, 16 ciphertexts of 11 limbs; and the compact
shape, 256 ciphertexts of 1 limb.  Errors: e0 of sigma = 2^20, e1 of sigma = 2^6.  One process, one card, all arrays resident,
warmed, alternating blocks (A, B, R, A, B, R, ...) of at least --block-seconds each; a block is timed with HIP events on the
stream the kernels run on and reports milliseconds per pass.  The two arms are compared word for word, for both values of
lead, before anything is timed; a mismatch or a missing device ends the run with a non-zero status.  Run it under a time
limit of its own (timeout 300 is ample).
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
SIGMA0_BITS, SIGMA1_BITS = 20, 6


def arms_for(g, nl, B, lead):
    ct, _ = make_inputs(g, nl, B, 0, 2026)
    rng = np.random.default_rng(10)
    N = g.N
    sk = np.empty((g.D, N), dtype=np.uint64)
    pk = np.empty((2, g.D, N), dtype=np.uint64)
    for l in range(g.D):
        sk[l] = rng.integers(0, int(g.moduli[l]), size=N, dtype=np.uint64)
        pk[:, l] = rng.integers(0, int(g.moduli[l]), size=(2, N), dtype=np.uint64)
    d_v, d_e0, d_e1 = g.empty((B, N), np.int8), g.empty((B, N), np.int64), g.empty((B, N), np.int64)
    key = rng.bytes(32)
    g.sample_ternary(d_v, B * N, key, 0)
    g.sample_gauss_wide(d_e0, B * N, 2.0 ** SIGMA0_BITS, key, 1)
    g.sample_gauss_wide(d_e1, B * N, 2.0 ** SIGMA1_BITS, key, 2)
    d_ct, d_sk, d_pk = g.to_device(ct), g.to_device(sk), g.to_device(pk)
    d_zero = g.to_device(np.zeros((B, N), dtype=np.int64), np.int64)
    # torch tensors where the composition has to assemble the ciphertext (x, 0): the library runs on torch's current stream
    t_x = torch.empty((B, nl, N), dtype=torch.int64, device="cuda")
    t_src = torch.zeros((B, 2, nl, N), dtype=torch.int64, device="cuda")  # component 1 is zero and stays zero
    d_a, d_b, d_r = g.empty((B, 2, nl, N)), g.empty((B, 2, nl, N)), g.empty((B, 2, nl, N))

    def arm_a():
        g.partial_decrypt(d_ct, d_sk, d_zero, t_x, B, nl, nl, lead)
        g.ntt_forward(t_x, B, nl)
        t_src[:, 0].copy_(t_x)  # one strided device copy, counted: the three entry points do not share a layout
        g.rerandomize(t_src, d_pk, d_v, d_e0, d_e1, d_a, B, nl, nl)

    def arm_b():
        g.switch_share(d_ct, d_sk, d_pk, d_v, d_e0, d_e1, nl, lead, out=d_b)

    def arm_r():
        g.rerandomize(d_ct, d_pk, d_v, d_e0, d_e1, d_r, B, nl, nl)

    return {"A": arm_a, "B": arm_b, "R": arm_r}, d_a, d_b


def run_ab(blocks, block_s, out):
    from ppqsflhe_amd import Context
    g = Context(*ARGS[:4], dnum=ARGS[4], device=0)  # raises without a device: no fallback
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    print(f"key-switch share A/B on {torch.cuda.get_device_name(0)}: N = 2^{ARGS[0]}, sigma0 = 2^{SIGMA0_BITS}, sigma1 = "
          f"2^{SIGMA1_BITS}; arm A = partial_decrypt_batch(e = 0) + ntt_forward_batch + copy into (x, 0) + rerandomize_batch, "
          f"arm B = switch_share_batch, arm R = rerandomize_batch alone (no c1 * s)", file=out)

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
                sys.exit(f"nl={nl} lead={lead}: mkckks_switch_share_batch differs from partial_decrypt + ntt_forward + rerandomize")
            for _ in range(3):
                for fn in arms.values():
                    fn()
            sync()
            t = {name: [] for name in arms}
            for _ in range(blocks):
                for name, fn in arms.items():
                    t[name].append(block(fn))
            ta, tb, tr = t["A"], t["B"], t["R"]
            ma, mb, mr = statistics.median(ta), statistics.median(tb), statistics.median(tr)
            print(f"{B} ciphertexts of {nl} limb(s), lead = {lead}: arm B == arm A on all words (bit-identical)", file=out)
            print(f"  arm A (three entry points):     median {ma:.4f} ms  min {min(ta):.4f}  max {max(ta):.4f}  "
                  f"({ma / B * 1e3:.2f} us per ciphertext)", file=out)
            print(f"  arm B (switch_share):           median {mb:.4f} ms  min {min(tb):.4f}  max {max(tb):.4f}  "
                  f"({mb / B * 1e3:.2f} us per ciphertext)", file=out)
            print(f"         A / B = {ma / mb:.2f} x  (A - B = {ma - mb:.4f} ms; spread A {max(ta) - min(ta):.4f} ms, "
                  f"B {max(tb) - min(tb):.4f} ms)", file=out)
            print(f"  arm R (rerandomize alone):      median {mr:.4f} ms  min {min(tr):.4f}  max {max(tr):.4f}  "
                  f"(B / R = {mb / mr:.2f} x)", file=out)
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
