#!/usr/bin/env python3
"""A/B of the weighted aggregation at the bench shape: N = 2^16, L = 12, dnum = 3, 8 clients x 16 ciphertexts.

  a   mkckks_reencrypt_sum_batch + mkckks_rescale_mult_const_batch(1/8)     today's unweighted step: the anchor
  b   mkckks_scale_evk_batch + mkckks_reencrypt_wsum_batch + mkckks_rescale_batch     the weighted step
  b'  the same without the key scaling: a round whose weights did not change
  c   what a user had to run for the same quantity: per client mkckks_reencrypt_batch +
      mkckks_rescale_mult_const_batch(w_c), then mkckks_eval_sum_batch (OpenFHE's order)
  d   mkckks_eval_wsum_batch over 8 in-domain clients
  d0  the same by mkckks_mult_const_batch per client + mkckks_eval_sum_batch

usage: tools/bench_weighted.py [--blocks 7] [--block-seconds 0.5] [--out profiles/weighted_ab.txt]

One process, one card, all arrays resident, warmed, alternating blocks of at least --block-seconds each; a block is timed
with HIP events on the stream the kernels run on and reports milliseconds per pass (median, min, max over the blocks).
Before anything is timed, b is compared word for word with mkckks_reencrypt_sum_batch on host-independent inputs scaled
on the device (the keys by scale_evk, c0 by eval_wsum of one term) and d with d0; a mismatch or a missing device ends
the run with a non-zero status.  The run ends with the precision pair of tests/test_weighted_aggregation.py when the
oracle is built.
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
NL, C, B = 12, 8, 16
COUNTS = [5.0, 3.0, 2.0, 7.0, 11.0, 1.0, 4.0, 6.0]


def run_ab(blocks, block_s, out):
    from ppqsflhe_amd import Context
    g = Context(*ARGS[:4], dnum=ARGS[4], device=0)  # raises without a device: no fallback
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    N = g.N
    w = np.array(COUNTS) / sum(COUNTS)
    sf_level = g.L - NL + 1
    print(f"weighted aggregation A/B on {torch.cuda.get_device_name(0)}: N = 2^{ARGS[0]}, nl = {NL}, {C} clients x {B} ciphertexts, "
          f"weights {':'.join(str(int(x)) for x in COUNTS)}", file=out)
    cts = np.stack([make_inputs(g, NL, B, 0, 100 + c)[0] for c in range(C)])
    evks = make_inputs(g, NL, 1, C, 7)[1]
    d_cts, d_evks = g.to_device(cts), g.to_device(evks)
    del cts, evks
    d_scaled = g.empty((C, g.beta, 2, g.D, N))
    d_sum, d_sum2 = g.empty((B, 2, NL, N)), g.empty((B, 2, NL, N))
    d_out = g.empty((B, 2, NL - 1, N))
    d_per = g.empty((C, B, 2, NL, N))
    d_per_out = g.empty((C, B, 2, NL - 1, N))
    ct_words, evk_words = B * 2 * NL * N, g.beta * 2 * g.D * N
    ct_v = [d_cts.view(c * ct_words, (B, 2, NL, N)) for c in range(C)]
    evk_v = [d_evks.view(c * evk_words, (g.beta, 2, g.D, N)) for c in range(C)]
    per_v = [d_per.view(c * ct_words, (B, 2, NL, N)) for c in range(C)]
    per_out_v = [d_per_out.view(c * B * 2 * (NL - 1) * N, (B, 2, NL - 1, N)) for c in range(C)]

    def arm_a():
        g.reencrypt_sum(d_cts, d_evks, d_sum, C, B, NL)
        g.rescale_mult_const(d_sum, d_out, B, NL, 1.0 / C)

    def arm_b1():
        g.reencrypt_wsum(d_cts, d_scaled, d_sum, C, B, NL, w, sf_level)
        g.rescale(d_sum, d_out, B, NL)

    def arm_b():
        g.scale_evk(d_evks, d_scaled, C, w, sf_level)
        arm_b1()

    def arm_c():
        for c in range(C):
            g.reencrypt(ct_v[c], evk_v[c], per_v[c], B, NL)
            g.rescale_mult_const(per_v[c], per_out_v[c], B, NL, w[c])
        g.eval_sum(d_per_out, d_out, C, B, NL - 1)

    def arm_d():
        g.eval_wsum(d_cts, d_sum, C, B, NL, w, sf_level - 1)

    def arm_d0():
        # mult_const works in place: on the inputs themselves, so the residues drift from pass to pass -- timing only
        for c in range(C):
            g.mult_const(per_v[c], B, NL, w[c])
        g.eval_sum(d_per, d_sum2, C, B, NL)

    def sync():
        torch.cuda.synchronize()

    # ---- checks before timing
    g.scale_evk(d_evks, d_scaled, C, w, sf_level)
    g.reencrypt_wsum(d_cts, d_scaled, d_sum, C, B, NL, w, sf_level)
    sync()
    got = d_sum.to_host()
    # c0 scaled on the device, client by client (eval_wsum of one term scales both components: c1 is put back), then the
    # plain sum with the scaled keys
    host = d_cts.to_host()
    for c in range(C):
        g.eval_wsum(ct_v[c], per_v[c], 1, B, NL, [w[c]], sf_level)
    sync()
    mixed = d_per.to_host()
    mixed[:, :, 1] = host[:, :, 1]
    d_per.upload(mixed)
    g.reencrypt_sum(d_per, d_scaled, d_sum2, C, B, NL)
    sync()
    if not np.array_equal(got, d_sum2.to_host()):
        sys.exit("reencrypt_wsum differs from reencrypt_sum on inputs with c0 scaled")
    del got, mixed, host
    d_per.upload(d_cts.to_host())
    arm_d()
    for c in range(C):
        g.mult_const(per_v[c], B, NL, w[c])  # mult_const at nl = L takes sf(L - nl) = sf(0): the level arm d is given
    g.eval_sum(d_per, d_sum2, C, B, NL)
    sync()
    if not np.array_equal(d_sum.to_host(), d_sum2.to_host()):
        sys.exit("eval_wsum differs from mult_const per client + eval_sum")
    print("checks: reencrypt_wsum == reencrypt_sum on c0-scaled inputs with the scaled keys; eval_wsum == mult_const x 8 + eval_sum "
          "(bit-identical)", file=out)

    def block(fn):
        reps, total = 0, 0.0
        while total < block_s * 1e3:
            n = 4 if reps else 1
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(n):
                fn()
            ev1.record()
            sync()
            total += ev0.elapsed_time(ev1)
            reps += n
        return total / reps

    arms = {"a": arm_a, "b": arm_b, "b'": arm_b1, "c": arm_c, "d": arm_d, "d0": arm_d0}
    for _ in range(2):
        for fn in arms.values():
            fn()
    sync()
    t = {name: [] for name in arms}
    for _ in range(blocks):
        for name, fn in arms.items():
            t[name].append(block(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    label = {"a": "a  reencrypt_sum + rescale_mult_const(1/8):", "b": "b  scale_evk + reencrypt_wsum + rescale:",
             "b'": "b' reencrypt_wsum + rescale (keys kept):", "c": "c  8 x (reencrypt + rescale_mult_const) + eval_sum:",
             "d": "d  eval_wsum (8 terms):", "d0": "d0 8 x mult_const + eval_sum:"}
    for k in arms:
        print(f"  {label[k]:52s} median {med[k]:.4f} ms  min {min(t[k]):.4f}  max {max(t[k]):.4f}", file=out)
    key_gb = 2 * C * evk_words * 8 / 1e9
    print(f"  b / a = {med['b'] / med['a']:.4f}   b' / a = {med[chr(98) + chr(39)] / med['a']:.4f}   c / a = {med['c'] / med['a']:.3f}   "
          f"c / b = {med['c'] / med['b']:.3f}   d0 / d = {med['d0'] / med['d']:.3f}", file=out)
    print(f"  b - b' = {med['b'] - med[chr(98) + chr(39)]:.4f} ms for one read and one write of the {C} keys ({key_gb:.2f} GB: "
          f"{key_gb / max(1e-9, med['b'] - med[chr(98) + chr(39)]) :.2f} TB/s)", file=out)
    print(f"  {blocks} alternating blocks per arm of >= {block_s} s, HIP-event time per pass", file=out)
    out.flush()
    g.close()


def precision(out):
    """The pair of tests/test_weighted_aggregation.py::test_weighted_mean_precision_against_the_openfhe_order."""
    try:
        import subprocess
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider",
                            os.path.join(ROOT, "tests", "test_weighted_aggregation.py"), "-k", "precision"],
                           capture_output=True, text=True, cwd=ROOT, timeout=600)
        lines = [ln for ln in r.stdout.splitlines() if "err_new" in ln]
        print("precision (decoded aggregate against the plaintext weighted mean; new order on the device, chain on the oracle):",
              file=out)
        print("  " + (lines[0] if lines else "not measured: " + r.stdout[-300:]), file=out)
    except Exception as e:  # the oracle is test infrastructure: its absence does not fail the timing run
        print(f"precision: not measured ({e})", file=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-precision", action="store_true")
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout
    run_ab(max(7, a.blocks), max(0.5, a.block_seconds), out)
    if not a.no_precision:
        precision(out)
    out.flush()


if __name__ == "__main__":
    main()
