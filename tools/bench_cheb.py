#!/usr/bin/env python3
"""A/B of the Chebyshev-series evaluation: the fused ladder step against its composition, the ladder and
mkckks_cheb_eval_batch under both forms, and mkckks_cheb_eval_batch against mkckks_poly_eval_batch at the same degree.

Leg 1: mkckks_cheb_tensor_batch, one ladder step before its relinearisation, as k_cheb_tensor (a context created under
MKCKKS_CHEB_FUSED=1, arm F) and as the composition -- packed prefix copies, k_tensor, doubling and - M t by k_wsum_ct /
k_poly_add_const, and for this entry point the copy of the packed result into the three-component output -- (a context
created under MKCKKS_CHEB_FUSED=0, arm C), on the four instances (square or general, constant or ciphertext term) with
the operands at 11, 10 and 9 limbs above a step of 9, the uneven step of a ladder.  The outputs are compared word for word
before anything is timed.  The kernel's byte rate (polynomials read + 3 written per ciphertext and limb over the HIP-event
time) stands beside a device-to-device copy that moves the same bytes.
Leg 2: mkckks_cheb_ladder_batch (n = 8) and mkckks_cheb_eval_batch (degrees 7, 15, 31 on [0.25, 4]) under the two forms.
Leg 3: mkckks_cheb_eval_batch on [-1, 1] (no map) and on [0.25, 4] (one level for the map) against mkckks_poly_eval_batch
at the same degree and limbs: the same plan and the same relinearisations.

usage: tools/bench_cheb.py [--blocks 7] [--block-seconds 0.5] [--out profiles/cheb_ab.txt]

Shape: Context(16, 10, 50, 60, dnum=3), 16 ciphertexts of 11 limbs.  One process, one card, all arrays resident, warmed,
alternating blocks of at least --block-seconds each; a block is timed with HIP events on the stream the kernels run on and
reports milliseconds per pass.  A mismatch or a missing device ends the run with a non-zero status.  Run it under a time
limit of its own (timeout 600 is ample).
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

ARGS, NL, CTS = (16, 10, 50, 60, 3), 11, 16
DEGREES = (7, 15, 31)
STEP_NL, STEP_A, STEP_B, STEP_T = 9, 10, 9, 11  # T_i, T_j and T_1 of an uneven step: read in place above the step's limbs
LADDER_N = 8


def context(fused):
    from ppqsflhe_amd import Context
    os.environ["MKCKKS_CHEB_FUSED"] = fused  # read once, when the context is created
    g = Context(*ARGS[:4], dnum=ARGS[4], device=0)  # raises without a device: no fallback
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    return g


def run_ab(blocks, block_s, out):
    g1, g0 = context("1"), context("0")
    os.environ.pop("MKCKKS_CHEB_FUSED")
    N, B_ct = g1.N, CTS
    print(f"Chebyshev series A/B on {torch.cuda.get_device_name(0)}: N = 2^{ARGS[0]}, {B_ct} ciphertexts of {NL} limbs", file=out)

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
        print(f"  {label:44s} median {statistics.median(ts):.4f} ms  min {min(ts):.4f}  max {max(ts):.4f}{extra}", file=out)

    def ratio(t, num, den):
        a, b = statistics.median(t[num]), statistics.median(t[den])
        print(f"         {num} / {den} = {a / b:.3f} x  ({num} - {den} = {a - b:.4f} ms; spread {den} {max(t[den]) - min(t[den]):.4f} ms, "
              f"{num} {max(t[num]) - min(t[num]):.4f} ms)", file=out)

    def dev(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()

    def as_torch(shape):
        return torch.zeros(shape, dtype=torch.int64, device="cuda")

    scale = g1.sf(g1.L - NL)
    x, evks = make_inputs(g1, NL, B_ct, 1, 2041)
    t_x = dev(x)
    d_rlk1, d_rlk0 = g1.to_device(evks[0]), g0.to_device(evks[0])
    rng = np.random.default_rng(2042)

    print("leg 1: one ladder step before relinearisation (cheb_tensor), arm F = k_cheb_tensor (MKCKKS_CHEB_FUSED=1), arm C = the "
          "composition (MKCKKS_CHEB_FUSED=0)", file=out)
    t_a = dev(make_inputs(g1, STEP_A, B_ct, 0, 2043)[0])
    t_b = dev(make_inputs(g1, STEP_B, B_ct, 0, 2044)[0])
    t_t = dev(make_inputs(g1, STEP_T, B_ct, 0, 2045)[0])
    s9 = g1.sf(g1.L - STEP_NL)
    for square, term in ((True, False), (False, False), (True, True), (False, True)):
        w = s9 * s9 / (s9 if term else 1.0)  # the size of a ladder's weight: S^2 for the constant, S for T_1
        t_f, t_c = as_torch((B_ct, 3, STEP_NL, N)), as_torch((B_ct, 3, STEP_NL, N))

        def step(g, o):
            g.cheb_tensor(t_a, STEP_A, t_a if square else t_b, STEP_A if square else STEP_B, t_t if term else None, STEP_T, w, o,
                          B_ct, STEP_NL)

        arms = {"F": lambda: step(g1, t_f), "C": lambda: step(g0, t_c)}
        for fn in arms.values():
            fn()
        sync()
        label = f"{'square' if square else 'general'}, {'ciphertext term T_1' if term else 'constant term'}"
        if not torch.equal(t_f, t_c):
            sys.exit(f"{label}: k_cheb_tensor differs from the composition")
        polys = (2 if square else 4) + (2 if term else 0) + 3
        moved = polys * B_ct * STEP_NL * N * 8
        c_in = torch.randint(0, 2 ** 40, (moved // 16,), dtype=torch.int64, device="cuda")  # read + written = moved
        c_out = torch.empty_like(c_in)
        arms["D"] = lambda: c_out.copy_(c_in)
        t = measure(arms)
        mf, md = statistics.median(t["F"]), statistics.median(t["D"])
        print(f"{label}: {polys - 3} polynomials read, 3 written, {STEP_NL} limbs: arm F == arm C on all words (bit-identical)", file=out)
        line("arm F (k_cheb_tensor):", t["F"], f"  ({moved / mf / 1e9:.2f} TB/s read + written, {moved / 1e6:.0f} MB)")
        line("arm C (composition):", t["C"])
        line("device-to-device copy, the same bytes:", t["D"], f"  ({moved / md / 1e9:.2f} TB/s; k_cheb_tensor / copy = {mf / md:.3f} x)")
        ratio(t, "C", "F")
        del t_f, t_c, c_in, c_out

    print("leg 2: the ladder and cheb_eval_batch, arm F under MKCKKS_CHEB_FUSED=1, arm C under MKCKKS_CHEB_FUSED=0", file=out)
    nls = [NL - (k - 1).bit_length() for k in range(1, LADDER_N + 1)]
    t_l1, t_l0 = as_torch((B_ct * 2 * N * sum(nls),)), as_torch((B_ct * 2 * N * sum(nls),))
    arms = {"F": lambda: g1.cheb_ladder(t_x, d_rlk1, t_l1, B_ct, NL, LADDER_N, scale),
            "C": lambda: g0.cheb_ladder(t_x, d_rlk0, t_l0, B_ct, NL, LADDER_N, scale)}
    for fn in arms.values():
        fn()
    sync()
    if not torch.equal(t_l1, t_l0):
        sys.exit("cheb_ladder differs between the fused and the composed step")
    t = measure(arms)
    print(f"cheb_ladder, n = {LADDER_N} ({LADDER_N - 1} steps, each with its relinearisation and rescale): bit-identical", file=out)
    line("arm F:", t["F"])
    line("arm C:", t["C"])
    ratio(t, "C", "F")
    del t_l1, t_l0
    coefs = {d: rng.uniform(-1.0, 1.0, size=d + 1) for d in DEGREES}
    for degree in DEGREES:
        p = g1.poly_plan(degree, NL - 1)
        t_e1, t_e0 = as_torch((B_ct, 2, p["nl_out"], N)), as_torch((B_ct, 2, p["nl_out"], N))
        arms = {"F": lambda: g1.cheb_eval(t_x, d_rlk1, coefs[degree], 0.25, 4.0, t_e1, B_ct, NL, scale),
                "C": lambda: g0.cheb_eval(t_x, d_rlk0, coefs[degree], 0.25, 4.0, t_e0, B_ct, NL, scale)}
        for fn in arms.values():
            fn()
        sync()
        if not torch.equal(t_e1, t_e0):
            sys.exit(f"degree {degree}: cheb_eval_batch differs between the fused and the composed step")
        t = measure(arms)
        print(f"cheb_eval_batch, degree {degree} on [0.25, 4]: {p['n_relin']} relinearisations, {NL} -> {p['nl_out']} limbs: bit-identical",
              file=out)
        line("arm F:", t["F"], f"  ({statistics.median(t['F']) / B_ct * 1e3:.1f} us per ciphertext)")
        line("arm C:", t["C"])
        ratio(t, "C", "F")
        del t_e1, t_e0

    print("leg 3: arm U = cheb_eval_batch on [-1, 1] (no map), arm M = cheb_eval_batch on [0.25, 4] (one level for the map), "
          "arm P = poly_eval_batch; the same degree, limbs and coefficients (read in the two bases: the outputs differ)", file=out)
    for degree in DEGREES:
        p, pm = g1.poly_plan(degree, NL), g1.poly_plan(degree, NL - 1)
        t_u, t_p, t_m = as_torch((B_ct, 2, p["nl_out"], N)), as_torch((B_ct, 2, p["nl_out"], N)), as_torch((B_ct, 2, pm["nl_out"], N))
        arms = {"U": lambda: g1.cheb_eval(t_x, d_rlk1, coefs[degree], -1.0, 1.0, t_u, B_ct, NL, scale),
                "M": lambda: g1.cheb_eval(t_x, d_rlk1, coefs[degree], 0.25, 4.0, t_m, B_ct, NL, scale),
                "P": lambda: g1.poly_eval(t_x, d_rlk1, coefs[degree], t_p, B_ct, NL, scale)}
        t = measure(arms)
        print(f"degree {degree}: B = {p['B']}, G = {p['G']}, {p['n_relin']} relinearisations in every arm", file=out)
        line("arm U (cheb_eval_batch, [-1, 1]):", t["U"])
        line("arm M (cheb_eval_batch, [0.25, 4]):", t["M"])
        line("arm P (poly_eval_batch):", t["P"])
        ratio(t, "U", "P")
        ratio(t, "M", "P")
        del t_u, t_p, t_m
    print(f"  {blocks} alternating blocks per arm of >= {block_s} s, HIP-event time per pass", file=out)
    out.flush()
    g1.close()
    g0.close()


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
