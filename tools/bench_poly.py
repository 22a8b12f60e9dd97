#!/usr/bin/env python3
"""A/B of the encrypted polynomial evaluation: the fused outer sum against its composition, and mkckks_poly_eval_batch
against the chain a caller without it would run.

Leg 1: mkckks_poly_tensor_batch as k_poly_tensor (a context created under MKCKKS_POLY_FUSED=1, arm F) and as the
composition -- packed prefix copies, eval_wsum's kernel per giant index, the constant column, tensor_sum's kernel, the
closing row -- (a context created under MKCKKS_POLY_FUSED=0, arm C), on the same operands and weights.  The outputs are
compared word for word before anything is timed.  The kernel's byte rate (2 (B - 1) + 2 (G - 1) polynomials read + 3 written
per ciphertext and limb over the HIP-event time) stands beside a device-to-device copy that moves the same bytes.
Leg 2: mkckks_poly_eval_batch (arm E) against the naive chain from the calls that existed before it (arm N): the powers
x^2 .. x^d by d - 1 mult_relin + rescale on level cuts (the ladder's pairing, so the chain has the depth of the ladder),
then per power a level cut to the lowest level, mult_const and eval_add.  Arm N is timed only: its terms sit at different
scales (the bookkeeping problem mkckks_poly_weights solves), so its output is not a polynomial and is compared with nothing.

usage: tools/bench_poly.py [--blocks 7] [--block-seconds 0.5] [--out profiles/poly_ab.txt]

Shape: Context(16, 10, 50, 60, dnum=3), 16 ciphertexts of 11 limbs, degrees 3, 7, 15, 31; leg 1 also runs degree 19
(B = 8, G = 3) and the largest plan B = G = 8, whose whole evaluation needs 13 limbs, on caller-supplied operands.  One
process, one card, all arrays resident, warmed, alternating blocks of at least --block-seconds each; a block is timed with
HIP events on the stream the kernels run on and reports milliseconds per pass.  A mismatch or a missing device ends the
run with a non-zero status.  Run it under a time limit of its own (timeout 600 is ample).
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
DEGREES = (3, 7, 15, 31)
# leg 1 also takes a plan with G = 3 (degree 19: B = 8) and, as None, the largest plan B = G = 8 with caller-supplied operands
LEG1 = (3, 7, 15, 19, 31, None)
LEG1_FULL = dict(B=8, G=8, nl_T=5, baby_nl=[11, 11, 10, 10, 9, 9, 9], giant_nl=[9, 8, 7, 7, 6, 6, 6])


def context(fused):
    from ppqsflhe_amd import Context
    os.environ["MKCKKS_POLY_FUSED"] = fused  # read once, when the context is created
    g = Context(*ARGS[:4], dnum=ARGS[4], device=0)  # raises without a device: no fallback
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    return g


def run_ab(blocks, block_s, out):
    g1, g0 = context("1"), context("0")
    os.environ.pop("MKCKKS_POLY_FUSED")
    N, B_ct = g1.N, CTS
    print(f"polynomial evaluation A/B on {torch.cuda.get_device_name(0)}: N = 2^{ARGS[0]}, {B_ct} ciphertexts of {NL} limbs", file=out)

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
        print(f"  {label:40s} median {statistics.median(ts):.4f} ms  min {min(ts):.4f}  max {max(ts):.4f}{extra}", file=out)

    def dev(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()

    def as_torch(shape):
        return torch.zeros(shape, dtype=torch.int64, device="cuda")

    scale = g1.sf(g1.L - NL)
    x, evks = make_inputs(g1, NL, B_ct, 1, 2031)
    t_x = dev(x)
    d_rlk1, d_rlk0 = g1.to_device(evks[0]), g0.to_device(evks[0])
    rng = np.random.default_rng(2032)
    print("leg 1: poly_tensor, arm F = k_poly_tensor (MKCKKS_POLY_FUSED=1), arm C = the composition (MKCKKS_POLY_FUSED=0)", file=out)
    for degree in LEG1:
        if degree is None:  # B = G = 8 (degree 63) does not fit 11 limbs as a whole evaluation; the outer sum takes the plan
            p = dict(LEG1_FULL)  # directly: operands as the ladders from 13 limbs would leave them, cut to 11
            cap = sum(int(m).bit_length() - 1 for m in g1.moduli[:p["nl_T"]]) - 2
            w = rng.uniform(-1.0, 1.0, size=(8, 8)) * 2.0 ** rng.integers(40, cap, size=(8, 8))
            label = "B = G = 8 (the plan of degrees 57 .. 63)"
        else:
            p = g1.poly_plan(degree, NL)
            coef = rng.uniform(-1.0, 1.0, size=degree + 1)
            w, _ = g1.poly_weights(coef, NL, scale)
            label = f"degree {degree}"
        Bp, G, nl_T = p["B"], p["G"], p["nl_T"]
        t_b = dev(np.concatenate([make_inputs(g1, nl, B_ct, 0, 2100 + i)[0].reshape(-1) for i, nl in enumerate(p["baby_nl"])]))
        t_g = dev(np.concatenate([make_inputs(g1, nl, B_ct, 0, 2200 + j)[0].reshape(-1) for j, nl in enumerate(p["giant_nl"])]))
        t_f, t_c = as_torch((B_ct, 3, nl_T, N)), as_torch((B_ct, 3, nl_T, N))
        arms = {"F": lambda: g1.poly_tensor(t_b, p["baby_nl"], t_g, p["giant_nl"], w, t_f, B_ct, nl_T),
                "C": lambda: g0.poly_tensor(t_b, p["baby_nl"], t_g, p["giant_nl"], w, t_c, B_ct, nl_T)}
        for fn in arms.values():
            fn()
        sync()
        if not torch.equal(t_f, t_c):
            sys.exit(f"{label}: k_poly_tensor differs from the composition")
        moved = (2 * (Bp - 1) + 2 * (G - 1) + 3) * B_ct * nl_T * N * 8
        c_in = torch.randint(0, 2 ** 40, (moved // 16,), dtype=torch.int64, device="cuda")  # read + written = moved
        c_out = torch.empty_like(c_in)
        arms["D"] = lambda: c_out.copy_(c_in)
        t = measure(arms)
        mf, mc, md = (statistics.median(t[k]) for k in "FCD")
        print(f"{label}: B = {Bp}, G = {G}, nl_T = {nl_T}: arm F == arm C on all words (bit-identical)", file=out)
        line("arm F (k_poly_tensor):", t["F"], f"  ({moved / mf / 1e9:.2f} TB/s read + written, {moved / 1e6:.0f} MB)")
        line("arm C (composition):", t["C"])
        line("device-to-device copy, the same bytes:", t["D"], f"  ({moved / md / 1e9:.2f} TB/s; k_poly_tensor / copy = {mf / md:.3f} x)")
        print(f"         C / F = {mc / mf:.3f} x  (C - F = {mc - mf:.4f} ms; spread F {max(t['F']) - min(t['F']):.4f} ms, "
              f"C {max(t['C']) - min(t['C']):.4f} ms)", file=out)
        del t_b, t_g, t_f, t_c, c_in, c_out
    print("leg 2: arm E = poly_eval_batch, arm N = the naive chain (d - 1 mult_relin + rescale, then level cut + mult_const + "
          "eval_add per power; timed only)", file=out)
    for degree in DEGREES:
        p = g1.poly_plan(degree, NL)
        coef = rng.uniform(-1.0, 1.0, size=degree + 1)
        t_e1, t_e0 = as_torch((B_ct, 2, p["nl_out"], N)), as_torch((B_ct, 2, p["nl_out"], N))
        nls = [NL - (k - 1).bit_length() for k in range(1, degree + 1)]
        nl_min = nls[-1]
        pw = {1: t_x}
        for k in range(2, degree + 1):
            pw[k] = as_torch((B_ct, 2, nls[k - 1], N))
        t_cut, t_prod = as_torch((B_ct, 2, NL, N)), as_torch((B_ct, 2, NL, N))
        t_term, t_acc = as_torch((B_ct, 2, nl_min, N)), as_torch((B_ct, 2, nl_min, N))

        def naive():
            for k in range(2, degree + 1):
                i = (k + 1) // 2
                j = k - i
                nli = nls[i - 1]
                a, b = pw[i], pw[j]
                if nls[j - 1] != nli:
                    cut = t_cut.view(-1)[:B_ct * 2 * nli * N].view(B_ct, 2, nli, N)
                    cut.copy_(b[:, :, :nli])
                    b = cut
                prod = t_prod.view(-1)[:B_ct * 2 * nli * N].view(B_ct, 2, nli, N)
                g1.mult_relin(a, b, d_rlk1, prod, B_ct, nli)
                g1.rescale(prod, pw[k], B_ct, nli)
            t_acc.zero_()
            for k in range(1, degree + 1):
                t_term.copy_(pw[k][:, :, :nl_min])
                g1.mult_const(t_term, B_ct, nl_min, float(coef[k]))
                g1.eval_add(t_acc, t_term, t_acc, B_ct, nl_min)

        arms = {"E": lambda: g1.poly_eval(t_x, d_rlk1, coef, t_e1, B_ct, NL, scale),
                "N": naive}
        g1.poly_eval(t_x, d_rlk1, coef, t_e1, B_ct, NL, scale)
        g0.poly_eval(t_x, d_rlk0, coef, t_e0, B_ct, NL, scale)
        sync()
        if not torch.equal(t_e1, t_e0):
            sys.exit(f"degree {degree}: poly_eval_batch differs between the fused and the composed outer sum")
        t = measure(arms)
        me, mn = statistics.median(t["E"]), statistics.median(t["N"])
        print(f"degree {degree}: {p['n_relin']} relinearisations against {degree - 1}; {NL} -> {p['nl_out']} limbs (arm N ends on {nl_min}); "
              f"arm E under MKCKKS_POLY_FUSED=0 and =1 bit-identical", file=out)
        line("arm E (poly_eval_batch):", t["E"], f"  ({me / B_ct * 1e3:.1f} us per ciphertext)")
        line("arm N (naive chain):", t["N"])
        print(f"         N / E = {mn / me:.3f} x  (N - E = {mn - me:.4f} ms; spread E {max(t['E']) - min(t['E']):.4f} ms, "
              f"N {max(t['N']) - min(t['N']):.4f} ms)", file=out)
        del pw, t_cut, t_prod, t_term, t_acc, t_e1, t_e0
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
