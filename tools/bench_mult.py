#!/usr/bin/env python3
"""A/B of the ciphertext product: mkckks_mult_relin_batch against the entry points that existed before it, and k_tensor
against a copy.

Arm M is mkckks_mult_relin_batch(a, b, rlk).  Arm C is the composition a caller without it would run, from the public
calls: X = copy(a), Y = copy(a) (mult_plain works in place); mult_plain(X, b0) = (a0 b0, a1 b0); mult_plain(Y, b1) =
(a0 b1, a1 b1); the two components of Y are copied into the c1 halves of two ciphertext arrays whose c0 stays zero;
eval_add(X, (0, a0 b1)) = (d0, d1); reencrypt((0, a1 b1), rlk); eval_add of the two.  b0 and b1 are split out of b before
anything is timed (in favour of arm C).  Arm A is arm C with mkckks_reencrypt_accumulate_batch in place of the last
reencrypt + eval_add.  Arm P is mkckks_reencrypt_batch alone on a: the floor, a product without its tensor.  Arm T is
mkckks_tensor_sum_batch with one term alone; its byte rate (4 polynomials read + 3 written per ciphertext and limb over
the HIP-event time) stands beside a device-to-device copy that moves the same bytes, timed in the same process on buffers
larger than the Infinity Cache.

usage: tools/bench_mult.py [--blocks 7] [--block-seconds 0.5] [--out profiles/mult_ab.txt]

Shapes: Context(16, 10, 50, 60, dnum=3), 16 ciphertexts of 11 limbs and of 2 limbs; Context(17, 2, 50, 60, dnum=2), 16
ciphertexts of 4 limbs.  One process, one card, all arrays resident, warmed, alternating blocks (M, C, A, P, T, M, ...) of
at least --block-seconds each; a block is timed with HIP events on the stream the kernels run on and reports milliseconds
per pass.  Arms M, C and A are compared word for word before anything is timed; a mismatch or a missing device ends the
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

SHAPES = [((16, 10, 50, 60, 3), 11, 16, True), ((16, 10, 50, 60, 3), 2, 16, False), ((17, 2, 50, 60, 2), 4, 16, False)]
STREAM_CTS = 64  # ciphertexts of the byte-rate measurement: 2 x 738 MB read, 1107 MB written at N = 2^16, 11 limbs


def run_ab(blocks, block_s, out):
    from ppqsflhe_amd import Context
    print(f"ciphertext product A/B on {torch.cuda.get_device_name(0)}: arm M = mult_relin_batch, arm C = copies + mult_plain x 2 + "
          f"eval_add + reencrypt + eval_add, arm A = the same with reencrypt_accumulate, arm P = reencrypt_batch alone, "
          f"arm T = tensor_sum_batch alone", file=out)

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
        print(f"  {label:36s} median {statistics.median(ts):.4f} ms  min {min(ts):.4f}  max {max(ts):.4f}{extra}", file=out)

    def as_torch(shape):
        return torch.zeros(shape, dtype=torch.int64, device="cuda")

    ctx = {}
    for args, nl, B, with_rate in SHAPES:
        if args not in ctx:
            ctx[args] = Context(*args[:4], dnum=args[4], device=0)  # raises without a device: no fallback
            ctx[args].set_stream(torch.cuda.current_stream().cuda_stream)
        g = ctx[args]
        N = g.N
        a, evks = make_inputs(g, nl, B, 1, 2029)
        b, _ = make_inputs(g, nl, B, 0, 2030)
        shape = (B, 2, nl, N)
        t_a = torch.from_numpy(a.view(np.int64)).cuda()
        t_b = torch.from_numpy(b.view(np.int64)).cuda()
        t_b0, t_b1 = t_b[:, 0].contiguous(), t_b[:, 1].contiguous()  # the plaintext operands of arm C, split beforehand
        d_rlk = g.to_device(evks[0])
        t_x, t_y, t_z1, t_z2, t_d, t_r, t_c, t_acc, t_m, t_p = (as_torch(shape) for _ in range(10))
        t_out3 = as_torch((B, 3, nl, N))

        def composition(accumulate):
            t_x.copy_(t_a)
            t_y.copy_(t_a)
            g.mult_plain(t_x, t_b0, B, B, nl)
            g.mult_plain(t_y, t_b1, B, B, nl)
            t_z1[:, 1].copy_(t_y[:, 0])  # (0, a0 b1)
            t_z2[:, 1].copy_(t_y[:, 1])  # (0, a1 b1)
            if accumulate:
                g.eval_add(t_x, t_z1, t_acc, B, nl)
                g.reencrypt_accumulate(t_z2, d_rlk, t_acc, B, nl)
            else:
                g.eval_add(t_x, t_z1, t_d, B, nl)
                g.reencrypt(t_z2, d_rlk, t_r, B, nl)
                g.eval_add(t_d, t_r, t_c, B, nl)

        arms = {"M": lambda: g.mult_relin(t_a, t_b, d_rlk, t_m, B, nl),
                "C": lambda: composition(False),
                "A": lambda: composition(True),
                "P": lambda: g.reencrypt(t_a, d_rlk, t_p, B, nl),
                "T": lambda: g.tensor_sum(t_a, t_b, t_out3, 1, B, nl)}
        for fn in arms.values():
            fn()
        sync()
        if not (torch.equal(t_m, t_c) and torch.equal(t_m, t_acc)):
            sys.exit(f"N={N} nl={nl}: mkckks_mult_relin_batch differs from the composition of the public calls")
        if not (torch.equal(t_out3[:, 0], t_x[:, 0]) and torch.equal(t_out3[:, 2], t_y[:, 1])):
            sys.exit(f"N={N} nl={nl}: mkckks_tensor_sum_batch differs from mult_plain on d0 / d2")
        t = measure(arms)
        mm, mc, ma, mp, mt = (statistics.median(t[k]) for k in "MCAPT")
        nbytes = 7 * B * nl * N * 8
        print(f"N = 2^{args[0]}, {B} ciphertexts of {nl} limb(s): arm M == arm C == arm A on all words (bit-identical)", file=out)
        line("arm M (mult_relin_batch):", t["M"], f"  ({mm / B * 1e3:.2f} us per ciphertext)")
        line("arm C (composition, eval_add last):", t["C"])
        line("arm A (composition, accumulate):", t["A"])
        line("arm P (reencrypt alone):", t["P"])
        line("arm T (tensor_sum alone):", t["T"], f"  ({nbytes / mt / 1e9:.2f} TB/s read + written, {nbytes / 1e6:.0f} MB)")
        print(f"         C / M = {mc / mm:.3f} x  (C - M = {mc - mm:.4f} ms; spread M {max(t['M']) - min(t['M']):.4f} ms, "
              f"C {max(t['C']) - min(t['C']):.4f} ms)", file=out)
        print(f"         A / M = {ma / mm:.3f} x  (A - M = {ma - mm:.4f} ms; spread A {max(t['A']) - min(t['A']):.4f} ms)", file=out)
        print(f"         M / P = {mm / mp:.3f} x  (M - P = {mm - mp:.4f} ms, tensor alone {mt:.4f} ms; spread P "
              f"{max(t['P']) - min(t['P']):.4f} ms)", file=out)
        del t_x, t_y, t_z1, t_z2, t_d, t_r, t_c, t_acc, t_m, t_p, t_out3
        if with_rate:
            # byte rate of k_tensor beside a copy, both on buffers beyond the Infinity Cache
            words = STREAM_CTS * 2 * nl * N
            s_a = torch.randint(0, 2 ** 40, (words,), dtype=torch.int64, device="cuda")
            s_b = torch.randint(0, 2 ** 40, (words,), dtype=torch.int64, device="cuda")
            s_o = torch.empty(words // 2 * 3, dtype=torch.int64, device="cuda")
            moved = 7 * STREAM_CTS * nl * N * 8
            c_in = torch.randint(0, 2 ** 40, (moved // 16,), dtype=torch.int64, device="cuda")  # read + written = moved
            c_out = torch.empty_like(c_in)
            tb = measure({"K": lambda: g.tensor_sum(s_a, s_b, s_o, 1, STREAM_CTS, nl),
                          "Q": lambda: g.tensor_sum(s_a, s_a, s_o, 1, STREAM_CTS, nl),
                          "D": lambda: c_out.copy_(c_in)})
            mk_, mq, md = (statistics.median(tb[k]) for k in "KQD")
            sq_moved = 5 * STREAM_CTS * nl * N * 8
            print(f"  byte rate, {STREAM_CTS} ciphertexts of {nl} limbs ({moved / 1e6:.0f} MB read + written per pass):", file=out)
            line("k_tensor:", tb["K"], f"  ({moved / mk_ / 1e9:.2f} TB/s)")
            line("device-to-device copy:", tb["D"], f"  ({moved / md / 1e9:.2f} TB/s; k_tensor / copy = {mk_ / md:.3f} x)")
            line("k_tensor, square instance:", tb["Q"], f"  ({sq_moved / mq / 1e9:.2f} TB/s on its {sq_moved / 1e6:.0f} MB)")
            del s_a, s_b, s_o, c_in, c_out
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
