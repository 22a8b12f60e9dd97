#!/usr/bin/env python3
"""A/B of the collective evaluation keys: the fused mkckks_relin_share (k_relshare_col + k_relshare_row) against its
composition (k_lift x 2 + the forward transform over D limbs + k_fma x 2), and mkckks_evk_sum beside a copy.

Arm F is mkckks_relin_share in a context created with the library's defaults, arm C the same call in a context created
under MKCKKS_RELSHARE_FUSED=0 (switches are read once, when a context is created); both contexts live in this process and
work on the same device arrays.  Arm S is mkckks_evk_sum of 8 parties x 15 keys; its byte rate (8 keys read + 1 written
per key over the HIP-event time) stands beside a device-to-device copy that moves the same bytes, timed in the same
process.

usage: tools/bench_collective_keys.py [--blocks 7] [--block-seconds 0.5] [--out profiles/collective_keys_ab.txt]

Shapes: Context(16, 10, 50, 60, dnum=3) (N = 2^16, beta = 3, D = 16: a key is 50 MB) and Context(17, 2, 50, 60, dnum=2)
(N = 2^17, where the row pass has no two-round radix kernel: both arms take the composition, and the profile says so).
One process, one card, all arrays resident, warmed, alternating blocks (F, C, F, ...) of at least --block-seconds each; a
block is timed with HIP events on the stream the kernels run on and reports milliseconds per pass.  The arms are compared
word for word before anything is timed; a mismatch or a missing device ends the run with a non-zero status.  Run it under
a time limit of its own (timeout 600 is ample).
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = [(16, 10, 50, 60, 3), (17, 2, 50, 60, 2)]
SUM_PARTIES, SUM_KEYS = 8, 15


def rand_limbs(g, rng, lead):
    """uniform residues u64[lead...][D][N]"""
    out = np.empty(lead + (g.D, g.N), dtype=np.uint64)
    for i in range(g.D):
        out[..., i, :] = rng.integers(0, int(g.moduli[i]), size=lead + (g.N,), dtype=np.uint64)
    return out


def run_ab(blocks, block_s, out):
    from ppqsflhe_amd import Context
    print(f"collective evaluation keys A/B on {torch.cuda.get_device_name(0)}: arm F = relin_share (library default), "
          f"arm C = relin_share under MKCKKS_RELSHARE_FUSED=0 (lift + transform + multiply-add), arm S = evk_sum", file=out)

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

    def context(args, fused):
        if fused:
            os.environ.pop("MKCKKS_RELSHARE_FUSED", None)
        else:
            os.environ["MKCKKS_RELSHARE_FUSED"] = "0"
        try:
            g = Context(*args[:4], dnum=args[4], device=0)  # raises without a device: no fallback
        finally:
            os.environ.pop("MKCKKS_RELSHARE_FUSED", None)
        g.set_stream(torch.cuda.current_stream().cuda_stream)
        return g

    for args in SHAPES:
        gf, gc = context(args, True), context(args, False)
        N, D, beta = gf.N, gf.D, gf.beta
        rng = np.random.default_rng(2031)
        key1, sk = rand_limbs(gf, rng, (beta, 2)), rand_limbs(gf, rng, ())
        e0 = np.rint(rng.normal(0.0, 3.19, size=(beta, N))).astype(np.int32)
        e1 = np.rint(rng.normal(0.0, 3.19, size=(beta, N))).astype(np.int32)
        t_key1 = torch.from_numpy(key1.view(np.int64)).cuda()
        t_sk = torch.from_numpy(sk.view(np.int64)).cuda()
        t_e0, t_e1 = torch.from_numpy(e0).cuda(), torch.from_numpy(e1).cuda()
        t_f, t_c = torch.zeros_like(t_key1), torch.zeros_like(t_key1)
        arms = {"F": lambda: gf.relin_share(t_key1, t_sk, t_e0, t_e1, t_f),
                "C": lambda: gc.relin_share(t_key1, t_sk, t_e0, t_e1, t_c)}
        for fn in arms.values():
            fn()
        sync()
        if not torch.equal(t_f, t_c):
            sys.exit(f"N={N}: the fused mkckks_relin_share differs from its composition")
        t = measure(arms)
        mf, mc = statistics.median(t["F"]), statistics.median(t["C"])
        key_mb = beta * 2 * D * N * 8 / 1e6
        print(f"N = 2^{args[0]}, beta = {beta}, D = {D} (a key is {key_mb:.0f} MB): arm F == arm C on all words (bit-identical)", file=out)
        line("arm F (relin_share, default):", t["F"])
        line("arm C (relin_share, composition):", t["C"])
        disjoint = max(t["F"]) < min(t["C"])
        print(f"         C / F = {mc / mf:.3f} x  (C - F = {mc - mf:.4f} ms; spread F {max(t['F']) - min(t['F']):.4f} ms, "
              f"C {max(t['C']) - min(t['C']):.4f} ms; F's blocks {'lie disjoint below' if disjoint else 'overlap'} C's)", file=out)
        del t_f, t_c
        if args == SHAPES[0]:
            words = SUM_KEYS * beta * 2 * D * N
            s_in = torch.randint(0, 2 ** 40, (SUM_PARTIES * words,), dtype=torch.int64, device="cuda")
            s_out = torch.empty(words, dtype=torch.int64, device="cuda")
            moved = (SUM_PARTIES + 1) * words * 8
            c_in = torch.randint(0, 2 ** 40, (moved // 16,), dtype=torch.int64, device="cuda")  # read + written = moved
            c_out = torch.empty_like(c_in)
            ts = measure({"S": lambda: gf.evk_sum(s_in, s_out, SUM_PARTIES, SUM_KEYS), "D": lambda: c_out.copy_(c_in)})
            ms, md = statistics.median(ts["S"]), statistics.median(ts["D"])
            print(f"  evk_sum, {SUM_PARTIES} parties x {SUM_KEYS} keys ({moved / 1e6:.0f} MB read + written per pass):", file=out)
            line("arm S (evk_sum):", ts["S"], f"  ({moved / ms / 1e9:.2f} TB/s)")
            line("device-to-device copy:", ts["D"], f"  ({moved / md / 1e9:.2f} TB/s; evk_sum / copy = {ms / md:.3f} x)")
            del s_in, s_out, c_in, c_out
        gf.close()
        gc.close()
    print(f"  {blocks} alternating blocks per arm of >= {block_s} s, HIP-event time per pass", file=out)
    out.flush()


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
