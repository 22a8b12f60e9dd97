#!/usr/bin/env python3
"""A/B of the double-hoisted linear transform: mkckks_linear_transform_batch against the public calls that compose it.

Arm F is mkckks_linear_transform_batch on n_rot diagonals (one ModUp per ciphertext, k_lt_accum, one ModDown per
component).  Arm C is the composition a caller without it would run: per diagonal mkckks_rotate_batch into slot r of a
[n_rot][B] buffer and mkckks_mult_plain_batch there with the diagonal's Q limbs, then one mkckks_eval_sum_batch over the
n_rot slots.  Arms F1 and F2 are arm F on contexts created under MKCKKS_LT_ORDER=1 (a workgroup walks the chunk's
ciphertexts) and MKCKKS_LT_ORDER=2 (ciphertext-major grid, no reuse of key tiles intended); arm F itself is order 0
(the workgroups of one (limb, tile) are neighbours on one XCD).  Arms U and D are mkckks_modup_batch on the B polynomials
c1 and mkckks_moddown_batch on 2 B extended polynomials: what arm F runs around its accumulate kernel, so F - U - D
estimates k_lt_accum alone (U also copies the digits' own limbs, which arm F does not: the estimate is a little low).

usage: tools/bench_linear_transform.py [--blocks 7] [--block-seconds 0.5] [--out profiles/linear_transform_ab.txt]

Shapes: Context(16, 10, 50, 60, dnum=3), 16 ciphertexts of 11 limbs, n_rot 4, 16 and 64; Context(17, 18, 50, 60, dnum=3), 16
ciphertexts of 20 limbs, n_rot 16.  One process, one card, all arrays resident and filled on the device (residues below
2^40 are canonical for every modulus here), warmed, alternating blocks of at least --block-seconds each; a block is timed
with HIP events on the stream the kernels run on and reports milliseconds per pass.  The rotations are 5^1 .. 5^(n_rot-1)
and one unrotated diagonal.  Arms F, F1, F2 are compared word for word before anything is timed.  Requirement checked at
the end: at n_rot = 16 the slowest block of arm F is below the fastest block of arm C; a miss, a mismatch or a missing
device ends the run with a non-zero status.  Run it under a time limit of its own (timeout 900 is ample).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = [((16, 10, 50, 60, 3), 11, 16, (4, 16, 64)), ((17, 18, 50, 60, 3), 20, 16, (16,))]
COPY_TBS = 5.97  # profiles/r03_ubench_hbm.txt, "copy 1 : 1"


def run_ab(blocks, block_s, out):
    from ppqsflhe_amd import Context
    print(f"linear transform A/B on {torch.cuda.get_device_name(0)}: arm F = linear_transform_batch (key reuse by grid order), "
          f"F1 = the same with the ciphertext walk, F2 = ciphertext-major grid, arm C = n_rot x (rotate_batch + "
          f"mult_plain_batch) + eval_sum_batch, U = modup_batch, D = moddown_batch", file=out)

    def sync():
        torch.cuda.synchronize()

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

    def measure(arms):
        for _ in range(2):
            for fn in arms.values():
                fn()
        sync()
        t = {name: [] for name in arms}
        for _ in range(blocks):
            for name, fn in arms.items():
                t[name].append(block(fn))
        return t

    def line(label, ts, extra=""):
        print(f"  {label:44s} median {statistics.median(ts):9.4f} ms  min {min(ts):9.4f}  max {max(ts):9.4f}{extra}", file=out)

    def rnd(shape):
        return torch.randint(0, 2 ** 40, shape, dtype=torch.int64, device="cuda")

    def make_ctx(args, order):
        os.environ["MKCKKS_LT_ORDER"] = str(order)  # switches are read once, when a context is created
        try:
            g = Context(*args[:4], dnum=args[4], device=0)  # raises without a device: no fallback
        finally:
            del os.environ["MKCKKS_LT_ORDER"]
        g.set_stream(torch.cuda.current_stream().cuda_stream)
        return g

    ok = True
    for args, nl, B, rots in SHAPES:
        g, g1, g2 = (make_ctx(args, order) for order in (0, 1, 2))
        N, K, D, beta = g.N, g.K, g.D, g.beta
        ext, nparts = nl + K, min(beta, -(-nl // g.alpha))
        ct = rnd((B, 2, nl, N))
        dig, til = g.empty((B, nparts, ext, N)), rnd((2 * B, ext, N))
        d_md = g.empty((2 * B, nl, N))
        c1 = ct[:, 1].contiguous()
        for n_rot in rots:
            evks, pts = rnd((n_rot, beta, 2, D, N)), rnd((n_rot, ext, N))
            gs = [1] + [g.galois_element(r) for r in range(1, n_rot)]
            o0, o1, o2 = (torch.empty_like(ct) for _ in range(3))
            comp, o_c = torch.empty((n_rot, B, 2, nl, N), dtype=torch.int64, device="cuda"), torch.empty_like(ct)

            def composition():
                for r in range(n_rot):
                    if gs[r] == 1:
                        comp[r].copy_(ct)
                    else:
                        g.rotate(ct, evks[r], comp[r], B, nl, gs[r])
                    g.mult_plain(comp[r], pts[r], B, 1, nl)  # the diagonal's Q limbs are the head of its extended plaintext
                g.eval_sum(comp, o_c, n_rot, B, nl)

            arms = {"F": lambda: g.linear_transform(ct, evks, pts, gs, o0, B, nl),
                    "F1": lambda: g1.linear_transform(ct, evks, pts, gs, o1, B, nl),
                    "F2": lambda: g2.linear_transform(ct, evks, pts, gs, o2, B, nl),
                    "C": composition,
                    "U": lambda: g.modup(c1, dig, B, nl),
                    "D": lambda: g.moddown(til, d_md, 2 * B, nl)}
            for fn in arms.values():
                fn()
            sync()
            if not (torch.equal(o0, o1) and torch.equal(o0, o2)):
                sys.exit(f"N={N} nl={nl} n_rot={n_rot}: the key-reuse orders of k_lt_accum differ")
            t = measure(arms)
            m = {k: statistics.median(v) for k, v in t.items()}
            print(f"N = 2^{args[0]}, {B} ciphertexts of {nl} limbs ({nparts} digits, K = {K}), n_rot = {n_rot}: arms F, F1, F2 "
                  f"bit-identical", file=out)
            line("arm F (linear_transform, grid order):", t["F"], f"  ({m['F'] / n_rot:.4f} ms per diagonal)")
            line("arm F1 (linear_transform, walk):", t["F1"], f"  (F1 / F = {m['F1'] / m['F']:.3f} x)")
            line("arm F2 (linear_transform, ct-major grid):", t["F2"], f"  (F2 / F = {m['F2'] / m['F']:.3f} x)")
            line("arm C (rotate + mult_plain, eval_sum):", t["C"], f"  ({m['C'] / n_rot:.4f} ms per diagonal)")
            line("arm U (modup_batch, B polynomials):", t["U"])
            line("arm D (moddown_batch, 2 B polynomials):", t["D"])
            acc = m["F"] - m["U"] - m["D"]
            keyed = n_rot - 1
            # bytes the workgroups of k_lt_accum request: per rotation and (ciphertext, extended row) the digit tiles, c0 on
            # the Q rows, 2 key rows per digit and the plaintext row; the output once
            rows = B * keyed * (ext * (3 * nparts + 1) + nl) + B * (ext + 2 * nl) + B * 2 * ext
            nbytes = rows * N * 8
            once = (keyed * (2 * nparts + 1) * ext + ext + B * (nparts * ext + 2 * nl) + B * 2 * ext) * N * 8
            print(f"         C / F = {m['C'] / m['F']:.3f} x;  slowest F block {max(t['F']):.4f} ms, fastest C block {min(t['C']):.4f} ms", file=out)
            print(f"         k_lt_accum by difference F - U - D = {acc:.4f} ms: {nbytes / 1e9:.2f} GB requested by its workgroups "
                  f"({nbytes / acc / 1e9:.2f} TB/s), {once / 1e9:.2f} GB if every array is fetched once ({once / acc / 1e9:.2f} TB/s; "
                  f"streaming copy {COPY_TBS} TB/s, profiles/r03_ubench_hbm.txt)", file=out)
            if n_rot == 16 and not max(t["F"]) < min(t["C"]):
                ok = False
                print("         REQUIREMENT MISSED: the slowest block of arm F is not below the fastest block of arm C", file=out)
            del evks, pts, comp, o0, o1, o2, o_c
            torch.cuda.empty_cache()
        for c in (g, g1, g2):
            c.close()
        del ct, til, c1
        torch.cuda.empty_cache()
    print(f"  {blocks} alternating blocks per arm of >= {block_s} s, HIP-event time per pass", file=out)
    print("  requirement (n_rot = 16: slowest F block below fastest C block): " + ("met" if ok else "MISSED"), file=out)
    out.flush()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout
    sys.exit(0 if run_ab(max(7, a.blocks), max(0.5, a.block_seconds), out) else 1)


if __name__ == "__main__":
    main()
