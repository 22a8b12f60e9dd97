#!/usr/bin/env python3
"""A/B of the per-slot aggregation weights: EvalMult(ct, plaintext) fused into the rescale against its composition.

  a   mkckks_mult_plain_rescale_batch                                  the fused call (k_ptmul_irow + k_ptresc_row)
  b   copy + mkckks_mult_plain_batch + mkckks_rescale_batch            the composition through a product ciphertext
  c   mkckks_mult_plain_rescale_batch under MKCKKS_PLAIN_FUSED=0        the library's own composition (k_mul_plain into a
                                                                       workspace + the fused rescale, no copy)
  r   mkckks_rescale_mult_const_batch(1/n)                             today's cost of the step: the anchor

Shapes: N = 2^16, nl = 12, 16 ciphertexts | N = 2^17, nl = 20, 8 ciphertexts | N = 2^16, nl = 2, 256 ciphertexts; one
plaintext per ciphertext (what the hosts pass) and, on the first shape, one plaintext for all.

usage: tools/bench_slot_weights.py [--blocks 7] [--block-seconds 0.5] [--out profiles/slot_weights_ab.txt]

One process, one card, all arrays resident, warmed, alternating blocks of at least --block-seconds each; a block is timed
with HIP events on the stream the kernels run on and reports milliseconds per pass (median, min, max over the blocks).
Before anything is timed the outputs of a, b and c are compared word for word; a mismatch or a missing device ends the
run with a non-zero status.  The fused form is the default on a ring only where its median is below both compositions'
and its block range is disjoint from theirs: the last line of every shape says which way that went.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

# (context arguments, nl, ciphertexts, plaintexts)
SHAPES = [((16, 10, 50, 60, 3), 12, 16, 16),
          ((16, 10, 50, 60, 3), 12, 16, 1),
          ((17, 18, 50, 60, 3), 20, 8, 8),
          ((16, 10, 50, 60, 3), 2, 256, 256)]


def residues(g, rng, lead, nl):
    """Canonical residues [lead..., nl, N] as a device tensor (int64 words hold the u64 bit patterns)."""
    out = np.empty(lead + (nl, g.N), dtype=np.uint64)
    for i in range(nl):
        out[..., i, :] = rng.integers(0, int(g.moduli[i]), size=lead + (g.N,), dtype=np.uint64)
    return torch.from_numpy(out.view(np.int64)).cuda()


def run_shape(args, nl, B, n_pt, blocks, block_s, out):
    from ppqsflhe_amd import Context
    g = Context(*args[:4], dnum=args[4], device=0)  # raises without a device: no fallback
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    os.environ["MKCKKS_PLAIN_FUSED"] = "0"  # switches are read once, when a context is created
    g0 = Context(*args[:4], dnum=args[4], device=0)
    del os.environ["MKCKKS_PLAIN_FUSED"]
    g0.set_stream(torch.cuda.current_stream().cuda_stream)
    N = g.N
    rng = np.random.default_rng(7)
    t_in = residues(g, rng, (B, 2), nl)
    t_pt = residues(g, rng, (n_pt,), nl)
    t_copy = torch.empty_like(t_in)
    t_a = torch.empty((B, 2, nl - 1, N), dtype=torch.int64, device="cuda")
    t_b, t_c, t_r = torch.empty_like(t_a), torch.empty_like(t_a), torch.empty_like(t_a)
    p_in, p_pt, p_copy, p_a, p_b, p_c, p_r = (t.data_ptr() for t in (t_in, t_pt, t_copy, t_a, t_b, t_c, t_r))

    def arm_a():
        g.mult_plain_rescale(p_in, p_pt, p_a, B, n_pt, nl)

    def arm_b():
        t_copy.copy_(t_in)
        g.mult_plain(p_copy, p_pt, B, n_pt, nl)
        g.rescale(p_copy, p_b, B, nl)

    def arm_c():
        g0.mult_plain_rescale(p_in, p_pt, p_c, B, n_pt, nl)

    def arm_r():
        g.rescale_mult_const(p_in, p_r, B, nl, 1.0 / 3.0)

    def sync():
        torch.cuda.synchronize()

    before = t_in.clone()
    arm_a()
    arm_b()
    arm_c()
    sync()
    if not torch.equal(t_a, t_b):
        sys.exit("mult_plain_rescale differs from copy + mult_plain + rescale")
    if not torch.equal(t_a, t_c):
        sys.exit("mult_plain_rescale differs from itself under MKCKKS_PLAIN_FUSED=0")
    if not torch.equal(t_in, before):
        sys.exit("mult_plain_rescale modified its input")
    del before

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

    arms = {"a": arm_a, "b": arm_b, "c": arm_c, "r": arm_r}
    for _ in range(2):
        for fn in arms.values():
            fn()
    sync()
    t = {name: [] for name in arms}
    for _ in range(blocks):
        for name, fn in arms.items():
            t[name].append(block(fn))
    med = {k: statistics.median(v) for k, v in t.items()}
    label = {"a": "a  mult_plain_rescale (fused):", "b": "b  copy + mult_plain + rescale:",
             "c": "c  the same call, PLAIN_FUSED=0:", "r": "r  rescale_mult_const (anchor):"}
    print(f"N = 2^{args[0]}, nl = {nl}, {B} ciphertexts, {n_pt} plaintext(s); a == b == c bit for bit, input unchanged", file=out)
    for k in arms:
        print(f"  {label[k]:34s} median {med[k]:.4f} ms  min {min(t[k]):.4f}  max {max(t[k]):.4f}", file=out)
    saved_gb = B * 4 * nl * N * 8 / 1e9  # one write and one read of the product
    disjoint = max(t["a"]) < min(t["b"]) and max(t["a"]) < min(t["c"])
    print(f"  a / b = {med['a'] / med['b']:.4f}   a / c = {med['a'] / med['c']:.4f}   a / r = {med['a'] / med['r']:.4f}   b - a = {med['b'] - med['a']:.4f} ms against "
          f"{saved_gb:.3f} GB of product traffic saved (copy not counted)", file=out)
    print(f"  fused below both compositions with disjoint block ranges: {'yes' if disjoint else 'NO'}", file=out)
    out.flush()
    g.close()
    g0.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-seconds", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = open(a.out, "w") if a.out else sys.stdout
    blocks, block_s = max(7, a.blocks), max(0.5, a.block_seconds)
    print(f"per-slot weights A/B on {torch.cuda.get_device_name(0)}: {blocks} alternating blocks per arm of >= {block_s} s, "
          f"HIP-event time per pass", file=out)
    for args, nl, B, n_pt in SHAPES:
        run_shape(args, nl, B, n_pt, blocks, block_s, out)
    out.flush()


if __name__ == "__main__":
    main()
