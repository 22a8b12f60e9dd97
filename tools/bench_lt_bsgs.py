#!/usr/bin/env python3
"""A/B of the baby-step giant-step linear transform: mkckks_linear_transform_bsgs_batch against its composition arm and
against the direct mkckks_linear_transform_batch on the same diagonals.

Arm B is mkckks_linear_transform_bsgs_batch (k_bsgs_baby, k_bsgs_inner, one ModDown and one ModUp over the keyed giants,
k_bsgs_giant).  Arm B0 is the same call on a context created under MKCKKS_BSGS_FUSED=0: the same sums from k_lt_accum (one
rotation, an all-ones plaintext) per baby and per giant, k_fma and k_automorph.  Arm L is the direct double-hoisted
mkckks_linear_transform_batch with one key per non-zero step.  Arms B and B0 are compared word for word before anything is
timed (arm L computes the same transform by another route: other roundings, other words).

usage: tools/bench_lt_bsgs.py [--blocks 7] [--block-seconds 0.5] [--no-phases] [--out profiles/lt_bsgs_ab.txt]

Shape: Context(16, 10, 50, 60, dnum=3), 16 ciphertexts of 11 limbs.  Cases: 64 diagonals (steps 0 .. 63) as 8 x 8 and as
16 x 4; 255 diagonals (steps -127 .. 127, the 128 x 128 block) as 16 x 16 and as 32 x 8, entry (G, b) = (-128, 0) absent.
One process, one card, all arrays resident and filled on the device (residues below 2^40 are canonical for every modulus
here), warmed, alternating blocks of at least --block-seconds each; a block is timed with HIP events on the stream the
kernels run on and reports milliseconds per pass.  Key bytes are those of the Galois keys each arm reads.

Per-phase times of arm B come from a kernel trace of its own: for every case the tool starts a fresh child process under
`rocprofv3 --kernel-trace` (this file with --trace-case) that runs three passes, and cuts the last pass's dispatches at
its three named kernels: what precedes k_bsgs_baby is the ModUp of c1, between k_bsgs_inner and k_bsgs_giant lie the
giants' ModDown and ModUp, after k_bsgs_giant the closing ModDown (kernel durations added up, per chunk, summed over the
chunks of a pass).  k_bsgs_inner's bytes: requested by its workgroups against every array fetched once.

Requirement checked at the end: at 255 diagonals with n1 = 32 the slowest block of arm B is below the fastest block of arm
L; a miss, a mismatch or a missing device ends the run with a non-zero status.  Run it under a time limit of its own.
"""
import argparse
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

ARGS, NL, B = (16, 10, 50, 60, 3), 11, 16
# (label, steps, n1)
CASES = [("64 diagonals as 8 x 8", range(0, 64), 8), ("64 diagonals as 16 x 4", range(0, 64), 16),
         ("255 diagonals as 16 x 16", range(-127, 128), 16), ("255 diagonals as 32 x 8", range(-127, 128), 32)]
REQUIRED = 3  # index in CASES
BABY_GROUP, GIANT_GROUP = 8, 4  # BSGS_GROUP, BSGS_GIANTS of ppqsflhe_amd/csrc/bsgs_kernels.hpp


def plan(steps, n1):
    """(baby steps, giant steps, present[n2][n1]) by the rule of ppqsflhe_amd/host/bsgs.hpp"""
    steps = set(steps)
    giants = sorted({r - r % n1 for r in steps})
    return list(range(n1)), giants, [[1 if G + b in steps else 0 for b in range(n1)] for G in giants]


def rnd(shape):
    return torch.randint(0, 2 ** 40, shape, dtype=torch.int64, device="cuda")


def make_ctx(fused):
    from ppqsflhe_amd import Context
    os.environ["MKCKKS_BSGS_FUSED"] = str(fused)  # switches are read once, when a context is created
    try:
        g = Context(*ARGS[:4], dnum=ARGS[4], device=0)  # raises without a device: no fallback
    finally:
        del os.environ["MKCKKS_BSGS_FUSED"]
    g.set_stream(torch.cuda.current_stream().cuda_stream)
    return g


def bsgs_inputs(g, steps, n1):
    babies, giants, present = plan(steps, n1)
    ext = NL + g.K
    gb, gg = [g.galois_element(b) for b in babies], [g.galois_element(G) for G in giants]
    bkeys, gkeys = rnd((len(babies), g.beta, 2, g.D, g.N)), rnd((len(giants), g.beta, 2, g.D, g.N))
    pts = rnd((len(giants), len(babies), ext, g.N))
    return gb, gg, present, bkeys, gkeys, pts


def trace_case(i):
    """child under rocprofv3: three passes of arm B of case i"""
    g = make_ctx(1)
    _, steps, n1 = CASES[i]
    gb, gg, present, bkeys, gkeys, pts = bsgs_inputs(g, steps, n1)
    ct = rnd((B, 2, NL, g.N))
    out = torch.empty_like(ct)
    for _ in range(3):
        g.linear_transform_bsgs(ct, bkeys, gb, gkeys, gg, pts, present, out, B, NL)
    torch.cuda.synchronize()
    g.close()


def phases(i):
    """per-phase kernel time (ms per pass) of arm B of case i from a kernel trace, or None where the tracer is missing"""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.access(prof, os.X_OK):
        return None
    d = tempfile.mkdtemp(prefix="lt_bsgs_trace_")
    try:
        r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--trace-case", str(i)], capture_output=True, text=True, timeout=600)
        files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
        if r.returncode != 0 or not files:
            return None
        ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(files[0]))
                    if "mk::" in r["Kernel_Name"])
    finally:
        shutil.rmtree(d, ignore_errors=True)
    baby = [k for k, e in enumerate(ev) if "k_bsgs_baby" in e[2]]
    if not baby or len(baby) % 3:
        return None
    chunks = len(baby) // 3
    head = baby[0]  # dispatches of a ModUp of c1: what precedes the first baby kernel
    names = ("ModUp of c1", "babies (k_bsgs_baby)", "inner sums (k_bsgs_inner)", "giants' ModDown and ModUp",
             "giant accumulate (k_bsgs_giant)", "closing ModDown")
    t = dict.fromkeys(names, 0.0)
    # a chunk: `head` dispatches, baby, inner, [giants' ModDown + ModUp], giant, closing ModDown; the last pass's chunks
    starts = [k - head for k in baby[2 * chunks:]] + [len(ev)]
    for c in range(chunks):
        stage = 0
        for k in range(starts[c], starts[c + 1]):
            s0, e0, name = ev[k]
            if "k_bsgs_baby" in name:
                stage = 1
            elif "k_bsgs_inner" in name:
                stage = 2
            elif "k_bsgs_giant" in name:
                stage = 4
            elif stage in (2, 4):
                stage += 1
            t[names[stage]] += e0 - s0
    return {name: v / 1e6 for name, v in t.items()}, chunks


def run_ab(blocks, block_s, with_phases, out):
    print(f"baby-step giant-step linear transform A/B on {torch.cuda.get_device_name(0)}: arm B = linear_transform_bsgs_batch, "
          f"B0 = the same under MKCKKS_BSGS_FUSED=0 (k_lt_accum per baby and per giant, k_fma, k_automorph), arm L = "
          f"linear_transform_batch with one key per non-zero step", file=out)

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

    g, g0 = make_ctx(1), make_ctx(0)
    N, K, D, beta = g.N, g.K, g.D, g.beta
    ext, nparts = NL + K, min(beta, -(-NL // g.alpha))
    key_bytes = beta * 2 * D * N * 8
    ct = rnd((B, 2, NL, N))
    ok = True
    for i, (label, steps, n1) in enumerate(CASES):
        gb, gg, present, bkeys, gkeys, pts = bsgs_inputs(g, steps, n1)
        n2, n_pres = len(gg), sum(map(sum, present))
        gs = [g.galois_element(r) for r in steps]
        evks, lpts = rnd((len(gs), beta, 2, D, N)), rnd((len(gs), ext, N))
        o_b, o_b0, o_l = (torch.empty_like(ct) for _ in range(3))
        arms = {"B": lambda: g.linear_transform_bsgs(ct, bkeys, gb, gkeys, gg, pts, present, o_b, B, NL),
                "B0": lambda: g0.linear_transform_bsgs(ct, bkeys, gb, gkeys, gg, pts, present, o_b0, B, NL),
                "L": lambda: g.linear_transform(ct, evks, lpts, gs, o_l, B, NL)}
        for fn in arms.values():
            fn()
        sync()
        if not torch.equal(o_b, o_b0):
            sys.exit(f"{label}: the fused kernels and the composition arm differ")
        t = measure(arms)
        m = {k: statistics.median(v) for k, v in t.items()}
        kb, kg, kl = sum(x != 1 for x in gb), sum(x != 1 for x in gg), sum(x != 1 for x in gs)
        print(f"N = 2^{ARGS[0]}, {B} ciphertexts of {NL} limbs ({nparts} digits, K = {K}), {label} ({n_pres} present entries): arms B "
              f"and B0 bit-identical", file=out)
        line("arm B (linear_transform_bsgs):", t["B"], f"  ({kb} + {kg} keys, {(kb + kg) * key_bytes / 1e9:.2f} GB)")
        line("arm B0 (MKCKKS_BSGS_FUSED=0):", t["B0"], f"  (B0 / B = {m['B0'] / m['B']:.3f} x)")
        line("arm L (linear_transform, direct):", t["L"], f"  ({kl} keys, {kl * key_bytes / 1e9:.2f} GB; L / B = {m['L'] / m['B']:.3f} x)")
        print(f"         slowest B block {max(t['B']):.4f} ms, fastest L block {min(t['L']):.4f} ms", file=out)
        if with_phases:
            ph = phases(i)
            if ph is None:
                print("         phases: no kernel trace (rocprofv3 missing or its run failed)", file=out)
            else:
                times, chunks = ph
                print(f"         kernel time per pass by phase ({chunks} chunk(s) per pass): " +
                      "; ".join(f"{k} {v:.3f} ms" for k, v in times.items()) + f"; sum {sum(times.values()):.3f} ms", file=out)
                # rows of N words k_bsgs_inner's workgroups request: the babies once (up to BABY_GROUP) or once per group of
                # giants, the present plaintext rows per ciphertext, the two sums of every giant; and every array once
                reads = (1 if n1 <= BABY_GROUP else -(-n2 // GIANT_GROUP)) * n1 * 2
                req = B * ext * (reads + n_pres + 2 * n2) * N * 8
                once = (B * ext * (n1 * 2 + 2 * n2) + ext * n_pres) * N * 8
                ti = times["inner sums (k_bsgs_inner)"]
                print(f"         k_bsgs_inner: {req / 1e9:.2f} GB requested by its workgroups ({req / ti / 1e9:.2f} TB/s), "
                      f"{once / 1e9:.2f} GB if every array is fetched once ({once / ti / 1e9:.2f} TB/s)", file=out)
        if i == REQUIRED and not max(t["B"]) < min(t["L"]):
            ok = False
            print("         REQUIREMENT MISSED: the slowest block of arm B is not below the fastest block of arm L", file=out)
        del bkeys, gkeys, pts, evks, lpts, o_b, o_b0, o_l
        torch.cuda.empty_cache()
        out.flush()
    g.close()
    g0.close()
    print(f"  {blocks} alternating blocks per arm of >= {block_s} s, HIP-event time per pass", file=out)
    print(f"  requirement ({CASES[REQUIRED][0]}: slowest B block below fastest L block): " + ("met" if ok else "MISSED"), file=out)
    out.flush()
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--block-seconds", type=float, default=0.5)
    ap.add_argument("--no-phases", action="store_true")
    ap.add_argument("--trace-case", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace_case is not None:
        trace_case(a.trace_case)
        return
    out = open(a.out, "w") if a.out else sys.stdout
    sys.exit(0 if run_ab(max(7, a.blocks), max(0.5, a.block_seconds), not a.no_phases, out) else 1)


if __name__ == "__main__":
    main()
