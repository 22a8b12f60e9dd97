"""ModUp targets converted inside the inverse column pass of their sources (k_icol_conv, switch MKCKKS_ICOL_CONV).

A digit whose sources are all fp64-class (every digit but the one that holds q_0, with 50-bit scaling) can have 1 to 3 of
its fp64-class targets converted by the workgroup that runs the inverse column pass of its sources; the conversion
kernels then skip those targets.  MKCKKS_ICOL_CONV = 0 keeps the conversion kernels for every target, 1 / 2 / 3 force
that many targets (as far as a digit has them), `auto` (anything else, the default) chooses per digit and call
(Engine: icol_conv_targets, exported as mkckks_icol_conv_targets).

One launch of k_icol_conv<LOG_H, NT> then runs the inverse column pass of every fp64-class limb, a job per digit (NT = the
largest count of the call; a digit with fewer targets, or none such as the digit that holds q_0, is a job of the same launch).

Shapes -- the smallest that reach every compiled instance (column radix 8 / 16) x (1..3 targets) and, as jobs, every
(1..4 sources) x (1..3 targets):

  tag   (depth, scaling_bits, first_bits, dnum)   (L, alpha, beta)   digits >= 1 at nl limbs: (sources, fp64-class targets)
  a4    (6, 50, 60, 2)                            (8, 4, 2)          nl 5..8: (1..4, 3)            a partial last digit below nl = 8
  a3    (7, 50, 60, 3)                            (9, 3, 3)          nl 9: (3, 5) (3, 5); nl 8: (3, 4) (2, 5); nl 7: (3, 3) (1, 5);
                                                                     nl 6: (3, 2); nl 5: (2, 2); nl 4: (1, 2)      odd and even counts

  N = 2^12 (radix 8): modup and single reencrypt (no merged flow on 64-point rows);  N = 2^14 (radix 8) and N = 2^16
  (radix 16): the merged n-client flow with its P-scaled tables, 2 clients x 2 indices, and one call at N = 2^14 large
  enough (8 clients x 16 indices) for `auto` to take the path.

Checks: every result is equal, word for word, to the oracle AND to the same call on a context created under
MKCKKS_ICOL_CONV=0.  Extreme residues (all q - 1; alternating 0 / q - 1) go through the forced three-target path.

CPU (`-m "not gpu"`): `icol_rule` restates the choice and is compared with the library's; `instances()` maps a case to the
(column radix, sources, targets) instances it launches, by the rules of Engine::modup_core, and the ledger test asserts
that the union over this module's parametrisation is every compiled instance, and that an all-integer context
(MKCKKS_NO_FP64) reaches none."""
import os

import numpy as np
import pytest

from oracle.oracle import FastCpuContext, OracleContext
from tests.test_digit_shapes import radix, split

gpu = pytest.mark.gpu

# tag: ((depth, scaling_bits, first_bits, dnum), (L, alpha, beta))
SHAPES = {"a4": ((6, 50, 60, 2), (8, 4, 2)), "a3": ((7, 50, 60, 3), (9, 3, 3))}
AUTO = "auto"
MODES = ("1", "2", "3", AUTO)
JOB_SHAPES = {(log_h, n_in, nt) for log_h in (3, 4) for n_in in (1, 2, 3, 4) for nt in (1, 2, 3)}
COMPILED = {(log_h, nt) for log_h in (3, 4) for nt in (1, 2, 3)}  # k_icol_conv<LOG_H, NT>
ICOL_CONV_MAX, ICOL_CONV_AUTO_MAX, ICOL_CONV_MIN_GRID = 3, 1, 2048  # engine.hpp

# ---- the parametrisation: the GPU tests run these lists, the ledger reads them ------------------------------------------
MODUP_CASES = [("a4", 12, nl, mode) for nl in (5, 6, 7, 8) for mode in MODES]        # modup and reencrypt, 2 items
SUM_CASES = ([("a4", 16, nl, mode, 2, 2) for nl in (5, 6, 7, 8) for mode in MODES] +
             [("a3", 14, nl, mode, 2, 2) for nl in (4, 5, 6, 7, 8, 9) for mode in MODES] +
             [("a3", 14, 9, AUTO, 8, 16)])                                            # grid 128 x 2 x 8 = 2048: auto takes one of 5 targets
EXTREME_CASES = [("a4", 16, 8, "3"), ("a3", 14, 9, "3"), ("a3", 14, 8, "2")]
NO_FP64_CASES = [("a4", 12, 8, "3"), ("a3", 14, 9, "3")]


# ---- the ledger ---------------------------------------------------------------------------------------------------------

def icol_rule(n_fp, grid, mode):
    """Engine: icol_conv_targets"""
    if mode != AUTO:
        return min(int(mode), n_fp)
    if grid < ICOL_CONV_MIN_GRID:
        return 0
    for nt in range(min(ICOL_CONV_AUTO_MAX, n_fp), 0, -1):
        if (n_fp - nt) % 2 == 0:
            return nt
    return 0


def instances(log_n, shape, nl, mode, items, fp64=True):
    """The k_icol_conv jobs with targets (column radix code, sources, targets) Engine::modup_core launches for `items` polynomials
    at nl limbs on a context whose limbs 1..L-1 are fp64-class (unless MKCKKS_NO_FP64) and whose q_0 and P are integer."""
    L, alpha, beta = shape
    col_h, row_h = radix(log_n)
    if not (fp64 and col_h >= 3 and row_h != 0 and nl >= 2) or mode == "0":
        return set()
    nparts = min(beta, -(-nl // alpha))
    digits = [(part * alpha, min(nl, (part + 1) * alpha)) for part in range(nparts)]
    # the coefficient-form digits travel as doubles only if every digit is "all fp64" or "q_0 first, then fp64" with at
    # most 4 sources (a digit that is q_0 alone is all-integer and takes packed halves)
    if any(hi - lo > 4 and not (lo == 0 and hi == 1) for lo, hi in digits):
        return set()
    eligible = [(hi - lo, (nl - 1) - (hi - lo)) for lo, hi in digits if lo >= 1 and (nl - 1) - (hi - lo) >= 1]
    r1, r2 = split(log_n)
    grid = items * len(eligible) * ((1 << r2) // (256 >> col_h))
    out = set()
    for n_in, n_fp in eligible:
        nt = icol_rule(n_fp, grid, mode)
        if nt:
            out.add((col_h, n_in, nt))
    return out


def reached():
    """(job shapes, kernel instances): a call's instance is k_icol_conv<column radix, largest target count of its jobs>"""
    jobs, kernels = set(), set()
    calls = [(tag, log_n, nl, mode, 2) for tag, log_n, nl, mode in MODUP_CASES]
    calls += [(tag, log_n, nl, mode, C * B) for tag, log_n, nl, mode, C, B in SUM_CASES]
    for tag, log_n, nl, mode, items in calls:
        got = instances(log_n, SHAPES[tag][1], nl, mode, items)
        jobs |= got
        if got:
            kernels.add((radix(log_n)[0], max(nt for _, _, nt in got)))
    return jobs, kernels


def test_rule_restatement_matches_the_library():
    from ppqsflhe_amd import binding
    f = binding.load_library().mkckks_icol_conv_targets
    for n_fp in range(0, 12):
        for grid in (0, 1, 511, 512, 2047, 2048, 2049, 4096, 1 << 33):
            for mode, code in (("0", 0), ("1", 1), ("2", 2), ("3", 3), (AUTO, -1), (AUTO, 4), (AUTO, 7)):
                assert f(n_fp, grid, code) == icol_rule(n_fp, grid, mode), (n_fp, grid, mode)
    # auto leaves the conversion kernels an even number of targets wherever it takes any
    for n_fp in range(1, 12):
        nt = icol_rule(n_fp, 1 << 20, AUTO)
        if nt:
            assert nt <= ICOL_CONV_AUTO_MAX and (n_fp - nt) % 2 == 0, (n_fp, nt)
        else:  # no count up to the shipped maximum has the parity
            assert all((n_fp - k) % 2 for k in range(1, min(ICOL_CONV_AUTO_MAX, n_fp) + 1)), n_fp


def test_ledger_reaches_every_compiled_instance():
    jobs, kernels = reached()
    assert jobs == JOB_SHAPES, (sorted(JOB_SHAPES - jobs), sorted(jobs - JOB_SHAPES))
    assert kernels == COMPILED, (sorted(COMPILED - kernels), sorted(kernels - COMPILED))
    # odd and even fp64-class target counts, a partial last digit, auto below and above its grid threshold
    assert instances(14, SHAPES["a3"][1], 9, AUTO, 4) == set()
    assert instances(14, SHAPES["a3"][1], 9, AUTO, 128) == {(3, 3, 1)}     # 5 targets -> 1, leaves 4
    assert instances(14, SHAPES["a3"][1], 8, AUTO, 128) == {(3, 2, 1)}     # 4 -> 0 (even already), 5 -> 1
    assert instances(16, SHAPES["a4"][1], 6, "3", 4) == {(4, 2, 3)}        # the last digit holds 2 of 4 limbs
    for tag, log_n, nl, mode in NO_FP64_CASES:
        assert instances(log_n, SHAPES[tag][1], nl, mode, 4, fp64=False) == set()
        assert instances(log_n, SHAPES[tag][1], nl, mode, 4) != set()


def test_shapes_are_what_the_ledger_assumes():
    from ppqsflhe_amd import Context
    for tag, log_n in {(c[0], c[1]) for c in MODUP_CASES + SUM_CASES}:
        a, (L, alpha, beta) = SHAPES[tag]
        c = Context(log_n, a[0], a[1], a[2], dnum=a[3], device=-1)
        assert (c.L, c.alpha, c.beta) == (L, alpha, beta), (tag, log_n)
        c.close()


# ---- GPU ------------------------------------------------------------------------------------------------------------------

class _Env:
    """Library switches are read once, when a context is created: set them around the constructor only."""

    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctxs():
    """Device contexts by (tag, ring, switches) and one oracle per (tag, ring), created on first use."""
    from ppqsflhe_amd import Context
    dev, ora = {}, {}

    def device(tag, log_n, mode, **env):
        if mode != AUTO:
            env = dict(env, MKCKKS_ICOL_CONV=mode)
        key = (tag, log_n, tuple(sorted(env.items())))
        if key not in dev:
            a = SHAPES[tag][0]
            with _Env(env):
                assert mode != AUTO or "MKCKKS_ICOL_CONV" not in os.environ
                dev[key] = g = Context(log_n, a[0], a[1], a[2], dnum=a[3], device=0)
            fp = 0 if "MKCKKS_NO_FP64" in env else 1
            assert [int(x == 1) for x in g.arith[:g.L]] == [0] + [fp] * (g.L - 1), (key, g.arith)
            assert not any(x == 1 for x in g.arith[g.L:]), (key, g.arith)
        return dev[key]

    def oracle(tag, log_n, fast=True):
        if (tag, log_n, fast) not in ora:
            a = SHAPES[tag][0]
            ora[tag, log_n, fast] = (FastCpuContext if fast else OracleContext)(log_n, a[0], a[1], a[2], dnum=a[3])
        return ora[tag, log_n, fast]

    device.oracle = oracle
    yield device
    for g in dev.values():
        g.close()


def rand_polys(rng, ctx, limb_ids, count):
    out = np.empty((count, len(limb_ids), ctx.N), dtype=np.uint64)
    for j, l in enumerate(limb_ids):
        out[:, j, :] = rng.integers(0, int(ctx.moduli[l]), size=(count, ctx.N), dtype=np.uint64)
    return out


def oracle_chain(o, cts, evks):
    C, B = cts.shape[:2]
    out = []
    for b in range(B):
        acc = o.reencrypt(cts[0, b], evks[0])
        for c in range(1, C):
            acc = o.eval_add(acc, o.reencrypt(cts[c, b], evks[c]))
        out.append(acc)
    return np.stack(out)


def gpu_modup(g, c1, nl):
    d = g.empty((c1.shape[0], g.num_parts(nl), nl + g.K, g.N))
    g.modup(g.to_device(c1), d, c1.shape[0], nl)
    return d.to_host()


def gpu_reencrypt(g, ct, evk, nl):
    d = g.empty(ct.shape)
    g.reencrypt(g.to_device(ct), g.to_device(evk), d, ct.shape[0], nl)
    return d.to_host()


def gpu_sum(g, cts, evks, nl):
    C, B = cts.shape[:2]
    d = g.empty((B, 2, nl, g.N))
    g.reencrypt_sum(g.to_device(cts), g.to_device(evks), d, C, B, nl)
    return d.to_host()


_cases = {}


def modup_case(ctxs, tag, log_n, nl):
    """Seeded inputs, their oracle results and the results of the MKCKKS_ICOL_CONV=0 context: once per shape, read-only."""
    key = ("modup", tag, log_n, nl)
    if key not in _cases:
        o, base = ctxs.oracle(tag, log_n, fast=False), ctxs(tag, log_n, "0")
        rng = np.random.default_rng(6100 + 31 * nl + log_n)
        c1 = rand_polys(rng, o, list(range(nl)), 2)
        c1[0, :, ::5] = (np.asarray(o.moduli[:nl], dtype=np.uint64) - np.uint64(1))[:, None]
        ct = rand_polys(rng, o, list(range(nl)) * 2, 2).reshape(2, 2, nl, o.N)
        evk = rand_polys(rng, o, list(range(o.D)) * (2 * o.beta), 1).reshape(o.beta, 2, o.D, o.N)
        want_dig = np.stack([o.modup_digits(c1[b]) for b in range(2)])
        want_ct = np.stack([o.reencrypt(ct[b], evk) for b in range(2)])
        _cases[key] = (c1, ct, evk, want_dig, want_ct, gpu_modup(base, c1, nl), gpu_reencrypt(base, ct, evk, nl))
        for a in _cases[key]:
            a.setflags(write=False)
    return _cases[key]


def sum_case(ctxs, tag, log_n, nl, C, B):
    key = ("sum", tag, log_n, nl, C, B)
    if key not in _cases:
        o, base = ctxs.oracle(tag, log_n), ctxs(tag, log_n, "0")
        rng = np.random.default_rng(6700 + 101 * nl + 17 * C + B + log_n)
        cts = rand_polys(rng, o, list(range(nl)) * 2, C * B).reshape(C, B, 2, nl, o.N)
        evks = rand_polys(rng, o, list(range(o.D)) * (2 * o.beta), C).reshape(C, o.beta, 2, o.D, o.N)
        _cases[key] = (cts, evks, oracle_chain(o, cts, evks), gpu_sum(base, cts, evks, nl))
        for a in _cases[key]:
            a.setflags(write=False)
    return _cases[key]


@gpu
@pytest.mark.parametrize("tag,log_n,nl,mode", MODUP_CASES)
def test_modup_and_reencrypt(ctxs, tag, log_n, nl, mode):
    c1, ct, evk, want_dig, want_ct, base_dig, base_ct = modup_case(ctxs, tag, log_n, nl)
    g = ctxs(tag, log_n, mode)
    dig, out = gpu_modup(g, c1, nl), gpu_reencrypt(g, ct, evk, nl)
    assert np.array_equal(base_dig, want_dig) and np.array_equal(base_ct, want_ct), "MKCKKS_ICOL_CONV=0 differs from the oracle"
    assert np.array_equal(dig, want_dig), "modup digits differ from the oracle"
    assert np.array_equal(dig, base_dig)
    assert np.array_equal(out, want_ct), "reencrypt differs from the oracle"
    assert np.array_equal(out, base_ct)


@gpu
@pytest.mark.parametrize("tag,log_n,nl,mode,C,B", SUM_CASES)
def test_merged_flow(ctxs, tag, log_n, nl, mode, C, B):
    cts, evks, want, base = sum_case(ctxs, tag, log_n, nl, C, B)
    got = gpu_sum(ctxs(tag, log_n, mode), cts, evks, nl)
    assert np.array_equal(base, want), "MKCKKS_ICOL_CONV=0 differs from the oracle chain"
    assert np.array_equal(got, want), "reencrypt_sum differs from the oracle chain"
    assert np.array_equal(got, base)


def extreme_case(o, nl, C, alternating):
    """Every residue of c0, c1 and of the eval keys q - 1, or alternating 0 / q - 1; the same for every client, so one
    oracle re-encryption serves the whole chain (tests/test_q0_walk.py)."""
    mask = (np.arange(o.N) % 2 == 0) if alternating else np.ones(o.N, dtype=bool)
    ct = np.zeros((2, nl, o.N), dtype=np.uint64)
    evk = np.zeros((o.beta, 2, o.D, o.N), dtype=np.uint64)
    for l in range(nl):
        ct[:, l, mask] = int(o.moduli[l]) - 1
    for l in range(o.D):
        evk[:, :, l, mask] = int(o.moduli[l]) - 1
    one = o.reencrypt(ct, evk)
    want = one
    for _ in range(1, C):
        want = o.eval_add(want, one)
    cts = np.ascontiguousarray(np.broadcast_to(ct, (C, 1) + ct.shape))
    evks = np.ascontiguousarray(np.broadcast_to(evk, (C,) + evk.shape))
    return cts, evks, one, want


@gpu
@pytest.mark.parametrize("alternating", [False, True])
@pytest.mark.parametrize("tag,log_n,nl,mode", EXTREME_CASES)
def test_extreme_residues(ctxs, tag, log_n, nl, mode, alternating):
    o = ctxs.oracle(tag, log_n)
    cts, evks, one, want = extreme_case(o, nl, 2, alternating)
    g, base = ctxs(tag, log_n, mode), ctxs(tag, log_n, "0")
    got = gpu_sum(g, cts, evks, nl)
    assert np.array_equal(got[0], want), "reencrypt_sum differs from the oracle"
    assert np.array_equal(got, gpu_sum(base, cts, evks, nl))
    single = gpu_reencrypt(g, cts[0], evks[0], nl)
    assert np.array_equal(single[0], one), "reencrypt differs from the oracle"
    assert np.array_equal(single, gpu_reencrypt(base, cts[0], evks[0], nl))
    dig = gpu_modup(g, cts[0, :, 1], nl)
    assert np.array_equal(dig[0], o.modup_digits(cts[0, 0, 1])), "modup digits differ from the oracle"
    assert np.array_equal(dig, gpu_modup(base, cts[0, :, 1], nl))


@gpu
@pytest.mark.parametrize("tag,log_n,nl,mode", NO_FP64_CASES)
def test_all_integer_context(ctxs, tag, log_n, nl, mode):
    """MKCKKS_NO_FP64: no digit has fp64-class sources, the switch changes nothing (the fixture asserts the classes)."""
    g, base = ctxs(tag, log_n, mode, MKCKKS_NO_FP64="1"), ctxs(tag, log_n, "0", MKCKKS_NO_FP64="1")
    if log_n == 12:
        c1, ct, evk, want_dig, want_ct, _, _ = modup_case(ctxs, tag, log_n, nl)
        for h in (g, base):
            assert np.array_equal(gpu_modup(h, c1, nl), want_dig)
            assert np.array_equal(gpu_reencrypt(h, ct, evk, nl), want_ct)
    else:
        cts, evks, want, _ = sum_case(ctxs, tag, log_n, nl, 2, 2)
        for h in (g, base):
            assert np.array_equal(gpu_sum(h, cts, evks, nl), want)
