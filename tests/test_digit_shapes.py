"""Every digit count (nparts 1..6) and every conversion fan-in (n_in 1..8) of the key switch on the fused ring sizes.

The key switch -- ModUp, the eval-key inner product, ModDown and the merged n-client `reencrypt_sum` -- ships one kernel
instance per digit count and per conversion fan-in, each for every column radix, row radix and arithmetic class.
tests/test_parameter_lattice.py creates alpha and K up to 8 and beta up to 6 at N = 2^12 only (64-point columns and rows,
no merged flow, no three-round row kernels, no 256-point columns).  This module creates them on the other rings:

  tag    (log_n, depth, scaling_bits, first_bits, dnum, aux_bits, extra_bits)   (L, K, alpha, beta)
  one8   (n, 6, 50, 60, 1, 52, 20)                                               (8, 8, 8, 1)   ModUp fan-in = nl = 1..8
  six1   (n, 4, 50, 60, 6, 60, 20)                                               (6, 1, 1, 6)   nparts = nl = 1..6, whole digits
  six2   (n, 10, 50, 60, 6, 60, 20)                                              (12, 2, 2, 6)  nl 7, 9, 11: a partial last digit
  k3..k7 (n, 2 .. 6, 50, 60, 1, 60, 20)                                          (K + 1, K, K + 1, 1)   ModDown fan-in K = 3..7

(k3 and k4 are here for the summed conversion of the merged flow: with 64-point columns no other test has K = 4, with
256-point columns none has K = 3.)  Arithmetic classes on the device (`Context.arith`; asserted by the fixture before any
test uses a context): at log_n 14, 16, 17 -- both passes on the radix kernels -- limbs 1..L-1 are fp64-class (1) and q_0 and
every P limb are integer-class; at log_n 9, 10, 13, 15 every limb is Shoup (0).  The integer class of q_0 and P on the radix
rings is pseudo-Mersenne (2) wherever P has 60-bit limbs (six1, six2, k3..k7) and Shoup (0) for one8, whose 52-bit P limbs
are not of the form 2^k - c with c <= 2^(k - 34): one limb outside that form takes the whole context to Shoup.  So one8 runs
the AR_INT instances of the fused integer kernels by default, the other tags the AR_PM ones, and MKCKKS_NO_PM changes
something only for the latter (SWITCHED).

Everything is compared word for word (np.array_equal) with the oracle: no tolerances.

CPU (`-m "not gpu"`): every context against the oracle on a host-only context, and the ledger: `arms()` maps a case (ring,
shape, nl, entry point) to the launcher arms it reaches -- (launcher, column radix, n_in) for conversions, (kernel family,
row code, nparts) for the inner-product and sum kernels -- by the split rule of Engine::Engine and fast_log_h / fast_row, and
the test asserts that the union over this module's own parametrisation lists contains every arm the suite did not reach
before.  It proves reachability by parameters only; the class assertions of the GPU fixture supply the rest.

GPU (`-m gpu`): the fan-in sweep (one8 on seven rings), the ModDown fan-in (K = 1..8 at log_n 14 and 16), the digit-count
sweep (six1, six2 at log_n 14, 16, 17: single and summed re-encryption, weighted sum, fan-out, compact fan-out) and the
same key switch under MKCKKS_NO_PM / MKCKKS_NO_FP64; and the refusal of a seventh digit, which context creation accepts.
Measured times per id, and the kernel mutations these tests were checked against: profiles/digit_shapes.txt."""
import numpy as np
import pytest

from oracle.oracle import OracleContext
from tests.test_compact_downlink import fanout_compact
from tests.test_gpu_parity import rand_ct, rand_polys
from tests.test_inner_walk import walk_length
from tests.test_parameter_lattice import _extreme_polys, _host_matches_oracle, _oracle_sum
from tests.test_reencrypt_fanout import fanout, rand_evks
from tests.test_weighted_aggregation import WEIGHTS, check_wsum, device_wsum, oracle_wsum, scaled_evk

SHOUP, FP64, PM = 0, 1, 2

# tag: ((depth, scaling_bits, first_bits, dnum, aux_bits, extra_bits), (L, K, alpha, beta))
SHAPES = {
    "one8": ((6, 50, 60, 1, 52, 20), (8, 8, 8, 1)),
    "six1": ((4, 50, 60, 6, 60, 20), (6, 1, 1, 6)),
    "six2": ((10, 50, 60, 6, 60, 20), (12, 2, 2, 6)),
    "k3": ((2, 50, 60, 1, 60, 20), (4, 3, 4, 1)),
    "k4": ((3, 50, 60, 1, 60, 20), (5, 4, 5, 1)),
    "k5": ((4, 50, 60, 1, 60, 20), (6, 5, 6, 1)),
    "k6": ((5, 50, 60, 1, 60, 20), (7, 6, 7, 1)),
    "k7": ((6, 50, 60, 1, 60, 20), (8, 7, 8, 1)),
}
# the digit count each case claims for its nl
DIGITS = {"one8": {nl: 1 for nl in range(1, 9)}, "six1": {nl: nl for nl in range(1, 7)},
          "six2": {7: 4, 8: 4, 9: 5, 10: 5, 11: 6, 12: 6}}
FP_RINGS = (14, 16, 17)  # both passes on the radix kernels: fp64-class limbs exist
W = walk_length()

# ---- the parametrisation: the GPU tests run these lists, the ledger reads them ------------------------------------------

# 1. one8: k_baseconv + generic passes; k_conv_col<2> + generic row; 64-point columns + generic row and unfused tail;
#    64-point columns + 256-point rows; k_baseconv + radix rows; 256-point columns + 256-point rows; ... + 512-point rows
FANIN_RINGS = (9, 10, 13, 14, 15, 16, 17)
FANIN_CASES = [(log_n, nl) for log_n in FANIN_RINGS for nl in range(1, 9)]
# 2. ModDown / summed-conversion fan-in K (one8 at 2^17 as well: the one-digit instance of the merged flow on 512-point rows)
MODDOWN_CASES = [(tag, log_n) for log_n in (14, 16) for tag in ("six1", "k3", "k4", "k5", "k6", "k7", "one8")] + [("one8", 17)]
# 3. digit counts 1..6 whole (six1) and 4..6 with and without a partial last digit (six2)
DIGIT_CASES = [(tag, log_n, nl) for log_n in FP_RINGS for tag, nls in (("six1", range(1, 7)), ("six2", range(7, 13)))
               for nl in nls]
GROUP_CASE = ("six2", 14, 11)                    # more clients than one group: the running sum continues from `out`
EXTREME_CASES = [("six2", 16, 12), ("six2", 16, 11)]
# 4. (tag, log_n, switch, class that must go, levels): six2 also at 9 and 8 limbs (5 and 4 digits), so that the
#    all-integer context runs k_inner_product_b<4..6>.  one8's default integer class is Shoup already: no MKCKKS_NO_PM run
SWITCHED = [("six2", 14, "MKCKKS_NO_PM", PM, (12, 11, 9, 8)), ("six2", 14, "MKCKKS_NO_FP64", FP64, (12, 11, 9, 8)),
            ("one8", 16, "MKCKKS_NO_FP64", FP64, (8, 7))]


def _args(tag, log_n):
    d = SHAPES[tag][0]
    return (log_n, d[0], d[1], d[2], d[3], d[4], d[5])


def _kwargs(a):
    return dict(first_bits=a[3], dnum=a[4], aux_bits=a[5], extra_bits=a[6])


def _all_contexts():
    keys = {("one8", log_n) for log_n in FANIN_RINGS} | set(MODDOWN_CASES) | {(t, n) for t, n, _ in DIGIT_CASES}
    keys |= {(t, n) for t, n, *_ in SWITCHED}
    return sorted(keys)


_ORACLES = {}


def oracle(tag, log_n):
    if (tag, log_n) not in _ORACLES:
        a = _args(tag, log_n)
        _ORACLES[tag, log_n] = OracleContext(a[0], a[1], a[2], **_kwargs(a))
    return _ORACLES[tag, log_n]


# ---- the ledger: which launcher arms a case reaches -------------------------------------------------------------------

def split(log_n, generic=False):
    """N = R1 x R2 (Engine::Engine): even splits of even log N land on the radix kernels"""
    r1 = (log_n // 2) & ~1 if log_n % 2 == 0 and not generic else log_n // 2
    return r1, log_n - r1


def fast_log_h(log_r, other_extent):
    if log_r not in (4, 6, 8):
        return 0
    return log_r // 2 if (256 >> (log_r // 2)) <= other_extent else 0


def fast_row(log_r2, rows):
    if log_r2 == 9 and rows >= 4:
        return 9
    return fast_log_h(log_r2, rows)


def radix(log_n, generic=False):
    """(column radix code, row code) of a ring: 0 = the generic LDS-stage pass"""
    r1, r2 = split(log_n, generic)
    return fast_log_h(r1, 1 << r2), fast_row(r2, 1 << r1)


def arms(log_n, shape, nl, entry, fp64=True):
    """The arms `entry` reaches at nl limbs on a context of `shape` whose limbs 1..L-1 are fp64-class wherever the ring
    allows it (and MKCKKS_NO_FP64 is not set: fp64) and whose q_0 and P limbs are integer-class."""
    L, K, alpha, beta = shape
    col_h, row_h = radix(log_n)
    nparts = -(-nl // alpha)
    has_fp = fp64 and col_h != 0 and row_h != 0 and nl >= 2

    def conv(n_in):  # modup_core / moddown_core: fused into the column pass where that has a radix kernel
        return ("launch_conv_col", col_h, n_in) if col_h else ("launch_baseconv", 0, n_in)

    up = {conv(min(alpha, nl - part * alpha)) for part in range(nparts)}
    down = {conv(K)}
    plain_inner = {("k_inner_product_b", row_h, nparts)}

    def single():  # keyswitch_digits + moddown_core
        if not (has_fp and row_h in (3, 4, 9)):
            return up | plain_inner | down
        out = up | down | {("k_row3_inner_fp" if row_h == 9 else "k_row_inner_fp", row_h, nparts)}
        if row_h == 3:
            return out | plain_inner
        return out | {("k_row3_inner_int", row_h, nparts), ("k_row3_inner_int+invp", row_h, nparts)}

    if entry == "modup":
        return up
    if entry == "moddown":
        return down
    if entry == "reencrypt":
        return single()
    if entry in ("sum", "wsum"):
        if not (has_fp and row_h in (4, 9) and col_h >= 3):  # qsum_ok
            return single()
        return up | {("launch_conv_col_psum", col_h, K), ("k_row3_inner_int", row_h, nparts),
                     ("k_row3_inner_int+invp", row_h, nparts), ("k_qsum3_fp" + ("+w" if entry == "wsum" else ""), row_h, nparts)}
    if entry == "fanout":
        if not (has_fp and row_h in (4, 9)):  # fanout_fused
            return up | plain_inner | down
        return up | down | {("k_fan3", row_h, nparts)}
    raise ValueError(entry)


def reached():
    """the union of arms() over what the GPU tests of this module run"""
    out = set()
    for log_n, nl in FANIN_CASES:
        for entry in ("modup", "moddown", "reencrypt"):
            out |= arms(log_n, SHAPES["one8"][1], nl, entry)
    for tag, log_n in MODDOWN_CASES:
        shape = SHAPES[tag][1]
        for nl in (shape[0], 1):
            out |= arms(log_n, shape, nl, "moddown") | arms(log_n, shape, nl, "reencrypt")
        out |= arms(log_n, shape, shape[0], "sum") | arms(log_n, shape, shape[0], "wsum")
    for tag, log_n, nl in DIGIT_CASES:
        for entry in ("modup", "reencrypt", "sum", "wsum", "fanout"):
            out |= arms(log_n, SHAPES[tag][1], nl, entry)
    for tag, log_n, nl in [GROUP_CASE] + EXTREME_CASES:
        out |= arms(log_n, SHAPES[tag][1], nl, "sum")
    for tag, log_n, switch, _, nls in SWITCHED:
        for nl in nls:
            for entry in ("reencrypt", "sum"):
                out |= arms(log_n, SHAPES[tag][1], nl, entry, fp64=switch != "MKCKKS_NO_FP64")
    return out


def required():
    """the arms no GPU test reached before this module (from reading the launch code), and the full grids"""
    req = set()
    for nparts in (4, 5, 6):  # nparts 4..6 on every N >= 2^14 path
        req |= {("k_row_inner_fp", 4, nparts), ("k_row3_inner_fp", 9, nparts), ("k_inner_product_b", 4, nparts)}
        for row in (4, 9):
            req |= {(f, row, nparts) for f in ("k_row3_inner_int", "k_row3_inner_int+invp", "k_qsum3_fp", "k_qsum3_fp+w",
                                               "k_fan3")}
    req |= {("launch_conv_col", 4, 5), ("launch_conv_col", 4, 8)}
    req |= {("launch_conv_col_psum", col, K) for col in (3, 4) for K in range(1, 9)} - {
        ("launch_conv_col_psum", 3, 2), ("launch_conv_col_psum", 3, 3), ("launch_conv_col_psum", 4, 2),
        ("launch_conv_col_psum", 4, 4)}
    req |= {("launch_baseconv", 0, n_in) for n_in in range(4, 9)}
    req |= {("launch_conv_col", 2, n_in) for n_in in range(4, 9)}
    for nparts in range(1, 7):  # the full grids of the fused kernels
        req |= {("k_row_inner_fp", 4, nparts), ("k_row3_inner_fp", 9, nparts)}
        for row in (4, 9):
            req |= {(f, row, nparts) for f in ("k_row3_inner_int", "k_row3_inner_int+invp", "k_qsum3_fp", "k_qsum3_fp+w")}
    return req


# ---- CPU --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,log_n", _all_contexts())
def test_context_on_a_host_only_context(tag, log_n):
    assert _host_matches_oracle(_args(tag, log_n)) == SHAPES[tag][1]


def test_claimed_digit_counts():
    for tag, claim in DIGITS.items():
        alpha = SHAPES[tag][1][2]
        assert {nl: -(-nl // alpha) for nl in claim} == claim, tag
    for tag, _, nl in DIGIT_CASES + [GROUP_CASE] + EXTREME_CASES:
        assert nl in DIGITS[tag]


def test_ledger_reaches_every_arm_that_was_unreached():
    missing = required() - reached()
    assert not missing, sorted(missing)


def test_ledger_follows_the_ring_split():
    assert [radix(n) for n in FANIN_RINGS] == [(0, 0), (2, 0), (3, 0), (3, 4), (0, 4), (4, 4), (4, 9)]
    assert radix(11) == (0, 3) and radix(12) == (3, 3)  # N = 2^11: generic columns, radix-8 (64-point) rows
    one8, six2 = SHAPES["one8"][1], SHAPES["six2"][1]
    assert arms(9, one8, 5, "reencrypt") == {("launch_baseconv", 0, 5), ("launch_baseconv", 0, 8), ("k_inner_product_b", 0, 1)}
    assert arms(16, one8, 5, "modup") == {("launch_conv_col", 4, 5)}
    assert arms(14, six2, 11, "modup") == {("launch_conv_col", 3, 2), ("launch_conv_col", 3, 1)}  # a partial last digit
    assert arms(14, six2, 1, "sum") == arms(14, six2, 1, "reencrypt")  # q_0 alone: no fp64-class limb, no merged flow
    assert ("k_inner_product_b", 4, 4) in arms(14, six2, 8, "reencrypt", fp64=False)
    assert ("k_qsum3_fp", 9, 6) in arms(17, six2, 12, "sum") and ("k_qsum3_fp+w", 9, 6) in arms(17, six2, 12, "wsum")


def test_arms_no_accepted_ring_produces():
    """Row radix 2 (16-point rows on the radix kernel) is never chosen, and column radix 2 only at N = 2^10, whose row pass
    is generic: so the <2> row instances and k_lift_col<2> / k_pdec_col<2> / k_switch_col<2> (which need both passes on
    the radix kernels) have no ring.  DESIGN.md, section 2."""
    for generic in (False, True):
        for log_n in range(8, 18):
            col_h, row_h = radix(log_n, generic)
            assert row_h in (0, 3, 4, 9), (log_n, generic)
            assert col_h != 2 or (log_n == 10 and row_h == 0 and not generic), (log_n, generic)


# ---- GPU --------------------------------------------------------------------------------------------------------------

def _check_classes(g, tag, log_n):
    L, K = g.L, g.K
    arith = [int(x) for x in g.arith]
    if log_n in FP_RINGS:
        assert arith[0] != FP64 and arith[1:L] == [FP64] * (L - 1) and FP64 not in arith[L:], (tag, log_n, arith)
        integer = SHOUP if tag == "one8" else PM  # the module docstring
        assert arith[0] == integer and arith[L:] == [integer] * K, (tag, log_n, arith)
    else:
        assert arith == [SHOUP] * (L + K), (tag, log_n, arith)


@pytest.fixture(scope="module")
def ctxs():
    from ppqsflhe_amd import Context
    cache = {}

    def get(tag, log_n):
        a, shape = _args(tag, log_n), SHAPES[tag][1]
        if (tag, log_n) not in cache:
            cache[tag, log_n] = Context(a[0], a[1], a[2], device=0, **_kwargs(a))
        g, o = cache[tag, log_n], oracle(tag, log_n)
        # before anything else: the case tests the region it was written for
        assert (g.L, g.K, g.alpha, g.beta) == shape, (tag, log_n)
        assert np.array_equal(g.moduli, o.moduli), (tag, log_n)
        assert len(set(g.moduli.tolist())) == g.D, (tag, log_n)
        for nl, parts in DIGITS.get(tag, {}).items():
            assert g.num_parts(nl) == parts, (tag, log_n, nl)
        _check_classes(g, tag, log_n)
        return g, o

    yield get
    for g in cache.values():
        g.close()


def _batch(log_n):
    return 2 if log_n <= 14 else 1


def _extreme_poly(g, ids, which):
    """one polynomial of _extreme_polys: every residue q - 1, or alternating 0 / q - 1 with period 1 or N / 2"""
    return _extreme_polys(g, ids)[which % 3]


def _extreme_sum_case(o, nl):
    """as test_parameter_lattice.ks_case builds it: client 0 every residue of ciphertext and key q - 1, client 1 alternating"""
    N, D = o.N, o.D
    x_cts, x_evks = np.zeros((2, 1, 2, nl, N), dtype=np.uint64), np.zeros((2, o.beta, 2, D, N), dtype=np.uint64)
    idx = np.arange(N)
    for c, m in enumerate((np.ones(N, dtype=bool), (idx // 8) % 2 == 0)):
        for l in range(nl):
            x_cts[c, :, :, l, m] = int(o.moduli[l]) - 1
        for l in range(D):
            x_evks[c, :, :, l, m] = int(o.moduli[l]) - 1
    return x_cts, x_evks, _oracle_sum(o, x_cts, x_evks, 0)[None]


def _reencrypt_both_ways(g, ct, evk, nl):
    B = ct.shape[0]
    d_ct, d_evk, d_out = g.to_device(ct), g.to_device(evk), g.empty((B, 2, nl, g.N))
    g.reencrypt(d_ct, d_evk, d_out, B, nl)
    out = d_out.to_host()
    g.reencrypt(d_ct, d_evk, d_ct, B, nl)
    return out, d_ct.to_host()


def _sum(g, cts, evks, nl):
    C, B = cts.shape[:2]
    d_out = g.empty((B, 2, nl, g.N))
    g.reencrypt_sum(g.to_device(cts), g.to_device(evks), d_out, C, B, nl)
    return d_out.to_host()


def _check_moddown(g, o, rng, nl, B, tag):
    ids = list(range(nl)) + list(range(g.L, g.D))
    x = np.concatenate([rand_polys(rng, g, ids, B), _extreme_poly(g, ids, nl)[None]])
    d_md = g.empty((B + 1, nl, g.N))
    g.moddown(g.to_device(x), d_md, B + 1, nl)
    md = d_md.to_host()
    for b in range(B + 1):
        assert np.array_equal(md[b], o.moddown(x[b])), (tag, "moddown", nl, b)


@pytest.mark.gpu
@pytest.mark.parametrize("log_n,nl", FANIN_CASES)
def test_fan_in_sweep(ctxs, log_n, nl):
    """ModUp fan-in nl (one digit of up to 8 limbs; the interchange format flips between nl = 4 and 5 where fp64-class limbs
    exist) and ModDown fan-in 8; the last polynomial of every batch is an extreme pattern."""
    g, o = ctxs("one8", log_n)
    rng = np.random.default_rng(7000 + 16 * log_n + nl)
    N, K, B = g.N, g.K, _batch(log_n)
    ids = list(range(nl))
    c1 = np.concatenate([rand_polys(rng, g, ids, B), _extreme_poly(g, ids, nl)[None]])
    d_dig = g.empty((B + 1, g.num_parts(nl), nl + K, N))
    g.modup(g.to_device(c1), d_dig, B + 1, nl)
    dig = d_dig.to_host()
    for b in range(B + 1):
        assert np.array_equal(dig[b], o.modup_digits(c1[b])), (log_n, "modup", nl, b)
    _check_moddown(g, o, rng, nl, B, log_n)
    x = _extreme_polys(g, ids)
    ct = np.concatenate([rand_ct(rng, g, nl, B), np.stack([x[nl % 3], x[(nl + 1) % 3]])[None]])
    evk = rand_evks(rng, g, 1)[0]
    out, in_place = _reencrypt_both_ways(g, ct, evk, nl)
    for b in range(B + 1):
        exp = o.reencrypt(ct[b], evk)
        assert np.array_equal(out[b], exp), (log_n, "reencrypt", nl, b)
        assert np.array_equal(in_place[b], exp), (log_n, "reencrypt in place", nl, b)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,log_n", MODDOWN_CASES)
def test_moddown_fan_in(ctxs, tag, log_n):
    """ModDown with K = 1..8 sources: the single conversion (k_conv_col2) and, in the merged n-client flow, the summed one
    (k_icol_sum + k_conv_col_psum / _psum2)."""
    g, o = ctxs(tag, log_n)
    rng = np.random.default_rng(8000 + 16 * log_n + g.K)
    L, B = g.L, _batch(log_n)
    for nl in (L, 1):
        _check_moddown(g, o, rng, nl, B, tag)
        ct, evk = rand_ct(rng, g, nl, B), rand_evks(rng, g, 1)[0]
        out, in_place = _reencrypt_both_ways(g, ct, evk, nl)
        for b in range(B):
            exp = o.reencrypt(ct[b], evk)
            assert np.array_equal(out[b], exp), (tag, log_n, "reencrypt", nl, b)
            assert np.array_equal(in_place[b], exp), (tag, log_n, "reencrypt in place", nl, b)
    cts, evks = np.stack([rand_ct(rng, g, L, 1) for _ in range(3)]), rand_evks(rng, g, 3)
    assert np.array_equal(_sum(g, cts, evks, L)[0], _oracle_sum(o, cts, evks, 0)), (tag, log_n, "reencrypt_sum")
    x_cts, x_evks, x_sum = _extreme_sum_case(o, L)
    assert np.array_equal(_sum(g, x_cts, x_evks, L), x_sum), (tag, log_n, "reencrypt_sum, extreme residues")
    check_wsum(g, o, L, 2, 1)


def _check_wsum_at_level(g, o, nl, C, B, sf_level, seed=31):
    """check_wsum with the level of the weight constants given"""
    rng = np.random.default_rng(seed)
    cts, evks = np.stack([rand_ct(rng, g, nl, B) for _ in range(C)]), rand_evks(rng, g, C)
    weights = WEIGHTS[1:C + 1]
    got, _ = device_wsum(g, cts, evks, weights, sf_level, nl)
    evks_s = [scaled_evk(o, evks[c], weights[c], sf_level) for c in range(C)]
    for b in range(B):
        assert np.array_equal(got[b], oracle_wsum(o, cts, evks_s, weights, sf_level, b)), (nl, C, B, b)


def _digit_inputs(o, log_n, nl, C=3):
    """seeded inputs of a digit-sweep case and the oracle's per-client re-encryptions [C][B] and their EvalAdd chain [B]"""
    rng = np.random.default_rng(9000 + 16 * log_n + nl)
    B = W + 1 if log_n == 14 else 2  # 2^14: a full walk of the fused integer kernel and a short last one
    cts, evks = np.stack([rand_ct(rng, o, nl, B) for _ in range(C)]), rand_evks(rng, o, C)
    per = [[o.reencrypt(cts[c, b], evks[c]) for b in range(B)] for c in range(C)]
    chain = []
    for b in range(B):
        acc = per[0][b]
        for c in range(1, C):
            acc = o.eval_add(acc, per[c][b])
        chain.append(acc)
    return cts, evks, per, np.stack(chain)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,log_n,nl", DIGIT_CASES)
def test_digit_count_sweep(ctxs, tag, log_n, nl):
    g, o = ctxs(tag, log_n)
    N, K = g.N, g.K
    cts, evks, per, chain = _digit_inputs(o, log_n, nl)
    B = cts.shape[1]
    where = (tag, log_n, nl)
    c1 = np.ascontiguousarray(cts[0, :, 1])
    d_dig = g.empty((B, g.num_parts(nl), nl + K, N))
    g.modup(g.to_device(c1), d_dig, B, nl)
    dig = d_dig.to_host()
    for b in range(B):
        assert np.array_equal(dig[b], o.modup_digits(c1[b])), (where, "modup", b)
    del d_dig, dig
    out, in_place = _reencrypt_both_ways(g, cts[0], evks[0], nl)
    for b in range(B):
        assert np.array_equal(out[b], per[0][b]), (where, "reencrypt", b)
        assert np.array_equal(in_place[b], per[0][b]), (where, "reencrypt in place", b)
    assert np.array_equal(_sum(g, cts, evks, nl), chain), (where, "reencrypt_sum")
    if nl >= 2:
        check_wsum(g, o, nl, 2, B)
    else:  # check_wsum takes its inputs for noiseScaleDeg 2 at level L - nl, whose constant a one-limb ciphertext cannot hold
        _check_wsum_at_level(g, o, nl, 2, B, 1)
    # fan-out of client 0's ciphertexts into the key domains 0 and 1, plain and compact (Rescale of the same)
    exp = [per[0], [o.reencrypt(cts[0, b], evks[1]) for b in range(B)]]
    got = fanout(g, cts[0], evks[:2], nl)
    for k in range(2):
        for b in range(B):
            assert np.array_equal(got[k, b], exp[k][b]), (where, "fanout", k, b)
    if nl >= 2:
        got = fanout_compact(g, cts[0], evks[:2], nl - 1)
        for k in range(2):
            for b in range(B):
                assert np.array_equal(got[k, b], o.rescale(exp[k][b])), (where, "fanout_compact", k, b)


@pytest.mark.gpu
def test_six_digits_across_client_groups(ctxs, monkeypatch):
    """C = 3 under MKCKKS_QSUM_GROUP=2: the second group's running sum continues from `out`, with six digits (one partial)."""
    from ppqsflhe_amd import Context
    tag, log_n, nl = GROUP_CASE
    _, o = ctxs(tag, log_n)
    cts, evks, _, chain = _digit_inputs(o, log_n, nl)
    monkeypatch.setenv("MKCKKS_QSUM_GROUP", "2")
    a = _args(tag, log_n)
    g2 = Context(a[0], a[1], a[2], device=0, **_kwargs(a))  # switches are read once, when a context is created
    try:
        assert g2.num_parts(nl) == 6
        assert np.array_equal(_sum(g2, cts, evks, nl), chain)
    finally:
        g2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [10, 14])  # k_inner_product_b's dispatch; the fused kernels'
def test_seven_digits_are_refused(log_n):
    """dnum = 7 on L = 7 limbs is accepted when the context is created; a key switch over 7 digits is refused with an
    error before its inner product is launched, and 6 digits of the same context work."""
    from ppqsflhe_amd import Context, MkckksError
    a = (log_n, 5, 50, 60, 7, 60, 20)
    g, o = Context(a[0], a[1], a[2], device=0, **_kwargs(a)), OracleContext(a[0], a[1], a[2], **_kwargs(a))
    try:
        assert (g.L, g.K, g.alpha, g.beta) == (7, 1, 1, 7) and g.num_parts(7) == 7 and g.num_parts(6) == 6
        rng = np.random.default_rng(77 + log_n)
        evk = rand_evks(rng, g, 1)[0]
        ct = rand_ct(rng, g, 7, 1)
        d_ct, d_evk, d_out = g.to_device(ct), g.to_device(evk), g.empty((1, 2, 7, g.N))
        for call in (lambda: g.reencrypt(d_ct, d_evk, d_out, 1, 7),
                     lambda: g.reencrypt_sum(d_ct, d_evk, d_out, 1, 1, 7),
                     lambda: g.reencrypt_fanout(d_ct, d_evk, d_out, 1, 1, 7)):
            with pytest.raises(MkckksError, match="more than 6 key-switch digits unsupported") as ei:
                call()
            assert ei.value.code == -1
        ct6 = rand_ct(rng, g, 6, 1)
        out, _ = _reencrypt_both_ways(g, ct6, evk, 6)
        assert np.array_equal(out[0], o.reencrypt(ct6[0], evk))
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tag,log_n,nl", EXTREME_CASES)
def test_digit_count_extreme_residues(ctxs, tag, log_n, nl):
    g, o = ctxs(tag, log_n)
    x_cts, x_evks, x_sum = _extreme_sum_case(o, nl)
    assert np.array_equal(_sum(g, x_cts, x_evks, nl), x_sum), (tag, log_n, nl)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,log_n,switch,absent,nls", SWITCHED, ids=[f"{s[0]}-{s[1]}-{s[2]}" for s in SWITCHED])
def test_key_switch_under_the_arithmetic_switches(ctxs, monkeypatch, tag, log_n, switch, absent, nls):
    """The same bits as the default context and the oracle from the other arithmetic: Shoup instead of pseudo-Mersenne
    (AR_INT instances of k_row3_inner_int), or every limb integer (no fused kernel: k_inner_product_b<nparts>)."""
    from ppqsflhe_amd import Context
    g, o = ctxs(tag, log_n)
    monkeypatch.setenv(switch, "1")
    a = _args(tag, log_n)
    g2 = Context(a[0], a[1], a[2], device=0, **_kwargs(a))
    try:
        assert absent in list(g.arith) and absent not in list(g2.arith), (tag, switch, list(g.arith), list(g2.arith))
        rng = np.random.default_rng(9900 + log_n)
        B = _batch(log_n)
        for nl in nls:
            where = (tag, log_n, switch, nl)
            ct, evk = rand_ct(rng, g, nl, B), rand_evks(rng, g, 1)[0]
            want, _ = _reencrypt_both_ways(g, ct, evk, nl)
            out, in_place = _reencrypt_both_ways(g2, ct, evk, nl)
            for b in range(B):  # the oracle first: a difference is then the switched context's own
                assert np.array_equal(out[b], o.reencrypt(ct[b], evk)), (where, "reencrypt", b)
            assert np.array_equal(out, want) and np.array_equal(in_place, want), (where, "reencrypt, default context")
            cts, evks = np.stack([rand_ct(rng, g, nl, 1) for _ in range(3)]), rand_evks(rng, g, 3)
            got = _sum(g2, cts, evks, nl)
            assert np.array_equal(got[0], _oracle_sum(o, cts, evks, 0)), (where, "reencrypt_sum")
            assert np.array_equal(got, _sum(g, cts, evks, nl)), (where, "reencrypt_sum, default context")
    finally:
        g2.close()
