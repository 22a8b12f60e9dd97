"""Polynomial and Chebyshev evaluation on every parameter region of tests/test_parameter_lattice.py's TABLE.

tests/test_poly.py and tests/test_cheb.py run on the CONFIGS shapes of tests/test_gpu_parity.py, which all have one class
layout (q_0 pseudo-Mersenne at 60 bits, fp64 scaling limbs of 40 or 50 bits, pseudo-Mersenne P limbs).  k_poly_tensor<2|4|8>,
k_cheb_tensor<SQUARE, TERM> and k_affine pick their arithmetic per limb from the limb table, so this file runs them, the two
ladders and the two evaluations once per TABLE entry: natural Shoup-class limbs of 51 .. 60 bits (B = 8 sends their
inner sum through reduce_wide, the Chebyshev d1 reduces twice for them), the all-integer rings, a 52-bit pseudo-Mersenne
q_0, an fp64 q_0, fp64 limbs of 21, 24 and 30 bits, fp64-class P limbs under the compositions, L = 32.

Built as tests/test_lattice_evaluation.py is: one test function per section, parametrised over every name of TABLE
(`test_every_section_covers_every_table_entry` checks that, without a device); the `ctxs` fixture is test_parameter_lattice's
and asserts the entry's arithmetic classes first; every comparison is np.array_equal against Python-integer or oracle
references -- the helpers of the feature test files, unchanged -- and there is no tolerance in this file.  Inputs and expected
results are built once per (section, entry) by the `*_case` functions, which need the oracle only, kept read-only by `cached`
and shared with the runs under the library switches (a fresh context per switch).  Outputs sit between POISON guard words and
inputs are read back unchanged.

The three kernels are pointwise, so their operands are COLUMNS = 512 distinct columns repeated along the ring: every device
word is compared and the Python-integer reference stays small at N = 2^17.  Limb layouts: nl = L with every operand at L
limbs, and (except on the three rings of 2^16 and 2^17) nl = L - 1 with the operands alternately at L and L - 1 limbs, read
in place at their own limb counts.  Plans (B, G) = (2, 2), (4, 3), (8, 8), weights from test_poly.tensor_weights with the cap
of the entry's own moduli; the four Chebyshev instances under test_cheb.step_weights.

Two input patterns beyond the `with_edges` columns, each with a CPU self-check that needs no device
(`test_the_extreme_patterns_are_what_they_claim`):
  * `integer_maximum`: every operand word q - 1 under constants that are all = q - 1 (mod q) on every limb: the largest value
    of the integer classes' 128-bit sums of whole products.
  * `poly_half_moduli` / `cheb_half_moduli`: every product of one lazy fp64 sum has its centred remainder within 2^8 of +q/2
    (a second column group: of -q/2), the pattern tests/test_lattice_evaluation.py's `with_half_moduli` introduced.

An evaluation whose weights do not fit half the modulus of their level is refused by the library before anything runs; which
(entry, degree, interval) that is, is predicted here from the Python restatements of the weights (`*_refusal`) and asserted,
message included, on a host-only context (`test_the_predicted_refusals_are_the_librarys`) and on the device.  The next lower
degree that fits runs instead; every entry evaluates at least degree 2 in both bases.

Ladders and evaluations run at nl = L with the scale of a fresh ciphertext on L limbs, sf_big(0) (sf(0) is the scale of the
20-bit extra limb, about 2^19: a ladder started there has scales below 1 after two steps).  What the library then refuses, on
this table: the unmapped Chebyshev series at degree 7 on s55n14, s30 and r8, 31 on d1 and 63 on al5 and al8k8 -- a ladder
step's constant carries S_i S_j, which outgrows the lower levels of a ladder that starts on the extra limb -- where degrees 3,
3, 3, 7 and 15 run instead; the same degrees pass as polynomials and on the mapped interval, which restarts from its level's
standard scale.  The 21- and 24-bit scaling limbs (s21n16, s24n17, f40) refuse nothing at the degree 3 their four limbs allow.

Teeth ("Teeth of the class bounds"): inner<8> through barrett_reduce128, and the Chebyshev integer d1 reduced once,
each fail their section on the eight entries with a natural 60-bit Shoup q_0.  Two cadences have slack these inputs cannot
take away.  POLY_FP_INNER = POLY_FP_GIANTS = 8 (no fold) passes everywhere: the widest fp64 limb generate() produces is just
above 2^50, so 2^53 = 8 q; q + 7 * 0.97 q = 7.79 q for the inner sum, and true remainders reach q/2, not the 0.75 q of the
bound, so d1 holds 0.51 q + 14 * 0.5 q = 7.51 q.  A plain fold in place of PolyWord<TENSOR_PM>::inner's pm_reduce128 (Q' below
1.25 * 2^k) leaves d1 below 2^(2k+5), inside the closing pm_reduce128's 2^(2k+6).

Wall time on an MI355X: the GPU tests of the file (199) 15 s; slowest test 0.62 s
(test_poly_tensor_is_the_integer_definition[d30]); the 49 device-free tests take 6 s on a CPU.
"""
import types
from fractions import Fraction

import numpy as np
import pytest

from tests.test_cheb import INSTANCES, cpu_cheb_eval, cpu_cheb_ladder, dev_cheb_tensor, ladder_weight, map_weights
from tests.test_cheb import dev_eval_by_hand as cheb_eval_by_hand
from tests.test_cheb import dev_ladder_by_hand as cheb_ladder_by_hand
from tests.test_cheb import py_affine, py_cheb_tensor, py_int, step_weights
from tests.test_cheb_surface import py_cheb_weights
from tests.test_gpu_parity import rand_ct
from tests.test_lattice_evaluation import _freeze, cached  # noqa: F401  (_freeze: cached's)
from tests.test_parameter_lattice import FP64, NAMES, PM, TABLE, _batch, _kwargs, ctxs, oracle  # noqa: F401  (ctxs: fixture)
from tests.test_poly import cpu_ladder, cpu_poly_eval, dev_poly_tensor, py_poly_tensor, split_powers, tensor_weights
from tests.test_poly import dev_eval_by_hand as poly_eval_by_hand
from tests.test_poly import dev_ladder_by_hand as power_ladder_by_hand
from tests.test_poly_surface import py_constants, py_ladder, py_plan, py_weights
from tests.test_product import POISON, oracle_relinearize, with_edges  # noqa: F401  (oracle_relinearize: the CPU chains')
from tests.test_rotation import rand_evks

gpu = pytest.mark.gpu

BIG = ("s56n16", "s21n16", "s24n17")  # N = 2^16 and 2^17: nl = L only
COLUMNS = 512
PLANS = ((2, 2), (4, 3), (8, 8))
CPU_CHAIN_N = 1 << 13  # the CPU chains run up to this ring
NEAR = 1 << 8          # the half-modulus patterns sit within this of +-q/2
# columns of the 512: 0 .. 3 with_edges; then the patterns
MAX0, MAX_COLS = 4, 16                 # integer_maximum of the Chebyshev operands
INNER0, GROUP = 4, 16                  # poly: one group per giant index j, 8 columns next to +q/2 and 8 next to -q/2
OUTER0 = INNER0 + 8 * GROUP            # poly: the outer sum's group
CHEB0 = MAX0 + MAX_COLS                # cheb: per weight 16 columns for the general instances, 16 for the square ones
MAX_W = 32                             # poly: the integer maximum runs under its own weights, on 32 columns of its own
DEGREES_63 = ("al8k8", "al5")
FORKS = [(n, "MKCKKS_POLY_FUSED", "0", None) for n in ("a45", "s59", "r13")] + \
        [(n, "MKCKKS_CHEB_FUSED", "0", None) for n in ("a45", "s59", "r13")] + \
        [(n, "MKCKKS_NO_FP64", "1", FP64) for n in ("d30", "al8k8", "s30")] + \
        [(n, "MKCKKS_NO_PM", "1", PM) for n in ("f52", "a55")]


def layouts(name):
    """(nl, limbs of the operands above nl, in turn)"""
    L = TABLE[name][1][0]
    return ((L, (0,)),) if name in BIG else ((L, (0,)), (L - 1, (1, 0)))


def narrow_ctx(o):
    return types.SimpleNamespace(N=min(o.N, COLUMNS), moduli=o.moduli)


def double_prefix(moduli, nl):
    """The longest prefix of the level whose modulus is a finite double: all nl limbs, except on d30 (L = 32, 1600 bits).  The
    weight helpers take their cap from it: a weight below a quarter of a prefix's modulus fits the level too."""
    bits = 0
    for k in range(nl):
        bits += int(moduli[k]).bit_length()
        if bits > 1020:
            return k
    return nl


def wide(x, N):
    return np.tile(x, N // x.shape[-1])


def same(got, want, *tag):
    assert np.array_equal(got, want), tag


def centred(r, q):
    return r - q if r > q // 2 else r


def near_half(rng, q, shape):
    """Residues within NEAR of +q/2 in the first half of the last axis, of -q/2 in the second; as Python integers."""
    h = (q - 1) // 2
    d = rng.integers(0, NEAR, size=shape)
    half = shape[-1] // 2
    out = np.empty(shape, dtype=object)
    out[..., :half] = h - d[..., :half].astype(object)
    out[..., half:] = h + 1 + d[..., half:].astype(object)
    return out


def is_near(r, q, col):
    """col < GROUP / 2: 0 < centred r, within NEAR of q/2; else the same below zero"""
    c = centred(int(r), q)
    return q // 2 - NEAR <= c <= q // 2 + 1 if col < GROUP // 2 else -(q // 2) - 1 <= c <= -(q // 2) + NEAR


# ---- the two extreme input patterns ------------------------------------------------------------------------------------

def integer_maximum(moduli, nl, operands, cols, constants):
    """Every word of `operands` (u64[..][2][nl_x][W]) in the columns `cols` becomes q_l - 1, and `constants` (Python integers,
    the M of the call) are asserted = q_l - 1 on every limb: all weights -1.0 for poly_tensor, +1.0 for cheb_tensor (whose
    table holds M' = q - M).  Targets the integer bounds of the kernel headers, which are attained by no other input:
    poly_kernels.hpp "B = 8 gives at most 7 q^2 + q" ((q - 1) + 7 (q - 1)^2 in PolyWord<TENSOR_INT>::inner<8>, through
    reduce_wide because it leaves barrett_reduce128's window 2^(k+62) on a 60-bit limb) and "d1 holds at most 2 * 7 products
    and the residue Q'_0" (pseudo-Mersenne); cheb_kernels.hpp "d1 is at most 4 q^2 + q^2" (pseudo-Mersenne) and "d1 with a
    term would be 5 q^2 ... REDUCED TWICE" (Shoup/Barrett)."""
    for l in range(nl):
        q = int(moduli[l])
        assert all(int(m) % q == q - 1 for m in constants), ("constants are not q - 1", l)
    for x in operands:
        for l in range(x.shape[-2]):
            x[..., l, cols] = np.uint64(int(moduli[l]) - 1)


def poly_half_moduli(rng, moduli, nl_T, babies, giants, M):
    """The longest same-sign runs of k_poly_tensor's lazy fp64 sums (poly_kernels.hpp: "at most q + 4 * 0.97 q = 4.88 q before
    the first reduction", "within 0.51 q + 3 * 1.5 q = 5.01 q"): with POLY_FP_INNER or POLY_FP_GIANTS raised, these columns
    are where a sum leaves 2^53 first on a 50-bit limb.
    (a) inner sum, one group of GROUP columns per giant index j (the babies are shared by all rows): both components of every
        baby are (h -+ d) M_{j,i}^-1 mod q, so every product M_{j,i} b_i of Q'_j has its centred remainder next to +q/2 (first
        half of the group) or -q/2 (second half).  A constant = 0 mod q contributes 0 whatever its baby: that baby stays random.
    (b) outer sum, GROUP columns: g_{j,1} = (h -+ d) Q'_{j,0}^-1 and g_{j,0} = (h -+ d) Q'_{j,1}^-1 from the exactly computed
        Q'_j of the column's (random) babies: all 2 (G - 1) products of d1 have one sign.  A column with a Q' = 0 mod q has its
        babies redrawn on that limb.
    Asserts the remainders on the exact products, and that no more than 1 in 16 of the pattern columns needed a redraw."""
    G, B = len(M), len(M[0])
    assert OUTER0 + GROUP <= babies[0].shape[-1] and G <= 8
    redrawn = set()
    for t in range(nl_T):
        q = int(moduli[t])
        m = [[v % q for v in row] for row in M]
        for j in range(G):  # (a)
            assert any(m[j][i] for i in range(1, B)), ("a row of dead constants", j, t)
            c0 = INNER0 + j * GROUP
            near = near_half(rng, q, (B - 1, 2, GROUP))
            for i in range(1, B):
                if m[j][i]:
                    inv = pow(m[j][i], -1, q)
                    babies[i - 1][0, :, t, c0:c0 + GROUP] = np.array(near[i - 1] * inv % q, dtype=np.uint64)
            for i in range(1, B):
                for c in range(2):
                    for k in range(GROUP):
                        r = m[j][i] * int(babies[i - 1][0, c, t, c0 + k]) % q
                        assert not m[j][i] or is_near(r, q, k), ("inner", j, i, c, t, k)

        def q_prime(col):
            return [[(m[j][0] * (1 - c) + sum(m[j][i] * int(babies[i - 1][0, c, t, col]) for i in range(1, B))) % q
                     for c in range(2)] for j in range(G)]

        for k in range(GROUP):  # (b)
            col = OUTER0 + k
            qp = q_prime(col)
            for _ in range(8):
                if all(qp[j][0] and qp[j][1] for j in range(1, G)):
                    break
                redrawn.add(k)
                for x in babies:
                    x[0, :, t, col] = rng.integers(0, q, size=2, dtype=np.uint64)
                qp = q_prime(col)
            assert all(qp[j][0] and qp[j][1] for j in range(1, G)), ("no invertible Q'", t, k)
            near = near_half(rng, q, (G, 2, GROUP))[:, :, k]
            for j in range(1, G):
                giants[j - 1][0, 1, t, col] = int(near[j, 0]) * pow(qp[j][0], -1, q) % q
                giants[j - 1][0, 0, t, col] = int(near[j, 1]) * pow(qp[j][1], -1, q) % q
                assert is_near(qp[j][0] * int(giants[j - 1][0, 1, t, col]) % q, q, k), ("outer", j, t, k)
                assert is_near(qp[j][1] * int(giants[j - 1][0, 0, t, col]) % q, q, k), ("outer", j, t, k)
    assert 16 * len(redrawn) <= GROUP, ("redraws", sorted(redrawn))
    return len(redrawn)


def cheb_half_moduli(rng, moduli, nl, a, b, t, weights):
    """(c) The largest same-sign d1 of k_cheb_tensor's fp64 class (cheb_kernels.hpp: "d1 = 2 (p + p) + p': 4 * 0.97 q + 0.97 q
    = 4.85 q", one reduction per output).  Per weight 2 * GROUP columns.  The first GROUP, for the general instances:
    a0 = a1 = 1, b0, b1 and M' t0, M' t1 all next to +q/2 (second half: -q/2), with t = (h -+ d) M'^-1 mod q.  The second
    GROUP, for the square instances: a0 = 1, a1 next to +-q/2 (d1 = 4 a0 a1), t as before.  A weight with M' = 0 mod q (the
    one below 0.5) has no term to place: its t stays random.  Asserts the remainders; nothing is ever redrawn here."""
    assert CHEB0 + 2 * GROUP * len(weights) <= a.shape[-1]
    for wi, w in enumerate(weights):
        c0 = CHEB0 + 2 * GROUP * wi
        gen, sq = slice(c0, c0 + GROUP), slice(c0 + GROUP, c0 + 2 * GROUP)
        for l in range(nl):
            q = int(moduli[l])
            mp = (q - py_int(w) % q) % q
            near = near_half(rng, q, (6, GROUP))
            a[0, :, l, gen] = 1
            b[0, 0, l, gen], b[0, 1, l, gen] = (np.array(near[k], dtype=np.uint64) for k in (0, 1))
            a[0, 0, l, sq], a[0, 1, l, sq] = 1, np.array(near[2], dtype=np.uint64)
            if mp:
                inv = pow(mp, -1, q)
                t[0, 0, l, gen], t[0, 1, l, gen] = (np.array(near[k] * inv % q, dtype=np.uint64) for k in (3, 4))
                t[0, 1, l, sq] = np.array(near[5] * inv % q, dtype=np.uint64)
            for k in range(GROUP):
                rem = [int(b[0, 0, l, c0 + k]), int(b[0, 1, l, c0 + k]), int(a[0, 1, l, c0 + GROUP + k])]
                if mp:
                    rem += [mp * int(t[0, c, l, c0 + k]) % q for c in range(2)] + [mp * int(t[0, 1, l, c0 + GROUP + k]) % q]
                assert all(is_near(r, q, k) for r in rem), ("cheb", wi, l, k)


# ---- 1: poly_tensor ---------------------------------------------------------------------------------------------------

def operand_limbs(nl_T, extra, B, G):
    return ([nl_T + extra[(i - 1) % len(extra)] for i in range(1, B)], [nl_T + extra[j % len(extra)] for j in range(1, G)])


def poly_tensor_inputs(name):
    """Per (plan, layout): COLUMNS-wide operands with the `with_edges` columns and the half-modulus runs under
    tensor_weights' random weights ("random"), and MAX_W-wide operands whose first half is the integer maximum under weights
    that are all -1.0 ("maximum").  No reference yet: this is what the device-free self-check builds."""
    o = oracle(name)
    p_bits = TABLE[name][0][2]
    case = {}
    for li, (nl_T, extra) in enumerate(layouts(name)):
        for B, G in PLANS:
            rng = np.random.default_rng(3100 + 97 * nl_T + 7 * B + G)
            baby_nl, giant_nl = operand_limbs(nl_T, extra, B, G)
            nar = narrow_ctx(o)
            babies = [with_edges(rand_ct(rng, nar, nl, 1), o.moduli) for nl in baby_nl]
            giants = [with_edges(rand_ct(rng, nar, nl, 1), o.moduli) for nl in giant_nl]
            w = tensor_weights(rng, o.moduli, double_prefix(o.moduli, nl_T), B, G, p_bits, li if (B, G) == (2, 2) else 0)
            M = py_constants(w)
            redrawn = poly_half_moduli(rng, o.moduli, nl_T, babies, giants, M)
            case["random", nl_T, B] = dict(babies=babies, baby_nl=baby_nl, giants=giants, giant_nl=giant_nl, w=w, M=M, G=G,
                                           redrawn=redrawn)
            nar = types.SimpleNamespace(N=MAX_W, moduli=o.moduli)
            babies = [rand_ct(rng, nar, nl, 1) for nl in baby_nl]
            giants = [rand_ct(rng, nar, nl, 1) for nl in giant_nl]
            w = np.full((G, B), -1.0)
            M = py_constants(w)
            integer_maximum(o.moduli, nl_T, babies + giants, slice(0, MAX_W // 2), [v for row in M for v in row])
            for t in range(nl_T):  # the inner sum of the header's bound, in whole integers
                q = int(o.moduli[t])
                inner = M[1][0] % q + sum((M[1][i] % q) * int(babies[i - 1][0, 0, t, 0]) for i in range(1, B))
                assert inner == (q - 1) + (B - 1) * (q - 1) ** 2, (name, B, t)
            case["maximum", nl_T, B] = dict(babies=babies, baby_nl=baby_nl, giants=giants, giant_nl=giant_nl, w=w, M=M, G=G)
    return case


def poly_tensor_case(name):
    o = oracle(name)
    case = {}
    for key, c in cached(poly_tensor_inputs, name).items():
        want = py_poly_tensor(o.moduli, [x[0] for x in c["babies"]], [y[0] for y in c["giants"]], c["M"], key[1])
        assert want[2].any()
        case[key] = dict(c, want=want)
    return case


def run_poly_tensor(g, o, name, tag):
    case = cached(poly_tensor_case, name)
    for (kind, nl_T, B), c in case.items():
        dev = ([wide(x, g.N) for x in c["babies"]], c["baby_nl"], [wide(y, g.N) for y in c["giants"]], c["giant_nl"], c["w"], None)
        got = dev_poly_tensor(g, dev, 1, nl_T)  # POISON around the output, inputs read back unchanged
        same(got[0], wide(c["want"], g.N), name, tag, "poly_tensor", kind, nl_T, B, c["G"])


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_poly_tensor_is_the_integer_definition(ctxs, name):
    g, o = ctxs(name)
    run_poly_tensor(g, o, name, "default")


# ---- 2: cheb_tensor ---------------------------------------------------------------------------------------------------

def cheb_weights_of(o, name, nl):
    """step_weights' four kinds (negative, large, a tie, M = 0) and +1.0: M' = q - 1, the constant of the integer maximum"""
    return step_weights(o.moduli, nl, TABLE[name][0][2]) + [1.0]


def cheb_tensor_inputs(name):
    o = oracle(name)
    case = {}
    for nl, extra in layouts(name):
        rng = np.random.default_rng(3200 + 97 * nl)
        nl_a, nl_b, nl_t = nl + extra[0], nl + extra[-1], nl + extra[0]
        nar = narrow_ctx(o)
        a, b, t = (with_edges(rand_ct(rng, nar, x, 1), o.moduli) for x in (nl_a, nl_b, nl_t))
        weights = cheb_weights_of(o, name, nl)
        assert [py_int(w) for w in weights[2:]] == [12346, 0, 1] and weights[0] < 0 < weights[1]
        integer_maximum(o.moduli, nl, [a, b, t], slice(MAX0, MAX0 + MAX_COLS), [-py_int(weights[4])])  # M' = -M
        cheb_half_moduli(rng, o.moduli, nl, a, b, t, weights)
        case[nl] = dict(a=a, nl_a=nl_a, b=b, nl_b=nl_b, t=t, nl_t=nl_t, weights=weights)
    return case


def cheb_tensor_case(name):
    o = oracle(name)
    case = {}
    for nl, c in cached(cheb_tensor_inputs, name).items():
        want = {}
        for inst, (square, term) in enumerate(INSTANCES):
            for wi, w in enumerate(c["weights"]):
                want[inst, wi] = py_cheb_tensor(o.moduli, c["a"][0], (c["a"] if square else c["b"])[0], c["t"][0] if term else None,
                                                py_int(w), nl)
        case[nl] = dict(c, want=want)
    return case


def run_cheb_tensor(g, o, name, tag):
    for nl, c in cached(cheb_tensor_case, name).items():
        a, b, t = (wide(c[k], g.N) for k in ("a", "b", "t"))
        dev = (a, c["nl_a"], b, c["nl_b"], t, c["nl_t"], c["weights"], None)
        bufs = tuple(g.to_device(x) for x in (a, b, t))
        for (inst, wi), want in c["want"].items():
            got = dev_cheb_tensor(g, dev, inst, wi, 1, nl, bufs)  # POISON around the output, inputs read back unchanged
            same(got[0], wide(want, g.N), name, tag, "cheb_tensor", nl, INSTANCES[inst], c["weights"][wi])


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_cheb_tensor_is_the_integer_definition_in_all_four_instances(ctxs, name):
    g, o = ctxs(name)
    run_cheb_tensor(g, o, name, "default")


# ---- 3: affine --------------------------------------------------------------------------------------------------------

def affine_case(name):
    """nl in {L, 1}, two ciphertexts; weights: negative, zero, a tie, M = 0, and 0.99 of 2^(sum of (bit length - 1)) / 2, which
    is below half the level's modulus whatever the primes are."""
    o = oracle(name)
    p = TABLE[name][0][2]
    rng = np.random.default_rng(3300)
    case = {}
    for nl in (o.L, 1):
        cap = sum(int(m).bit_length() - 1 for m in o.moduli[:double_prefix(o.moduli, nl)]) - 1
        top = 0.99 * 2.0 ** cap
        pairs = [(-0.7 * 2.0 ** min(p, cap - 1), 0.625 * 2.0 ** min(2 * p, cap - 1)), (-12345.5, 0.3), (0.0, -3.0), (top, -top),
                 (1.0, top)]
        ct = with_edges(rand_ct(rng, narrow_ctx(o), nl, 2), o.moduli)
        want = [np.stack([py_affine(o.moduli, ct[c], py_int(wm), py_int(wa)) for c in range(2)]) for wm, wa in pairs]
        case[nl] = dict(ct=ct, pairs=pairs, want=want)
    return case


def guarded(g, shape):
    words = int(np.prod(shape))
    d_big = g.to_device(np.full(words + 4 * g.N, POISON, dtype=np.uint64))
    return d_big, d_big.view(2 * g.N, tuple(shape)), words


def guards_intact(g, d_big, words):
    big = d_big.to_host()
    return bool(np.all(big[:2 * g.N] == POISON) and np.all(big[2 * g.N + words:] == POISON))


def run_affine(g, o, name, tag):
    for nl, c in cached(affine_case, name).items():
        ct = wide(c["ct"], g.N)
        for (w_mul, w_add), want in zip(c["pairs"], c["want"]):
            d_in = g.to_device(ct)
            d_big, d_out, words = guarded(g, ct.shape)
            g.affine(d_in, d_out, 2, nl, w_mul, w_add)
            assert guards_intact(g, d_big, words), (name, tag, "affine wrote outside its output", nl)
            same(d_in.to_host(), ct, name, tag, "affine changed its input", nl)
            same(d_out.to_host(), wide(want, g.N), name, tag, "affine", nl, w_mul, w_add)
            g.affine(d_in, d_in, 2, nl, w_mul, w_add)
            same(d_in.to_host(), wide(want, g.N), name, tag, "affine in place", nl, w_mul, w_add)


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_affine_in_place_and_out_of_place(ctxs, name):
    g, o = ctxs(name)
    run_affine(g, o, name, "default")


# ---- the weights' fit, predicted from the Python restatements ------------------------------------------------------------

REFUSAL = "does not fit half the modulus of its level"


def fits(moduli, w, nl):
    half = Fraction(1, 2)
    for m in moduli[:nl]:
        half *= int(m)
    return Fraction(abs(float(w))) < half


def ladder_fits(moduli, nl, n, scale):
    """every step weight S_i S_j / S_{i-j} of a Chebyshev ladder below half the modulus of the step's level"""
    nls, sc = py_ladder(moduli, nl, n, scale)
    return all(fits(moduli, ladder_weight(sc, (k + 1) // 2, k - (k + 1) // 2), nls[(k + 1) // 2 - 1]) for k in range(2, n + 1))


def poly_refusal(o, coef, nl, scale):
    """None, or the text with which poly_eval refuses: too few limbs first, then a weight that does not fit."""
    p = py_plan(len(coef) - 1, nl)
    if p["nl_out"] < 1:
        return f"needs {p['depth'] + 1} limbs"
    w, _ = py_weights(o.moduli, o.L, o.sf, coef, nl, scale)
    return None if all(fits(o.moduli, v, p["nl_T"]) for v in w.reshape(-1)) else REFUSAL


def cheb_refusal(o, coef, a, b, nl, scale):
    if (a, b) != (-1.0, 1.0) and nl < 2:
        return "needs 2 limbs"
    w_mul, w_add, nl_u, s_u = map_weights(o.moduli, o.L, o.sf, nl, a, b, scale)
    p = py_plan(len(coef) - 1, nl_u)
    if p["nl_out"] < 1:
        return f"needs {p['depth'] + 1} limbs"
    if w_mul is not None and not (fits(o.moduli, w_mul, nl) and fits(o.moduli, w_add, nl)):
        return REFUSAL
    w, _ = py_cheb_weights(o.moduli, o.L, o.sf, coef, nl_u, s_u)
    if not all(fits(o.moduli, v, p["nl_T"]) for v in w.reshape(-1)):
        return REFUSAL
    nlx, sx = py_ladder(o.moduli, nl_u, p["B"], s_u)
    ok = ladder_fits(o.moduli, nl_u, p["B"], s_u) and ladder_fits(o.moduli, nlx[-1], p["G"] - 1, sx[-1])
    return None if ok else REFUSAL


def eval_coef(degree):
    coef = np.random.default_rng(3500 + degree).uniform(-1, 1, size=degree + 1)
    coef[1] = 0.0
    return coef


KINDS = {"poly": None, "cheb": (-1.0, 1.0), "mapped": (0.25, 4.0)}


def refusal_of(o, kind, degree, nl, scale):
    coef = eval_coef(degree)
    return poly_refusal(o, coef, nl, scale) if kind == "poly" else cheb_refusal(o, coef, *KINDS[kind], nl, scale)


def eval_plan(name):
    """[(kind, degree, refusal text or None)] at nl = L: degree 3 everywhere, 7 wherever L >= 5, 63 (B = G = 8) on al8k8 and
    al5, 31 on d1; the three kinds each.  A refusal for want of a level (the mapped interval spends one) stands as it is; a
    refused weight is followed by the largest lower degree that fits."""
    o = oracle(name)
    L, scale = o.L, o.sf_big(0)
    degrees = [3] + ([7] if L >= 5 else []) + ([63] if name in DEGREES_63 else []) + ([31] if name == "d1" else [])
    plan = []
    for kind in KINDS:
        for degree in degrees:
            why = refusal_of(o, kind, degree, L, scale)
            plan.append((kind, degree, why))
            if why == REFUSAL:
                lower = [d for d in range(degree - 1, 1, -1) if refusal_of(o, kind, d, L, scale) is None]
                if lower and (kind, lower[0], None) not in plan:
                    plan.append((kind, lower[0], None))
    return plan


# ---- 4: ladders ---------------------------------------------------------------------------------------------------------

def ladder_case(name):
    """powers and cheb_ladder at n = 3, nl = L; the CPU chains up to N = 2^13.  The relinearisation key is random words."""
    o = oracle(name)
    rng = np.random.default_rng(3400)
    L, n_ct = o.L, _batch(o)
    z = with_edges(rand_ct(rng, o, L, n_ct), o.moduli)
    rlk = rand_evks(rng, o, 1)[0]
    scale = o.sf_big(0)  # the scale of a fresh ciphertext on L limbs; sf(0) is that of the 20-bit extra limb
    assert ladder_fits(o.moduli, L, 3, scale), name
    nls, scales = py_ladder(o.moduli, L, 3, scale)
    assert nls == [L, L - 1, L - 2]
    case = dict(z=z, rlk=rlk, scale=scale, nls=nls, scales=scales)
    if o.N <= CPU_CHAIN_N:
        case["powers"] = cpu_ladder(o, z[0], rlk, 3)
        case["cheb"], cpu_s = cpu_cheb_ladder(o, z[0], rlk, 3, scale)
        assert cpu_s == scales
    return case


def run_ladders(g, o, name, tag):
    c = cached(ladder_case, name)
    N, L, n_ct = g.N, g.L, c["z"].shape[0]
    assert g.sf_big(0) == c["scale"]
    d_z, d_rlk = g.to_device(c["z"]), g.to_device(c["rlk"])
    hand = {"powers": power_ladder_by_hand(g, c["z"], d_rlk, n_ct, L, 3),
            "cheb": [x.to_host() for x in cheb_ladder_by_hand(g, c["z"], d_rlk, n_ct, L, 3, c["scale"])[0]]}
    for what, call in (("powers", g.powers), ("cheb", g.cheb_ladder)):
        d_big, d_out, words = guarded(g, (n_ct * 2 * N * sum(c["nls"]),))
        nls, scales = call(d_z, d_rlk, d_out, n_ct, L, 3, c["scale"])
        assert nls == c["nls"] and scales == c["scales"], (name, tag, what, nls, scales)
        assert guards_intact(g, d_big, words), (name, tag, what, "wrote outside its output")
        same(d_z.to_host(), c["z"], name, tag, what, "changed its input")
        got = split_powers(d_out.to_host(), nls, n_ct, N)
        for k in range(3):
            same(got[k], hand[what][k], name, tag, what, k + 1, "by hand")
            if what in c:
                same(got[k][0], c[what][k], name, tag, what, k + 1, "CPU chain")


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_ladders_are_their_loops(ctxs, name):
    g, o = ctxs(name)
    run_ladders(g, o, name, "default")


# ---- 5: poly_eval and cheb_eval -------------------------------------------------------------------------------------------

def eval_input(name):
    o = oracle(name)
    return dict(ct=rand_ct(np.random.default_rng(3600), o, o.L, _batch(o)), plan=eval_plan(name))


def eval_case_of(kind):
    """The CPU chains of one kind (up to N = 2^13), as a builder `cached` keeps under its own name."""
    def build(name):
        o = oracle(name)
        lad, ct = cached(ladder_case, name), cached(eval_input, name)["ct"]
        case = {}
        if o.N <= CPU_CHAIN_N:
            for k, degree, why in cached(eval_input, name)["plan"]:
                if k == kind and why is None and kind == "poly":
                    case[kind, degree] = cpu_poly_eval(o, ct[0], lad["rlk"], eval_coef(degree), lad["scale"])
                elif k == kind and why is None:
                    case[kind, degree] = cpu_cheb_eval(o, ct[0], lad["rlk"], eval_coef(degree), *KINDS[kind], lad["scale"])
        return case
    build.__name__ = "eval_case_" + kind
    return build


EVAL_CASES = {kind: eval_case_of(kind) for kind in KINDS}


def refused(call, text):
    from ppqsflhe_amd.binding import MkckksError
    with pytest.raises(MkckksError) as e:
        call()
    assert e.value.code == -1 and text in str(e.value), (text, str(e.value))


def dev_eval(g, kind, d_ct, d_rlk, coef, d_out, n_ct, nl, scale):
    if kind == "poly":
        return g.poly_eval(d_ct, d_rlk, coef, d_out, n_ct, nl, scale)
    return g.cheb_eval(d_ct, d_rlk, coef, *KINDS[kind], d_out, n_ct, nl, scale)


def run_one_eval(g, o, name, tag, case, kind, degree, ct, rlk, d_rlk, scale):
    N, L, n_ct = g.N, g.L, ct.shape[0]
    coef = eval_coef(degree)
    if kind == "poly":
        want, want_s = poly_eval_by_hand(g, ct, d_rlk, coef, n_ct, L, scale)
        nl_out = g.poly_plan(degree, L)["nl_out"]
    else:
        want, want_s, nl_out = cheb_eval_by_hand(g, ct, d_rlk, coef, *KINDS[kind], n_ct, L, scale)
    d_ct = g.to_device(ct)
    d_big, d_out, words = guarded(g, (n_ct, 2, nl_out, N))
    s_out = dev_eval(g, kind, d_ct, d_rlk, coef, d_out, n_ct, L, scale)
    assert guards_intact(g, d_big, words), (name, tag, kind, degree, "wrote outside its output")
    same(d_ct.to_host(), ct, name, tag, kind, degree, "changed its input")
    assert s_out == want_s == g.sf(L - nl_out), (name, tag, kind, degree)
    got = d_out.to_host()
    same(got, want, name, tag, kind, degree, "by hand")
    if (kind, degree) in case:
        cpu, cpu_s = case[kind, degree]
        assert cpu_s == s_out, (name, tag, kind, degree)
        same(got[0], cpu, name, tag, kind, degree, "CPU chain")


def run_evals(g, o, name, tag, kinds=tuple(KINDS)):
    inp, lad = cached(eval_input, name), cached(ladder_case, name)
    ct, rlk, scale = inp["ct"], lad["rlk"], lad["scale"]
    d_rlk = g.to_device(rlk)
    for kind in kinds:
        case, ran = cached(EVAL_CASES[kind], name), 0
        for k, degree, why in inp["plan"]:
            if k != kind:
                continue
            if why is not None:
                d_ct, d_out = g.to_device(ct), g.empty(ct.shape)
                refused(lambda: dev_eval(g, kind, d_ct, d_rlk, eval_coef(degree), d_out, ct.shape[0], g.L, scale), why)
                continue
            run_one_eval(g, o, name, tag, case, kind, degree, ct, rlk, d_rlk, scale)
            ran = max(ran, degree)
        assert ran >= 2 or kind == "mapped", (name, kind)  # no entry without a passing evaluation in both bases


@gpu
@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", NAMES)
def test_evaluations_are_their_compositions(ctxs, name, kind):
    g, o = ctxs(name)
    run_evals(g, o, name, "default", (kind,))


SECTIONS = (test_poly_tensor_is_the_integer_definition, test_cheb_tensor_is_the_integer_definition_in_all_four_instances,
            test_affine_in_place_and_out_of_place, test_ladders_are_their_loops, test_evaluations_are_their_compositions)


# ---- device-free: coverage, the patterns' self-checks, the predicted refusals ---------------------------------------------

def test_every_section_covers_every_table_entry():
    """No device needed: each section is parametrised over exactly the names of TABLE, and the subsets are names of it."""
    for f in SECTIONS:
        over = [m.args[1] for m in f.pytestmark if m.name == "parametrize" and m.args[0] == "name"]
        assert len(over) == 1 and len(over[0]) == len(NAMES) and set(over[0]) == set(NAMES), f.__name__
        assert any(m.name == "gpu" for m in f.pytestmark), f.__name__
    assert set(BIG + DEGREES_63 + ("d1", "a45")) | {f[0] for f in FORKS} <= set(NAMES)
    assert OUTER0 + GROUP <= 1 << 8 and CHEB0 + 2 * GROUP * 5 <= 1 << 8  # the patterns fit the smallest ring's 256 columns


@pytest.mark.parametrize("name", NAMES)
def test_the_extreme_patterns_are_what_they_claim(name):
    """The builders assert it while they build (constants = q - 1 and the inner sum (q - 1) + (B - 1) (q - 1)^2 in whole
    integers; every remainder of a run within 2^8 of +q/2 or -q/2; at most 1 in 16 pattern columns redrawn): here they are
    built for every plan and layout of the entry, and what the assertions walked over is counted."""
    o = oracle(name)
    case = cached(poly_tensor_inputs, name)
    assert len(case) == 2 * len(PLANS) * len(layouts(name))
    for (kind, nl_T, B), c in case.items():
        assert nl_T in (o.L, o.L - 1) and len(c["babies"]) == B - 1 and len(c["giants"]) == c["G"] - 1
        if kind == "maximum":
            for t in range(nl_T):
                assert all(int(x[0, k, t, 0]) == int(o.moduli[t]) - 1 for x in c["babies"] + c["giants"] for k in range(2))
        else:
            assert 16 * c["redrawn"] <= GROUP
    for nl, c in cached(cheb_tensor_inputs, name).items():
        for l in range(nl):
            q = int(o.moduli[l])
            assert all(int(c[k][0, comp, l, MAX0]) == q - 1 for k in "abt" for comp in range(2))
            assert (q - py_int(c["weights"][4]) % q) % q == q - 1  # M' of the kernel's table


@pytest.mark.parametrize("name", NAMES)
def test_the_predicted_refusals_are_the_librarys(name):
    """A host-only context refuses before it asks for a device: a predicted refusal comes with its text (MKCKKS_E_INVALID),
    everything else gets as far as MKCKKS_E_NODEVICE.  Every entry keeps an evaluation of degree >= 2 in both bases."""
    from ppqsflhe_amd import Context
    from ppqsflhe_amd.binding import MkckksError
    args = TABLE[name][0]
    o = oracle(name)
    plan = eval_plan(name)
    for kind in ("poly", "cheb"):
        assert max([d for k, d, why in plan if k == kind and why is None], default=0) >= 2, (name, kind, plan)
    c = Context(args[0], args[1], args[2], device=-1, **_kwargs(args))
    try:
        big = 1 << 40
        assert c.sf_big(0) == o.sf_big(0)
        for kind, degree, why in plan:
            with pytest.raises(MkckksError) as e:
                dev_eval(c, kind, big, 2 * big, eval_coef(degree), 3 * big, 1, c.L, c.sf_big(0))
            if why is None:
                assert e.value.code == -2, (name, kind, degree, str(e.value))
            else:
                assert e.value.code == -1 and why in str(e.value), (name, kind, degree, why, str(e.value))
    finally:
        c.close()


# ---- 6: the library switches ------------------------------------------------------------------------------------------------

FORK_SECTIONS = {"poly_tensor": run_poly_tensor, "cheb_tensor": run_cheb_tensor, "ladders": run_ladders, "evals": run_evals}
SWITCH_SECTIONS = {"MKCKKS_POLY_FUSED": ("poly_tensor", "evals"), "MKCKKS_CHEB_FUSED": ("cheb_tensor", "ladders", "evals"),
                   "MKCKKS_NO_FP64": ("poly_tensor", "cheb_tensor", "evals"),
                   "MKCKKS_NO_PM": ("poly_tensor", "cheb_tensor", "evals")}


def fork_context(monkeypatch, name, switch, value, absent):
    from ppqsflhe_amd import Context
    args, shape, arith = TABLE[name]
    o = oracle(name)
    monkeypatch.setenv(switch, value)
    g2 = Context(args[0], args[1], args[2], device=0, **_kwargs(args))
    try:
        if absent is None:
            assert [int(x) for x in g2.arith] == arith, (name, switch, list(g2.arith))
        else:
            assert absent in arith and absent not in list(g2.arith), (name, switch, list(g2.arith))
        assert (g2.L, g2.K, g2.alpha, g2.beta) == shape and np.array_equal(g2.moduli, o.moduli), (name, switch)
    except BaseException:
        g2.close()
        raise
    return g2, o


@gpu
@pytest.mark.parametrize("name,switch,value,absent,section",
                         [f + (s,) for f in FORKS for s in SWITCH_SECTIONS[f[1]]])
def test_sections_under_the_library_switches(monkeypatch, name, switch, value, absent, section):
    """Switches are read once, when a context is created: the entry once more under the switch gives the reference's bits
    from the other arithmetic, or from the composition (k_wsum_ct, k_poly_add_const, k_poly_add_row, k_tensor)."""
    g2, o = fork_context(monkeypatch, name, switch, value, absent)
    try:
        FORK_SECTIONS[section](g2, o, name, (switch, value))
    finally:
        g2.close()


@gpu
def test_poly_eval_across_workspace_chunks(ctxs, monkeypatch):
    """MKCKKS_CHUNK = 1, 3 ciphertexts through poly_eval on a45 (fp64-class P limbs), in a fresh context: every chunk reuses
    the engine's buffers.  The bits are the default context's, its composition's and the CPU chain's."""
    g, o = ctxs("a45")
    inp, case, lad = cached(eval_input, "a45"), cached(EVAL_CASES["poly"], "a45"), cached(ladder_case, "a45")
    rlk, scale = lad["rlk"], lad["scale"]
    ct = np.concatenate([inp["ct"], rand_ct(np.random.default_rng(3700), o, o.L, 3 - inp["ct"].shape[0])])
    coef = eval_coef(3)
    assert ("poly", 3, None) in inp["plan"] and ("poly", 3) in case
    nl_out = g.poly_plan(3, g.L)["nl_out"]
    d_out = g.empty((3, 2, nl_out, g.N))
    s_out = g.poly_eval(g.to_device(ct), g.to_device(rlk), coef, d_out, 3, g.L, scale)
    want = d_out.to_host()
    g2, _ = fork_context(monkeypatch, "a45", "MKCKKS_CHUNK", "1", None)
    try:
        run_one_eval(g2, o, "a45", "MKCKKS_CHUNK=1", case, "poly", 3, ct, rlk, g2.to_device(rlk), scale)
        d_out2 = g2.empty((3, 2, nl_out, g.N))
        assert g2.poly_eval(g2.to_device(ct), g2.to_device(rlk), coef, d_out2, 3, g2.L, scale) == s_out
        same(d_out2.to_host(), want, "a45", "MKCKKS_CHUNK=1 against the default context")
    finally:
        g2.close()
