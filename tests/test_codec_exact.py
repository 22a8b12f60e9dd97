"""The fp64 codec and the narrow Gaussian sampler against exact references.

Everything else in this library is compared word for word with the oracle; Encode / Decode (csrc/codec_kernels.hpp,
`lift_value(double)` in engine.hip) and `k_sample_gauss` cannot be, and the oracle's own `fft_special*` is the same
algorithm as the device's, so a shared mistake would cancel.  The references here are independent of both:

* the canonical embedding written out: slot j sits at zeta^(5^j), zeta = exp(i pi / N), so for real slot values
  coefficient k of the encoding is (scale / (N/2)) sum_j vals_j cos(pi (k 5^j mod 2N) / N) and decode is the transpose
  sum / scale.  `k 5^j mod 2N` is reduced in integers, the cosine table (first quadrant, reflected) and the sums are
  np.longdouble (64-bit mantissa): O(N^2), cached per ring, log_n <= 11 only;
* closed forms at any N: a sum of cosines a_k cos(pi (k 5^j mod 2N) / N) encodes to +a_k scale / 2 at k and
  -a_k scale / 2 at N - k (a_0 scale at 0); a single slot j0 encodes to (v scale / (N/2)) cos(pi (k 5^j0 mod 2N) / N);
  a constant c encodes to the constant c scale.  The exact decode of an integer polynomial x near such a closed form
  is the closed form's slot values + the embedding of the small remainder x - closed form (fp64 FFT of numbers of a few
  units: its own error is 2^-50 of an already negligible term);
* the centred CRT in Python integers, and x / scale as a Fraction;
* D_{Z,sigma}'s cumulative table from mpmath at 80 digits and the documented ChaCha20 mapping in numpy.

Bounds.  Encode, per coefficient: |x_dev - exact| <= 0.5 + 4 max(E_oracle, U), U = scale max|vals| 2^-53, E_oracle
the oracle's own maximum error against the same exact reference on the same input (computed here; the factor 4 is for
rounding order -- x * (scale / slots) against (x / size) * scale, FMA contraction -- not for growth).  Decode, per
slot: 4 max(E_oracle, max|vals| 2^-53).  Edge integers (one coefficient x at position 0, every slot = x / scale):
relative error <= (2 nl + 2) 2^-53 against the exact rational (one multiply and one add per Horner step, the
division); at positions 1 and N/2 + 1 that term times |x / scale| plus the decode bound.  The oracle is held to the
same bounds on the CPU, and to E_oracle <= 0.5 + 2 log2(N) U (encode) and 2 log2(N) max|vals| 2^-53 (decode): the
textbook growth of a radix-2 fp64 FFT's error (about one rounded complex multiply and add, < 2 units, per stage; the
rounding of the closed form's input values to doubles adds at most one U), which makes it a usable yardstick.
The reference's own error is 2^-64 relative per term: below U / 2^10 everywhere.

Measured on the MI355X (err_dev / max(E_oracle, floor), worst case of each ring; profiles/codec_exact.txt has every
case):
  encode  r8 1.01  tiny 1.12  n11 1.08  r13 1.10  ref 1.00  c3 0.98  n17 1.00
  decode  r8 1.08  tiny 1.12  n11 1.21  r13 0.96  ref 1.04  c3 1.00  n17 1.00
so the device errs as the oracle does and the factor 4 is nowhere in use.  The nl = 32 launch of k_crt_symmetrise
(65,536 B of dynamic LDS + 96 B static) is accepted without a function attribute -- a workgroup may have all 160 KiB
of a gfx950 CU -- and its estimates match the exact integers to 1e-15.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle.oracle import OracleContext
from tests.test_decode_flood import centred_ints, chacha20_blocks, embed_real, log2_sigma_exact

LD = np.longdouble
PI = LD("3.14159265358979323846264338327950288419716939937510")
E_INVALID = -1

CONFIGS = {
    # name: (log_n, depth, scaling_bits, first_bits, dnum)
    "r8": (8, 3, 50, 60, 2),        # N/2 = 128 slots: below one 256-thread block; N/4 below one FLOOD_THREADS block
    "tiny": (10, 3, 40, 60, 2),
    "n11": (11, 2, 40, 60, 2),      # odd log N
    "r13": (13, 2, 50, 60, 2),
    "ref": (14, 2, 40, 60, 2),      # 40-bit limbs
    "c3": (16, 10, 50, 60, 3),
    "n17": (17, 2, 50, 60, 2),
    "c5s": (12, 18, 50, 60, 3),     # L = 20: Q ~ 2^980, still inside a double
    "d30n8": (8, 30, 50, 60, 4),    # L = 32 = CRT_MAX_LIMBS: Q ~ 2^1580
    "s54": (12, 2, 54, 60, 2),      # q_0 and P Shoup-class (test_parameter_lattice.TABLE)
}
ENCODE_RINGS = ["r8", "tiny", "n11", "r13", "ref", "c3", "n17"]
DENSE_MAX_LOG_N = 11

_ORACLES = {}


def oracle(name):
    if name not in _ORACLES:
        a = CONFIGS[name]
        _ORACLES[name] = OracleContext(a[0], a[1], a[2], a[3], dnum=a[4])
    return _ORACLES[name]


# ---- the embedding, written out -------------------------------------------------------------------------------------

_TABLES, _DENSE = {}, {}


def tables(N):
    """rot[j] = 5^j mod 2N (int64[N/2]); cos_t[r] = cos(pi r / N), r < 2N, longdouble: the first quadrant, reflected"""
    if N not in _TABLES:
        rot = np.empty(N // 2, dtype=np.int64)
        r = 1
        for j in range(N // 2):
            rot[j] = r
            r = r * 5 % (2 * N)
        q = np.cos(PI * np.arange(N // 2 + 1, dtype=LD) / LD(N))
        q[N // 2] = 0
        c = np.empty(2 * N, dtype=LD)
        c[:N // 2 + 1] = q
        c[N // 2 + 1:N + 1] = -q[N // 2 - 1::-1]  # cos(pi (N - r) / N) = -cos(pi r / N)
        c[N + 1:] = c[N - 1:0:-1]                 # cos(pi (2N - r) / N) = cos(pi r / N)
        _TABLES[N] = rot, c
    return _TABLES[N]


def dense_matrix(N):
    """M[k][j] = cos(pi (k 5^j mod 2N) / N), longdouble [N][N/2]"""
    assert N <= 1 << DENSE_MAX_LOG_N
    if N not in _DENSE:
        rot, c = tables(N)
        _DENSE[N] = c[(np.arange(N, dtype=np.int64)[:, None] * rot[None, :]) % (2 * N)]
    return _DENSE[N]


def encode_dense(vals, scale, N):
    return (dense_matrix(N) @ np.asarray(vals, dtype=LD)) * LD(scale) / LD(N // 2)


def decode_dense(coef, scale, N):
    return (np.asarray(coef, dtype=LD) @ dense_matrix(N)) / LD(scale)


def cos_row(N, k):
    """cos(pi (k 5^j mod 2N) / N) over the slots j"""
    rot, c = tables(N)
    return c[(k * rot) % (2 * N)]


def cos_col(N, j0):
    """cos(pi (k 5^j0 mod 2N) / N) over the coefficients k"""
    rot, c = tables(N)
    return c[(np.arange(N, dtype=np.int64) * int(rot[j0])) % (2 * N)]


def sparse_form(N, ks, amps, scale):
    """slot values sum_k a_k cos(pi (k 5^j mod 2N) / N) (longdouble) and their exact encoding"""
    vals = np.zeros(N // 2, dtype=LD)
    coef = np.zeros(N, dtype=LD)
    for k, a in zip(ks, amps):
        assert 0 <= k < N and k != N // 2
        vals += LD(a) * cos_row(N, k)
        if k == 0:
            coef[0] += LD(a) * LD(scale)
        else:
            coef[k] += LD(a) * LD(scale) / 2
            coef[N - k] -= LD(a) * LD(scale) / 2
    return vals, coef


def single_slot_form(N, j0, v, scale):
    vals = np.zeros(N // 2, dtype=LD)
    vals[j0] = LD(v)
    return vals, LD(v) * LD(scale) / LD(N // 2) * cos_col(N, j0)


def to_ld(x):
    """object array of Python ints (|x| < 2^95) -> longdouble, rounded once"""
    x = np.asarray(x, dtype=object)
    return (x >> 32).astype(np.int64).astype(LD) * LD(2 ** 32) + (x & 0xFFFFFFFF).astype(np.int64).astype(LD)


def crt2(o, r0, r1):
    """residues modulo q_0 and q_1 -> centred Python ints"""
    q0, q1 = int(o.moduli[0]), int(o.moduli[1])
    a = r0.astype(object)
    x = a + q0 * (((r1.astype(object) - a) * pow(q0, -1, q1)) % q1)
    return np.where(x > (q0 * q1) // 2, x - q0 * q1, x)


def coefficients(o, pt):
    """an evaluation-format plaintext [>= 2][N] -> its centred integer coefficients (limbs 0 and 1)"""
    return crt2(o, o.ntt_inv(0, pt[0]), o.ntt_inv(1, pt[1]))


def ld_ratio(x, scale):
    """x / scale (Python int over a power of two) as a longdouble, rounded once"""
    v = Fraction(x) / Fraction(scale)
    hi = float(v)
    return LD(hi) + LD(float(v - Fraction(hi)))


class Case:
    """one encode input: vals (the doubles given to encode), coef (exact real coefficients, longdouble), slots (the exact
    slot values of `coef`, longdouble), and the oracle's integers with their error E against coef"""

    def __init__(self, tag, N, slots, coef, scale):
        self.tag, self.N, self.scale = tag, N, scale
        self.slots, self.coef = slots, coef
        self.vals = slots.astype(np.float64)
        self.vmax = float(np.abs(self.vals).max())
        self.U = scale * self.vmax * 2.0 ** -53

    def exact_decode(self, x):
        """exact slot values of the integer polynomial x (Python ints) / scale"""
        if self.tag == "dense":
            return decode_dense(to_ld(x), self.scale, self.N)
        rest = (to_ld(x) - self.coef).astype(np.float64)
        assert np.abs(rest).max() < 2.0 ** 30  # x is this case's encoding, up to rounding
        return self.slots + embed_real(rest).astype(LD) / LD(self.scale)


_RINGS = {}


def ring_cases(name):
    """the inputs of sections 2 and 4 on one ring, with the oracle's encodings: built once"""
    if name not in _RINGS:
        o = oracle(name)
        N, log_n = o.N, CONFIGS[name][0]
        scale = o.sf_big(0)
        rng = np.random.default_rng(1000 + log_n)
        cases = []
        if log_n <= DENSE_MAX_LOG_N:
            vals = rng.uniform(-0.3, 0.3, N // 2)
            cases.append(Case("dense", N, vals.astype(LD), encode_dense(vals, scale, N), scale))
        ks = [0, 1, 2, N // 4, N // 2 - 1, N // 2 + 1, N - 1, int(rng.integers(3, N // 4))]
        cases.append(Case("sparse", N, *sparse_form(N, ks, rng.uniform(-0.04, 0.04, len(ks)), scale), scale))
        cases.append(Case("slot0", N, *single_slot_form(N, 0, 0.3 * rng.uniform(0.5, 1), scale), scale))
        cases.append(Case("slot_last", N, *single_slot_form(N, N // 2 - 1, -0.3 * rng.uniform(0.5, 1), scale), scale))
        cases.append(Case("mean", N, *single_slot_form(N, 0, rng.normal(0, 0.05), scale), scale))
        for c in cases:
            c.x_oracle = coefficients(o, o.encode(c.vals, scale, 2))
            c.E = float(np.abs(to_ld(c.x_oracle) - c.coef).max())
        _RINGS[name] = cases
    return _RINGS[name]


def batches(cases):
    """items of three with an all-zero one in the middle: [(case, None, case), ...]"""
    out = []
    for i in range(0, len(cases), 2):
        out.append((cases[i], None, cases[i + 1] if i + 1 < len(cases) else cases[0]))
    return out


def batch_vals(batch, N):
    return np.stack([np.zeros(N // 2) if c is None else c.vals for c in batch])


def report(kind, name, tag, err, yard, bound):
    print(f"codec_exact {kind:6s} {name:6s} {tag:10s} err={err:.6g} yardstick={yard:.6g} ratio={err / yard:.3f} "
          f"bound={bound:.6g}")


def check_encode(name, case, x):
    err = float(np.abs(to_ld(x) - case.coef).max())
    yard = max(case.E, case.U)
    bound = 0.5 + 4 * yard
    report("encode", name, case.tag, err, yard, bound)
    assert err <= bound, (name, case.tag, err, case.E, case.U)


def check_decode(name, case, x, got, ref):
    """got: the decoder under test on the integer polynomial x; ref: the oracle's decode of the same polynomial"""
    exact = case.exact_decode(x)
    E = float(np.abs(ref.astype(LD) - exact).max())
    err = float(np.abs(got.astype(LD) - exact).max())
    yard = max(E, case.vmax * 2.0 ** -53)
    report("decode", name, case.tag, err, yard, 4 * yard)
    assert err <= 4 * yard, (name, case.tag, err, E)
    return E


def trivial_ct(pt):
    """(pt, 0): decrypts to INTT(pt) under any key"""
    ct = np.zeros((2,) + pt.shape, dtype=np.uint64)
    ct[0] = pt
    return ct


# ---- CPU: the references against each other, and the oracle alone within the bounds ---------------------------------

@pytest.mark.parametrize("log_n", [8, 10])
def test_dense_formula_and_closed_forms_agree(log_n):
    N, scale = 1 << log_n, 2.0 ** 50
    rng = np.random.default_rng(log_n)
    tol = LD(scale) * LD(2.0 ** -58)  # values below 1/2; N/2 <= 512 terms, each rounded at 2^-64
    ks = [0, 1, 2, N // 4, N // 2 - 1, N // 2 + 1, N - 1, int(rng.integers(3, N // 4))]
    forms = [sparse_form(N, ks, rng.uniform(-0.04, 0.04, len(ks)), scale),
             single_slot_form(N, 0, 0.25, scale), single_slot_form(N, N // 2 - 1, -0.2, scale)]
    const = np.zeros(N, dtype=LD)
    const[0] = LD(0.125) * LD(scale)
    forms.append((np.full(N // 2, 0.125, dtype=LD), const))
    for slots, coef in forms:
        assert np.abs(encode_dense(slots, scale, N) - coef).max() <= tol
        assert np.abs(decode_dense(coef, scale, N) - slots).max() <= tol / LD(scale) * N
    # cos(pi (N/2) 5^j / N) = 0: coefficient N/2 never carries a real message
    assert not cos_row(N, N // 2).any()


@pytest.mark.parametrize("name", ENCODE_RINGS)
def test_oracle_encode_and_decode_within_the_bounds(name):
    o = oracle(name)
    N, L, log_n = o.N, o.L, CONFIGS[name][0]
    zero_sk = np.zeros((o.D, N), dtype=np.uint64)
    for case in ring_cases(name):
        check_encode(name, case, case.x_oracle)
        assert case.E <= 0.5 + 2 * log_n * case.U, (name, case.tag, case.E, case.U)
        pt = o.encode(case.vals, case.scale, L)
        for l in range(2, L):  # every limb holds the same integers
            q = int(o.moduli[l])
            assert np.array_equal(o.ntt_inv(l, pt[l]), (case.x_oracle % q).astype(np.uint64)), (name, case.tag, l)
        dec = o.decrypt_decode(trivial_ct(pt), zero_sk, case.scale)
        E = check_decode(name, case, case.x_oracle, dec, dec)
        assert E <= 2 * log_n * case.vmax * 2.0 ** -53, (name, case.tag, E)
    zero = o.encode(np.zeros(N // 2), ring_cases(name)[0].scale, L)
    assert not zero.any()


# ---- edge integers of the centred CRT ------------------------------------------------------------------------------

EDGE_CASES = [("tiny", 1), ("tiny", 2), ("tiny", 5), ("c5s", 20), ("d30n8", 32)]
FP64_LIFT_LIMIT = 1000  # the device lifts in fp64: at nl = 32 only |x| < 2^1000 (include/mkckks.h, mkckks_decode_batch)


def mixed_radix(digits, qs):
    x = 0
    for d, q in zip(reversed(digits), reversed(qs)):
        x = x * q + d
    return x


def edge_values(moduli, nl):
    """centred integers at the branches of crt_centred: around 0, around (Q - 1) / 2, and for every limb t the two
    neighbours of the tie 'digits above t equal (q_a - 1) / 2': digit t one above with zeros below (the smallest
    negative lift with that prefix), digit t one below with q_a - 1 below (the largest positive one)"""
    qs = [int(q) for q in moduli[:nl]]
    Q = math.prod(qs)
    h = (Q - 1) // 2
    half = [(q - 1) // 2 for q in qs]
    assert mixed_radix(half, qs) == h
    if Q.bit_length() > FP64_LIFT_LIMIT:
        xs = [0, 1, -1, 2 ** 52 + 1, -(2 ** 53 + 1), 2 ** 999 + 12345, math.prod(qs[:16]) + 1, -(2 ** 900 + 3),
              -math.prod(qs[:7]) - 1]
    else:
        xs = [0, 1, -1, h, h + 1, h - 1, h + 2, Q - 1, 2 ** 52 + 1, -(2 ** 53 + 1)]
        for t in range(nl):
            xs.append(mixed_radix([0] * t + [half[t] + 1] + half[t + 1:], qs))
            xs.append(mixed_radix([q - 1 for q in qs[:t]] + [half[t] - 1] + half[t + 1:], qs))
    out = []
    for x in xs:
        x %= Q
        out.append(x - Q if x > h else x)
    return out, Q


def edge_scale(Q):
    """a power of two that keeps every x / scale, 1 <= |x| <= Q / 2, finite and normal"""
    return 2.0 ** max(1, min(Q.bit_length(), FP64_LIFT_LIMIT) - 64)


def one_coefficient(moduli, nl, N, xs, pos):
    """[len(xs)][nl][N] coefficient-format residues of the polynomials x * X^pos"""
    m = np.zeros((len(xs), nl, N), dtype=np.uint64)
    for i, x in enumerate(xs):
        for a in range(nl):
            m[i, a, pos] = x % int(moduli[a])
    return m


def check_edges_at_zero(tag, nl, xs, scale, got):
    """position 0: every slot = x / scale, relative error (2 nl + 2) 2^-53 against the exact rational"""
    rel = Fraction(2 * nl + 2, 2 ** 53)
    for i, x in enumerate(xs):
        exact = Fraction(x) / Fraction(scale)
        assert math.isfinite(float(exact)) and (x == 0 or abs(float(exact)) >= 2.0 ** -1022)
        for v in np.unique(got[i]):
            assert math.isfinite(v), (tag, nl, i, x, v)
            err = abs(Fraction(float(v)) - exact)
            assert err <= rel * abs(exact), (tag, nl, i, x, float(v), float(exact), float(err / abs(exact)) * 2.0 ** 53)


def check_edges_at(tag, o, nl, xs, scale, pos, got, ref):
    """position pos > 0: slot j = (x / scale) cos(pi (pos 5^j mod 2N) / N)"""
    for i, x in enumerate(xs):
        r = ld_ratio(x, scale)
        exact = r * cos_row(o.N, pos)
        E = float(np.abs(ref[i].astype(LD) - exact).max())
        mag = abs(float(r))
        bound = (2 * nl + 2) * 2.0 ** -53 * mag + 4 * max(E, mag * 2.0 ** -53)
        err = float(np.abs(got[i].astype(LD) - exact).max())
        assert err <= bound, (tag, nl, pos, i, x, err, bound, E)


def shifted_subset(xs):
    """a few of the edge values for positions 1 and N/2 + 1: the small ones, the two around the top tie, the last tie"""
    pick = [x for x in xs[1:3]] + [x for x in xs[3:5]] + [2 ** 52 + 1, xs[-2], xs[-1]]
    return list(dict.fromkeys(pick))


def oracle_decode(o, m, scale):
    """the oracle's decode of coefficient-format residues [items][nl][N], through the trivial ciphertext"""
    zero_sk = np.zeros((o.D, o.N), dtype=np.uint64)
    out = []
    for item in m:
        pt = np.stack([o.ntt_fwd(a, item[a]) for a in range(item.shape[0])])
        out.append(o.decrypt_decode(trivial_ct(pt), zero_sk, scale))
    return np.stack(out)


@pytest.mark.parametrize("name,nl", EDGE_CASES)
def test_oracle_decodes_edge_integers(name, nl):
    o = oracle(name)
    xs, Q = edge_values(o.moduli, nl)
    scale = edge_scale(Q)
    check_edges_at_zero("oracle", nl, xs, scale, oracle_decode(o, one_coefficient(o.moduli, nl, o.N, xs, 0), scale))
    sub = shifted_subset(xs)
    for pos in (1, o.N // 2 + 1):
        ref = oracle_decode(o, one_coefficient(o.moduli, nl, o.N, sub, pos), scale)
        check_edges_at("oracle", o, nl, sub, scale, pos, ref, ref)


# ---- the narrow Gaussian, restated ---------------------------------------------------------------------------------

def gauss_thresholds(sigma):
    """thr[k] = floor(2^64 P(|x| <= k)) for D_{Z,sigma} cut at ceil(12 sigma); the last entry saturates"""
    import mpmath
    with mpmath.workdps(80):
        count = math.ceil(12.0 * sigma) + 1
        s2 = 2 * mpmath.mpf(sigma) ** 2
        w = [mpmath.exp(-mpmath.mpf(k * k) / s2) * (2 if k else 1) for k in range(count)]
        total, acc, thr = mpmath.fsum(w), mpmath.mpf(0), []
        for k in range(count):
            acc += w[k]
            thr.append(min(int(mpmath.floor(acc / total * 2 ** 64)), 2 ** 64 - 1))
        thr[-1] = 2 ** 64 - 1
    return thr


def gauss_words(key, sid, count):
    """(r, sign) of elements i < count: block i / 4 under nonce (block >> 32, sid, 0); r = 64-bit word 2 (i % 4), the sign
    bit 0 of the next 32-bit word"""
    i = np.arange(count, dtype=np.uint64)
    b = i >> np.uint64(2)
    blk = chacha20_blocks(key, (b & np.uint64(0xFFFFFFFF)).astype(np.uint32), (b >> np.uint64(32)).astype(np.uint32),
                          sid, 0).astype(np.uint64)
    j = (i & np.uint64(3)).astype(np.int64)
    row = np.arange(count)
    return blk[row, 4 * j] | (blk[row, 4 * j + 1] << np.uint64(32)), (blk[row, 4 * j + 2] & np.uint64(1)).astype(bool)


def gauss_restated(key, sid, count, sigma):
    thr = np.array(gauss_thresholds(sigma), dtype=np.uint64)
    r, sign = gauss_words(key, sid, count)
    k = np.searchsorted(thr[:-1], r, side="right").astype(np.int32)  # the first index with r < thr[k]
    return np.where(sign, -k, k).astype(np.int32), r, thr


def test_gauss_table_is_the_discrete_gaussian():
    """the restated table against the distribution's definition in plain floats, and its documented shape"""
    for sigma in (3.19, 0.8, 3.9):
        thr = gauss_thresholds(sigma)
        assert len(thr) == math.ceil(12 * sigma) + 1 <= 48 and thr[-1] == 2 ** 64 - 1
        assert all(a <= b for a, b in zip(thr, thr[1:]))
        S = sum(math.exp(-k * k / (2 * sigma * sigma)) for k in range(-60, 61))
        cum = 0.0
        for k in range(6):
            cum += math.exp(-k * k / (2 * sigma * sigma)) * (2 if k else 1) / S
            assert abs(thr[k] / 2.0 ** 64 - cum) < 1e-12, (sigma, k)


# ---- GPU -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctxs():
    from ppqsflhe_amd import Context
    cache = {}

    def get(name):
        if name not in cache:
            a = CONFIGS[name]
            cache[name] = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)
        g, o = cache[name], oracle(name)
        assert np.array_equal(g.moduli, o.moduli), name
        return g, o

    yield get
    for g in cache.values():
        g.close()


@pytest.fixture(scope="module")
def encoded(ctxs):
    """the device's encodings of ring_cases(name), in batches of three with a zero item in the middle: [(batch, pt)]"""
    cache = {}

    def get(name):
        if name not in cache:
            g, _ = ctxs(name)
            out = []
            for batch in batches(ring_cases(name)):
                d_pt = g.empty((3, g.L, g.N))
                g.encode(g.to_device(batch_vals(batch, g.N)), d_pt, 3, g.L, batch[0].scale)
                out.append((batch, d_pt.to_host()))
            cache[name] = out
        return cache[name]

    return get


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENCODE_RINGS)
def test_encode_on_device(ctxs, encoded, name):
    g, o = ctxs(name)
    for batch, pt in encoded(name):
        assert not pt[1].any(), (name, "the all-zero item")
        for i in (0, 2):
            x = coefficients(o, pt[i])
            for l in range(2, g.L):  # every limb holds the same integers
                q = int(g.moduli[l])
                assert np.array_equal(o.ntt_inv(l, pt[i, l]), (x % q).astype(np.uint64)), (name, batch[i].tag, l)
            check_encode(name, batch[i], x)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "s54", "c3"])
def test_encode_powers_of_two_bit_exact(ctxs, name):
    """scale = 2^s, vals = +-2^k constant: the evaluation-format constant (+-2^(k+s)) mod q_l in every word.  s + k = 62,
    63, 64 cross the a < 2^63 switch of lift_value(double); 100 and 119 reach its sh >= 64 branch."""
    g, _ = ctxs(name)
    N, L = g.N, g.L
    for s, k in ((59, 3), (66, -3), (60, 4), (97, 3), (119, 0), (121, -2)):
        vals = np.stack([np.full(N // 2, 2.0 ** k), np.full(N // 2, -(2.0 ** k))])
        d_pt = g.empty((2, L, N))
        g.encode(g.to_device(vals), d_pt, 2, L, 2.0 ** s)
        pt = d_pt.to_host()
        for b, sign in enumerate((1, -1)):
            for l in range(L):
                want = (sign * 2 ** (k + s)) % int(g.moduli[l])
                assert (pt[b, l] == np.uint64(want)).all(), (name, s, k, sign, l, int(pt[b, l, 0]), want)


LIFT_EXTREMES = ([2.0 ** 63 - 1024, 2.0 ** 63, 2.0 ** 64, 2.0 ** 120 - 2.0 ** 67, 0.49999999999999994, 1.5, 2.5]
                 + [2.0 ** 52 + 0.5, 2.0 ** 52 - 0.5, 2.0 ** 53 - 1, 2.0 ** 100, 2.0 ** 119])


def round_half_away(x):
    f = Fraction(x)
    n = int(abs(f) + Fraction(1, 2))
    return -n if f < 0 else n


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "c3", "s54"])
def test_lift_ntt_extremes(ctxs, name):
    g, o = ctxs(name)
    N, L = g.N, g.L
    special = [s * v for v in LIFT_EXTREMES for s in (1.0, -1.0)] + [-0.0, 0.0]
    assert 2.0 ** 63 - 1024 < 2.0 ** 63 and 2.0 ** 120 - 2.0 ** 67 < 2.0 ** 120 and 0.49999999999999994 + 0.5 == 1.0
    rng = np.random.default_rng(16)
    coef = np.rint(rng.normal(0, 2.0 ** 45, size=(1, N)))
    coef[0, :len(special)] = special
    assert math.copysign(1.0, coef[0, len(special) - 2]) == -1.0
    ints = [round_half_away(x) for x in coef[0, :len(special)]] + [int(x) for x in coef[0, len(special):]]
    d_out = g.empty((1, L, N))
    g.lift_ntt(g.to_device(coef), d_out, 1, L)
    got = d_out.to_host()
    for l in (0, 1, L - 1):
        q = int(g.moduli[l])
        res = np.array([v % q for v in ints], dtype=np.uint64)
        lifted = o.ntt_inv(l, got[0, l])  # names the coefficients that differ; the comparison itself is the next line's
        bad = np.flatnonzero(lifted != res)[:8]
        assert not bad.size, (name, l, [(int(i), float(coef[0, i]), int(lifted[i]), int(res[i])) for i in bad])
        assert np.array_equal(got[0, l], o.ntt_fwd(l, res)), (name, l)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ENCODE_RINGS)
def test_decode_on_device(ctxs, encoded, name):
    """the integer polynomials the device encoded, through decrypt of the trivial ciphertext (pt, 0) under a zero key"""
    g, o = ctxs(name)
    N, L, slots = g.N, g.L, g.N // 2
    zero_sk = np.zeros((g.D, N), dtype=np.uint64)
    d_sk = g.to_device(zero_sk)
    for batch, pt in encoded(name):
        ct = np.stack([trivial_ct(pt[i]) for i in range(3)])
        d_m, d_vals = g.empty((3, L, N)), g.empty((3, slots), dtype=np.float64)
        g.decrypt(g.to_device(ct), d_sk, d_m, 3, L)
        g.decode(d_m, d_vals, 3, L, batch[0].scale)
        got = d_vals.to_host()
        assert not got[1].any(), (name, "the all-zero item")
        for i in (0, 2):
            x = coefficients(o, pt[i])
            check_decode(name, batch[i], x, got[i], o.decrypt_decode(ct[i], zero_sk, batch[i].scale))


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl", EDGE_CASES)
def test_decode_edge_integers_on_device(ctxs, name, nl):
    g, o = ctxs(name)
    N, slots = g.N, g.N // 2
    xs, Q = edge_values(g.moduli, nl)
    scale = edge_scale(Q)

    def decode(m):
        d_vals = g.empty((m.shape[0], slots), dtype=np.float64)
        g.decode(g.to_device(m), d_vals, m.shape[0], nl, scale)
        return d_vals.to_host()

    check_edges_at_zero(name, nl, xs, scale, decode(one_coefficient(g.moduli, nl, N, xs, 0)))
    sub = shifted_subset(xs)
    for pos in (1, N // 2 + 1):
        m = one_coefficient(g.moduli, nl, N, sub, pos)
        check_edges_at(name, o, nl, sub, scale, pos, decode(m), oracle_decode(o, m, scale))


def flood_items(o, nl, rng):
    """three decrypted polynomials as exact integers: small noise; the same with two pairs (j, N - j) whose residues add
    up past Q (x_j = (Q - 1) / 2, x_{N-j} = 7 - (Q - 1) / 2: one lift on each side of Q / 2, d = 7); all zero"""
    N = o.N
    Q = math.prod(int(q) for q in o.moduli[:nl])
    h = (Q - 1) // 2
    xs = [rng.integers(-1024, 1025, N).astype(object) for _ in range(2)] + [np.zeros(N, dtype=np.int64).astype(object)]
    xs[1][3], xs[1][N - 3] = h, 7 - h                     # thread 3, its first pair
    xs[1][N // 2 - 5], xs[1][N // 2 + 5] = -h, h - 11     # thread 5, its second pair
    xs[1][N // 2] = -3                                    # d_{N/2} = 2 m_{N/2}, counted once
    m = np.stack([np.stack([(x % int(o.moduli[a])).astype(np.uint64) for a in range(nl)]) for x in xs])
    return xs, m


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl", [("tiny", 1), ("r8", 5), ("c5s", 20), ("d30n8", 32)])
def test_decode_flood_estimator_at_the_limb_count_limits(ctxs, name, nl):
    """nl = 1, nl = 32 = CRT_MAX_LIMBS (k_crt_symmetrise's u64[32][256] of dynamic LDS: 64 KiB on top of its static 96 B)
    and N = 2^8, where N / 4 is below one FLOOD_THREADS block"""
    g, o = ctxs(name)
    rng = np.random.default_rng(41)
    xs, m = flood_items(o, nl, rng)
    want = [log2_sigma_exact(x) for x in xs]
    for x, mi in zip(xs, m):
        assert np.array_equal(centred_ints(mi, o.moduli), x)
    assert want[2] == -math.inf and all(w < CONFIGS[name][2] - 5 for w in want)
    d_vals = g.empty((3, g.N // 2), dtype=np.float64)
    got = g.decode_flood(g.to_device(m), d_vals, 3, nl, 2.0 ** CONFIGS[name][2], bytes(range(32)))
    print(f"codec_exact flood  {name:6s} nl={nl} log2 sigma = {[float(x) for x in got]} (exact {want})")
    assert got[2] == -math.inf
    for w, x in zip(want[:2], got[:2]):
        assert abs(w - x) < 1e-9, (name, nl, want, list(got))
    assert np.isfinite(d_vals.to_host()).all()


GAUSS_KEY = bytes((7 * i + 1) & 0xFF for i in range(32))


def device_gauss(g, count, sigma, key, sid):
    d = g.empty((max(count, 1),), dtype=np.int32)
    g.sample_gauss(d, count, sigma, key, sid)
    return d.to_host()[:count]


@pytest.mark.gpu
@pytest.mark.parametrize("sigma", [3.19, 0.8, 3.9])
def test_sample_gauss_word_for_word(ctxs, sigma):
    g, _ = ctxs("tiny")
    n = 1 << 18
    for sid in (1, 0x80000002):
        want, r, thr = gauss_restated(GAUSS_KEY, sid, n, sigma)
        got = device_gauss(g, n, sigma, GAUSS_KEY, sid)
        if not np.array_equal(got, want):
            for i in np.flatnonzero(got != want)[:8]:
                k = abs(int(want[i]))
                print(f"draw {i}: r = {int(r[i])}, device {int(got[i])}, restated {int(want[i])}, thresholds "
                      f"{int(thr[k - 1]) if k else 0} .. {int(thr[k])}")
            raise AssertionError((sigma, sid, int((got != want).sum())))
        assert np.abs(want).max() <= math.ceil(12 * sigma)
    # the result does not depend on count: a shorter call, not a multiple of 4, is a prefix of the longer one
    short = device_gauss(g, n - 4093, sigma, GAUSS_KEY, 0x80000002)
    assert np.array_equal(short, want[:n - 4093])


@pytest.mark.gpu
def test_sample_gauss_call_properties(ctxs):
    from ppqsflhe_amd import MkckksError
    g, _ = ctxs("tiny")
    d = g.to_device(np.full(64, 12345, dtype=np.int32))
    g.sample_gauss(d, 0, 3.19, GAUSS_KEY, 0)
    assert (d.to_host() == 12345).all()  # count == 0 writes nothing
    g.sample_gauss(d, 3, 3.19, GAUSS_KEY, 0)
    out = d.to_host()
    assert np.array_equal(out[:3], gauss_restated(GAUSS_KEY, 0, 3, 3.19)[0]) and (out[3:] == 12345).all()
    for sigma in (3.92, 0.0, -1.0, math.nan):
        with pytest.raises(MkckksError) as ei:
            g.sample_gauss(d, 8, sigma, GAUSS_KEY, 0)
        assert ei.value.code == E_INVALID, sigma
    assert (d.to_host()[3:] == 12345).all()
