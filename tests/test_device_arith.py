"""The modular-arithmetic primitives of modarith.hpp and the butterflies of ntt_kernels.hpp / ntt_radix.hpp, one at a time,
at the edges of their documented domains, against Python integers.

Every stored word of the library goes through these primitives.  Each exists in a host form (plain C++) and a device
form (inline v_mad_u64_u32 / v_addc_co_u32 strings, alignbit, carries held in scalar pairs); the fp64 primitives have a
device form only.  Whole kernels are fed canonical residues and cannot steer an internal lazy word to the top of its
range, so this file drives each primitive alone through Context.debug_arith (mkckks_debug_arith):

* operands: (a) the full cross product of per-operand edge sets (0, 1, 2^32 - 1, 2^32, q - 1, q, 2q - 1, the top of the
  documented domain and the word below it, all-ones low half under the largest admissible high half), (b) uniform draws
  over the documented domain under a fixed seed, (c) for fp64 and prime q, pairs whose product sits next to a half-integer
  multiple of q (made through w^-1), at magnitudes across the domain.  A register round has 31 operands: its edge part is
  the cross product of whole-vector patterns (all at the bound, all zero, alternating, one hot) instead.  No operand
  leaves the domain the code documents.
* reference: Python integers (int, pow, %); nothing comes from the oracle or the library.
* coverage: for every carry / select inside a device form the tuples on each side are counted FROM THE PYTHON MODEL and
  both counts must be positive, so the host-context run shows the inputs reach both sides before a GPU is involved.
  The subtraction of 2q at the end of Barrett's reduction is the one select with a side that most moduli cannot reach:
  barrett_sup bounds the estimate's error, the model must never see that side where the bound proves it away (every
  prime next to a power of two), and a general 60-bit prime (B60) is in the list at which it is taken and left.
* CPU tests (device = -1 context, host forms): residue, documented output range, exact words where the result is
  canonical or a 128-bit sum; rounds against the exact 16-point partial transform.
* GPU tests: integer and pseudo-Mersenne device words equal the host words bit for bit; fp64 outputs are integer-valued,
  congruent and within the magnitude bound the code's comments state (derivable bounds, no measured tolerance).  The largest
  |out| / q seen per op and modulus is printed next to its bound (profiles/device_arith.txt is such a run: set
  MKCKKS_ARITH_MARGINS to a file name to write one).
"""
import functools
import itertools
import os
import random
from fractions import Fraction

import numpy as np
import pytest

from ppqsflhe_amd.binding import ARITH_OPS

M64 = (1 << 64) - 1
FP_LIMIT = 5 << 48
N_RANDOM = 1 << 13  # uniform draws per op and modulus
N_ROUND = 1 << 10   # ... for a register round (31 operands each)


# ---- moduli -----------------------------------------------------------------------------------------------------------
def is_prime(n):
    """Deterministic Miller-Rabin for n < 2^64 (first twelve primes as witnesses)."""
    if n < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in small:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in small:
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def pm_eligible(q):
    k = q.bit_length()
    return 40 <= k <= 60 and (1 << k) - q <= 1 << (k - 34)


@functools.lru_cache(maxsize=None)
def context_moduli(args):
    from ppqsflhe_amd import Context
    c = Context(args[0], args[1], args[2], args[3], dnum=args[4], aux_bits=args[5], extra_bits=args[6], device=-1)
    m = [int(x) for x in c.moduli]
    L = c.L
    c.close()
    return m, L


@functools.lru_cache(maxsize=None)
def moduli():
    """name -> q.  Integer class: the reference context's q_0 and special primes, the 55- and 58-bit primes of
    pm_glue_selftest.cpp, the 52-bit pseudo-Mersenne q_0 of context "f52", a Shoup-only 54-bit scaling prime of context
    "s54", a 20-bit prime (the extra limb).  fp64 class: 557057, a 40-bit prime, 50-bit primes above and below 2^50 as
    a context generates them, the largest prime below 5 * 2^48 (that is 5 * 2^48 - 1 itself: the widest modulus the class
    admits is a prime) and the largest odd non-prime below it, 5 * 2^48 - 3, for the ops that need no inverse."""
    ref, L = context_moduli((14, 2, 40, 60, 2, 60, 20))
    out = {"q0": ref[0]}
    for i, q in enumerate(ref[L:]):
        out[f"p{i}"] = q
    out["e20"] = ref[L - 1]
    out["s40"] = ref[1]
    out["k55"] = context_moduli((14, 2, 40, 55, 2, 60, 20))[0][0]
    out["k58"] = context_moduli((14, 2, 40, 58, 2, 60, 20))[0][0]
    out["f52"] = context_moduli((12, 2, 40, 52, 2, 60, 20))[0][0]
    s54, L54 = context_moduli((12, 2, 54, 60, 2, 60, 20))
    out["s54"] = next(q for q in s54[1:L54 - 1] if not pm_eligible(q))
    s50, L50 = context_moduli((12, 3, 50, 60, 2, 60, 20))
    out["s50lo"] = max(q for q in s50[1:L50 - 1] if q < 1 << 50)
    out["s50hi"] = min(q for q in s50[1:L50 - 1] if q > 1 << 50)
    out["b60"] = B60
    out["tiny"] = 557057
    top = FP_LIMIT - 1
    while not is_prime(top):
        top -= 2
    out["fptop"] = top
    odd = FP_LIMIT - 1
    while is_prime(odd):
        odd -= 2
    out["fpodd"] = odd
    return out


# Every prime a context generates sits next to a power of two, and for those Barrett's estimate is never 2 short (see
# barrett_sup): b60 is a 60-bit prime just above 2^59 with frac(2^122 / q) = 0.95, the general modulus at which the
# subtraction of 2q in barrett_reduce128 / reduce_cols is taken and reduce_cols_lazy returns words above 2q
B60 = 576460752488429881
INT_MODULI = ["q0", "p0", "p1", "k55", "k58", "f52", "s54", "e20", "b60"]
PM_MODULI = ["q0", "p0", "p1", "k55", "k58", "f52"]
FP_MODULI = ["tiny", "s40", "s50lo", "s50hi", "fptop", "fpodd"]


def test_moduli_have_the_widths_and_forms_the_ops_need():
    m = moduli()
    assert m["q0"].bit_length() == 60 and m["p0"].bit_length() == 60 and m["p1"].bit_length() == 60
    assert len({m["q0"], m["p0"], m["p1"]}) == 3
    assert m["b60"].bit_length() == 60 and barrett_sup("barrett_reduce128", m["b60"]) > Fraction(14, 10)
    assert barrett_sup("reduce_cols", m["b60"]) > Fraction(14, 10)
    assert m["k55"].bit_length() == 55 and m["k58"].bit_length() == 58 and m["f52"].bit_length() == 52
    assert all(pm_eligible(m[n]) for n in PM_MODULI)
    assert m["s54"].bit_length() in (54, 55) and not pm_eligible(m["s54"])
    assert m["e20"].bit_length() == 20 and m["s40"].bit_length() in (40, 41)
    assert m["s50lo"] < 1 << 50 < m["s50hi"] < FP_LIMIT and m["s50lo"].bit_length() == 50
    assert is_prime(m["fptop"]) and m["fptop"] == FP_LIMIT - 1
    assert not is_prime(m["fpodd"]) and m["fpodd"] == FP_LIMIT - 3
    for n in INT_MODULI + FP_MODULI[:5]:
        assert is_prime(m[n]), n
    # reduce_cols_lazy shifts the middle column left (e1 = 32 - k >= 0) for the 20-bit prime and right for the others
    assert 32 - m["e20"].bit_length() >= 0 and all(32 - m[n].bit_length() < 0 for n in INT_MODULI if n != "e20")


def barrett_sup(op, q):
    """Upper bound of X / q - (Barrett's quotient estimate as a real number) for op under q.  With a = X / 2^(k-2) the
    window, m = 2^(62+k) / q and the truncated fractions f1 (of the window; up to two floors in reduce_cols) and
    f2 = frac(m), the error is (f1 m + a f2 - f1 f2) / 2^64 < F 2^(k-2) / q + f2 sup(a) / 2^64.  The estimate is 2 short
    of the quotient (the subtraction of 2q is taken) only if the error exceeds 1: where this bound is <= 1 that side is
    unreachable, which the checks assert from the model.  It is always below 1.5: remainders stay below 2.5q."""
    k = q.bit_length()
    m64, f2 = Fraction(1 << (k - 2), q), Fraction(1 << (62 + k), q) % 1
    if op == "barrett_reduce128":
        return m64 + f2                                        # X < 2^(k+62): a < 2^64
    if op == "mul_mod":
        return m64 + f2 * Fraction(1 << (k + 2), 1 << 64)      # X < q^2: a < 2^(k+2)
    if op == "reduce_word":
        return m64 + f2 * min(1, Fraction(1 << (66 - k), 1 << 64))
    if op in ("reduce_wide", "reduce_cols4"):                  # folded X' < 2^(k+60) + 2^64
        return m64 + f2 * Fraction((1 << 62) + (1 << (66 - k)), 1 << 64)
    if op in ("reduce_cols", "reduce_cols_lazy"):              # S < 4 2^60 q: a < 2^64 q / 2^k
        return (2 if k - 2 > 30 else 1) * m64 + f2 * Fraction(q, 1 << k)
    raise KeyError(op)


# ---- operand sets ------------------------------------------------------------------------------------------------------
def edge_set(q, top, extra=()):
    """Edge words of an operand whose domain is [0, top]."""
    s = {0, 1, (1 << 32) - 1, 1 << 32, q - 1, q, 2 * q - 1, top, top - 1}
    if top >> 32:
        v = ((top >> 32) << 32) | 0xFFFFFFFF
        s.add(v if v <= top else v - (1 << 32))
    s.update(extra)
    return sorted(v for v in s if 0 <= v <= top)


def rng_for(op, q):
    return random.Random(f"{op}/{q}")


def planes(rows):
    """list of operand tuples -> uint64[n_in][count]"""
    return np.array(rows, dtype=np.uint64).T.copy() if rows else np.zeros((0, 0), dtype=np.uint64)


def dbl(v):
    """bit pattern of the double that holds the integer v exactly (|v| <= 2^53)"""
    assert abs(v) <= 1 << 53
    return int(np.array(float(v), dtype=np.float64).view(np.uint64))


def mac_cols(prods):
    c0 = c1 = c2 = 0
    for a, b in prods:
        a0, a1, b0, b1 = a & 0x3FFFFFFF, a >> 30, b & 0x3FFFFFFF, b >> 30
        c0, c1, c2 = c0 + a0 * b0, c1 + a0 * b1 + a1 * b0, c2 + a1 * b1
    return c0, c1, c2


def mac_cols4(prods):
    c0 = c1a = c1b = c2 = 0
    for a, b in prods:
        a0, a1, b0, b1 = a & 0x3FFFFFFF, a >> 30, b & 0x3FFFFFFF, b >> 30
        c0, c1a, c1b, c2 = c0 + a0 * b0, c1a + a0 * b1, c1b + a1 * b0, c2 + a1 * b1
    return c0, c1a, c1b, c2


def column_products(q, terms, rnd, n):
    """lists of `terms` products (a < 2^60, b < q): every column of maximal products first, then edge factors, then draws"""
    amax, bmax = (1 << 60) - 1, q - 1
    ea, eb = edge_set(q, amax), edge_set(q, bmax)
    out = [[(amax, bmax)] * terms]
    for a, b in itertools.product(ea, eb):
        for t in (terms, 1):
            out.append([(a, b)] * t)
    for a, b in itertools.product(ea[-3:], eb[-3:]):  # one edge product next to maximal ones
        out.append([(amax, bmax)] * (terms - 1) + [(a, b)])
    for _ in range(n):
        t = rnd.randint(1, terms)
        out.append([(rnd.choice(ea) if rnd.random() < 0.2 else rnd.randrange(amax + 1),
                     rnd.choice(eb) if rnd.random() < 0.2 else rnd.randrange(q)) for _ in range(t)])
    return out


def vector_patterns(lo, hi, n, rnd):
    """whole-vector patterns over the closed range [lo, hi] for the n values of a round"""
    pats = [[hi] * n, [lo] * n, [hi if i % 2 else lo for i in range(n)], [lo if i % 2 else hi for i in range(n)],
            [hi - 1] * n, [0] * n, [1] * n, [hi if i < n // 2 else lo for i in range(n)],
            [lo if i < n // 2 else hi for i in range(n)]]
    for hot in (0, n // 2, n - 1):
        pats.append([hi if i == hot else 0 for i in range(n)])
    pats.append([rnd.choice((lo, hi)) for _ in range(n)])
    return pats


def round_cases(q, lo, hi, rnd, conv=lambda v: v):
    wp = [[q - 1] * 15, [1] * 15, [0] * 15, [q // 2] * 15, [rnd.randrange(q) for _ in range(15)],
          [(q - 1) if i % 2 else 1 for i in range(15)]]
    rows = [[conv(v) for v in x] + w for x in vector_patterns(lo, hi, 16, rnd) for w in wp]
    for _ in range(N_ROUND):
        rows.append([conv(rnd.randint(lo, hi)) for _ in range(16)] + [rnd.randrange(q) for _ in range(15)])
    return rows


def signed_edges(q, top):
    """integer-valued doubles of magnitude <= top: the edge set and its negation"""
    e = edge_set(q, top)
    return sorted(set(e) | {-v for v in e})


def tie_pairs(q, ymax, rnd, n, wmax=None):
    """(y, w) with y w = (q +- 1) / 2 (mod q): y w / q sits next to a half-integer.  |y| from 1 to ymax across the
    magnitudes; w < q made through y^-1 (q prime)."""
    out = []
    bits = ymax.bit_length()
    while len(out) < n:
        b = rnd.randint(1, bits)
        y = min(ymax, rnd.randrange(1 << (b - 1), 1 << b))
        if y % q == 0:
            continue
        half = (q + rnd.choice((1, -1))) // 2
        w = half * pow(y, -1, q) % q
        out.append((rnd.choice((1, -1)) * y, w))
    return out


@functools.lru_cache(maxsize=None)
def cases(op, q):
    """operand planes uint64[n_in][count] of op under q (deterministic)"""
    rnd = rng_for(op, q)
    k = q.bit_length()
    U = 1 << k
    rows = []
    R = N_RANDOM if op in INT_OPS or op in PM_OPS else N_RANDOM // 2  # (every fp64 rounding is modelled with fractions)
    if op == "csub":  # x, m < 2^63; the library subtracts q, 2q and 4q
        top = (1 << 63) - 1
        for m in (q, 2 * q, 4 * q):
            xs = edge_set(q, top, (m - 1, m, m + 1, 2 * m - 1, 2 * m))
            rows += [(x, m) for x in xs]
            rows += [(rnd.randrange(top + 1), m) for _ in range(R // 4)] + [(rnd.randrange(2 * m), m) for _ in range(R // 4)]
        rows += [(x, m) for x in edge_set(q, top) for m in edge_set(q, top) if m]
    elif op in ("add_mod", "sub_mod", "mul_mod"):
        e = edge_set(q, q - 1, (q - 2, q // 2, q // 2 + 1))
        rows = list(itertools.product(e, e)) + [(rnd.randrange(q), rnd.randrange(q)) for _ in range(R)]
    elif op in ("shoup_lazy", "shoup_mul"):  # any 64-bit a
        ea, ew = edge_set(q, M64, (8 * q - 1, 1 << 63, (1 << 63) - 1)), edge_set(q, q - 1, (q - 2, q // 2))
        rows = list(itertools.product(ea, ew)) + [(rnd.randrange(1 << 64), rnd.randrange(q)) for _ in range(R)]
        rows += [(rnd.randrange(2 * q), rnd.randrange(q)) for _ in range(R // 2)]
    elif op in ("barrett_reduce128", "reduce_wide", "pm_reduce128"):
        top = (1 << {"barrett_reduce128": k + 62, "reduce_wide": 124, "pm_reduce128": 2 * k + 6}[op]) - 1
        ex = edge_set(q, top, ((q - 1) ** 2, (1 << 64) - 1, 1 << 64, (q << 64) - 1, q << 64, 6 * (8 * U - 1) * (q - 1),
                               4 * ((1 << 60) - 1) * (q - 1), ((top >> 64) << 64) | 1, (top >> 64) << 64))
        xs = ex + [rnd.randrange(top + 1) for _ in range(R)] + [rnd.randrange(q * q) for _ in range(R // 2)]
        # low words that make the folding multiply-add carry, under every high word edge
        xs += [(h << 64) | (M64 - rnd.randrange(1 << 16)) for h in edge_set(q, top >> 64) for _ in range(8)]
        xs += [rnd.randrange(top >> 64) << 64 | (M64 - rnd.randrange(1 << 32)) for _ in range(R // 4)]
        # multiples of q (and the words behind them) at the top of the domain: where the quotient estimate loses most
        xs += [(top // q - rnd.randrange(min(1 << 40, top // q))) * q + rnd.choice((0, 1, 2)) for _ in range(R // 4)]
        rows = [(x >> 64, x & M64) for x in xs if x <= top]
    elif op == "reduce_word":
        rows = [(x,) for x in edge_set(q, M64, ((1 << 63) - 1, 1 << 63, q * (M64 // q), q * (M64 // q) - 1))]
        rows += [(rnd.randrange(1 << 64),) for _ in range(R)]
    elif op in ("reduce_cols_lazy", "reduce_cols", "pm_reduce_cols"):
        rows = [mac_cols(p) for p in column_products(q, 4, rnd, R)]
        # four nearly maximal products: the top of the Barrett window, with the fractions its floors drop spread out
        rows += [mac_cols([((1 << 60) - 1 - rnd.randrange(1 << 40), q - 1 - rnd.randrange(min(q, 1 << 40))) for _ in range(4)])
                 for _ in range(R // 4)]
    elif op == "reduce_cols4":
        rows = [mac_cols4(p) for p in column_products(q, 8, rnd, R)]
    elif op in ("mac128", "mac128_split"):  # a < 2^63 (a lazy word), b < 2^60 (a residue), the sum stays below 2^128
        ea = edge_set(q, (1 << 63) - 1, (8 * U - 1,))
        eb = edge_set(q, (1 << 60) - 1)
        full = (1 << 128) - 1

        def accs(p):
            """accumulators for the product p: small ones, the ones that bring the sum to 2^128 - 1 and next to it, the
            low words that make the low multiply-add carry (or just not), full words under the largest high word"""
            room = full - p
            lowc = (-p) & M64
            cand = [0, 1, M64, 1 << 64, room, room - 1, (room >> 64) << 64, ((room >> 64) << 64) | M64,
                    (((room >> 64) - 1) << 64) | M64, lowc, lowc - 1, ((room >> 65) << 64) | lowc, M64 - (p & 0xFFFFFFFF)]
            return [v for v in cand if 0 <= v <= room]
        for a, b in itertools.product(ea, eb):
            rows += [(s >> 64, s & M64, a, b) for s in accs(a * b)]
        for _ in range(R):
            a, b = rnd.randrange(1 << 63), rnd.randrange(1 << 60)
            s = rnd.choice(accs(a * b)) if rnd.random() < 0.3 else rnd.randrange(full - a * b + 1)
            rows.append((s >> 64, s & M64, a, b))
    elif op in ("ct_butterfly_c4", "ct_butterfly_nc", "gs_butterfly"):
        xtop = {"ct_butterfly_c4": 8 * q - 1, "ct_butterfly_nc": 6 * q - 1, "gs_butterfly": 2 * q - 1}[op]
        ytop = 2 * q - 1 if op == "gs_butterfly" else 8 * q - 1
        ex, ey = edge_set(q, xtop, (4 * q - 1, 4 * q)), edge_set(q, ytop, (4 * q - 1, 4 * q))
        ew = edge_set(q, q - 1, (q - 2, q // 2))
        rows = list(itertools.product(ex, ey, ew))
        rows += [(rnd.randrange(xtop + 1), rnd.randrange(ytop + 1), rnd.randrange(q)) for _ in range(R)]
    elif op == "canon8":
        rows = [(v,) for v in edge_set(q, 8 * q - 1, [j * q + d for j in range(1, 8) for d in (-1, 0, 1)])]
        rows += [(rnd.randrange(8 * q),) for _ in range(R)]
    elif op in ("radix_forward4", "radix_inverse4"):
        rows = round_cases(q, 0, (8 if op == "radix_forward4" else 2) * q - 1, rnd)
    elif op == "pm_fold":
        rows = [(x,) for x in edge_set(q, M64, (U - 1, U, 8 * U - 1, 8 * U, (1 << 63) - 1, 1 << 63))]
        rows += [(rnd.randrange(1 << 64),) for _ in range(R)]
    elif op == "pm_lazy":  # a < 8U
        ea = edge_set(q, 8 * U - 1, (U - 1, U, ((8 * U - 1) >> 32) << 32))
        ew = edge_set(q, q - 1, (q - 2, q // 2, q - 0xFFFFFFFF))
        rows = list(itertools.product(ea, ew)) + [(rnd.randrange(8 * U), rnd.randrange(q)) for _ in range(2 * R)]
    elif op in ("ct_butterfly_pm_f", "ct_butterfly_pm_n", "gs_butterfly_pm"):
        # f: x, y < 8U (round inputs); n: x < 4.001U (an f output), y < 8U; inverse: x, y < 2.375U
        xtop = {"ct_butterfly_pm_f": 8 * U, "ct_butterfly_pm_n": 4001 * U // 1000, "gs_butterfly_pm": 19 * U // 8}[op] - 1
        ytop = 19 * U // 8 - 1 if op == "gs_butterfly_pm" else 8 * U - 1
        ex, ey = edge_set(q, xtop, (U - 1, U)), edge_set(q, ytop, (U - 1, U))
        ew = edge_set(q, q - 1, (q - 2, q // 2))
        rows = list(itertools.product(ex, ey, ew))
        rows += [(rnd.randrange(xtop + 1), rnd.randrange(ytop + 1), rnd.randrange(q)) for _ in range(R)]
    elif op in ("radix_forward_pm4", "radix_inverse_pm4"):
        rows = round_cases(q, 0, (8 * U if op == "radix_forward_pm4" else 19 * U // 8) - 1, rnd)
    # ---- fp64 class: values are integer-valued doubles
    elif op == "fp_mulmod":  # |y| <= 2^52
        ey, ew = signed_edges(q, 1 << 52), edge_set(q, q - 1, (q - 2, q // 2, q // 2 + 1))
        rows = list(itertools.product(ey, ew))
        rows += [(rnd.randint(-(1 << 52), 1 << 52), rnd.randrange(q)) for _ in range(R)]
        rows += [(rnd.randint(-3 * q, 3 * q), rnd.randrange(q)) for _ in range(R // 2)]
        if is_prime(q):
            rows += tie_pairs(q, 1 << 52, rnd, R)
        rows = [(dbl(y), w) for y, w in rows]
    elif op in ("fp_reduce", "fp_to_canonical"):  # |x| < 2^53
        top = (1 << 53) - 1
        xs = signed_edges(q, top) + [rnd.randint(-top, top) for _ in range(R)] + [rnd.randint(-4 * q, 4 * q) for _ in range(R // 2)]
        for _ in range(R):  # next to half-integer multiples of q
            t = rnd.randint(-(top // q), top // q - 1)
            xs.append(t * q + (q + rnd.choice((1, -1))) // 2)
        xs += [t * q + d for t in range(-3, 4) for d in (-1, 0, 1)]
        rows = [(dbl(x),) for x in xs if abs(x) <= top]
    elif op == "fp_mulmod_any":  # e in [0, q), |y| <= q (result <= 0.97q); |y| <= 0.51q (result <= 0.75q)
        half = 51 * q // 100
        ey, ee = signed_edges(q, q), edge_set(q, q - 1, (q - 2, q // 2, q // 2 + 1))
        rows = list(itertools.product(sorted(set(ey) | {half, -half, half - 1, 1 - half}), ee))
        rows += [(rnd.randint(-q, q), rnd.randrange(q)) for _ in range(R)]
        rows += [(rnd.randint(-half, half), rnd.randrange(q)) for _ in range(R)]
        if is_prime(q):
            rows += tie_pairs(q, q - 1, rnd, R // 2) + tie_pairs(q, half, rnd, R // 2)
        rows = [(dbl(y), dbl(e)) for y, e in rows]
    elif op == "u52_to_double":
        rows = [(v,) for v in edge_set(q, (1 << 52) - 1)] + [(rnd.randrange(1 << 52),) for _ in range(R)]
    elif op == "split30_d":  # an integer below 2^52 (a canonical residue of any fp64-class limb) held in a double
        rows = [(dbl(v),) for v in edge_set(q, (1 << 52) - 1, ((1 << 30) - 1, 1 << 30))]  # the helper's domain: below 2^52
        rows += [(dbl(rnd.randrange(q)),) for _ in range(R // 2)] + [(dbl(rnd.randrange(1 << 52)),) for _ in range(R // 2)]
    elif op in ("ct_butterfly_fp", "ct_butterfly_fp_nr", "gs_butterfly_fp"):
        # forward, re-centring stage: inputs up to 3.1q.  Forward, plain stage: its inputs are the outputs of a re-centring
        # one, X -> 1.01q + 0.31 X, i.e. up to 1.971q (from there 1.31 X + 0.5q stays below 3.1q).  Inverse: 1.33q
        top = {"ct_butterfly_fp": 31 * q // 10, "ct_butterfly_fp_nr": 1971 * q // 1000, "gs_butterfly_fp": 133 * q // 100}[op]
        ev, ew = signed_edges(q, top), edge_set(q, q - 1, (q - 2, q // 2))
        rows = list(itertools.product(ev, ev, ew))
        rows += [(rnd.randint(-top, top), rnd.randint(-top, top), rnd.randrange(q)) for _ in range(R)]
        if is_prime(q):
            for y, w in tie_pairs(q, top if op != "gs_butterfly_fp" else 2 * top, rnd, R // 2):
                if op == "gs_butterfly_fp":  # the product operand is d = x - y, |d| <= 2.66q: split it over x and y
                    d = y
                    x = d - d // 2
                    rows.append((x, x - d, w))
                else:
                    rows.append((rnd.randint(-top, top), y, w))
        assert all(abs(x) <= top and abs(y) <= top for x, y, w in rows)
        rows = [(dbl(x), dbl(y), w) for x, y, w in rows]
    elif op in ("radix_forward_fp4", "radix_inverse_fp4"):
        top = 31 * q // 10 if op == "radix_forward_fp4" else 133 * q // 100
        rows = round_cases(q, -top, top, rnd, conv=dbl)
    else:
        raise KeyError(op)
    x = planes(rows)
    assert x.shape[0] == ARITH_OPS[op][1], (op, x.shape)
    return x


# ---- Python models and checks ----------------------------------------------------------------------------------------------
def m_csub(x, m):
    return x - m if x >= m else x


def forward_round_exact(x, w, q):
    x = list(x)
    for s in range(4):
        dist = 16 >> (s + 1)
        for p in range(8):
            g = p // dist
            k0 = g * 2 * dist + p % dist
            v = x[k0 + dist] * w[(1 << s) - 1 + g]
            x[k0], x[k0 + dist] = (x[k0] + v) % q, (x[k0] - v) % q
    return x


def inverse_round_exact(x, w, q):
    x = list(x)
    for s in range(3, -1, -1):
        dist = 16 >> (s + 1)
        for p in range(8):
            g = p // dist
            k0 = g * 2 * dist + p % dist
            a, b = x[k0], x[k0 + dist]
            x[k0], x[k0 + dist] = (a + b) % q, (a - b) * w[(1 << s) - 1 + g] % q
    return x


class Cover(dict):
    """tuples on each side of a carry / select of a device form, counted from the Python model"""

    def hit(self, name, side):
        self[name, bool(side)] = self.get((name, bool(side)), 0) + 1

    def require(self, *names):
        for n in names:
            assert self.get((n, True), 0) > 0 and self.get((n, False), 0) > 0, (n, self.get((n, True), 0), self.get((n, False), 0))


def barrett_tail(op, q, y, lo, cov):
    """model of the end of barrett_reduce128 for the window y and the low word lo: the uncorrected remainder, with its two
    conditional subtractions counted"""
    k = q.bit_length()
    r = (lo - ((y * ((1 << (62 + k)) // q)) >> 64) * q) & M64
    assert r < 5 * q // 2
    cov.hit(op + " csub 2q", r >= 2 * q)
    cov.hit(op + " csub q", m_csub(r, 2 * q) >= q)
    return r


def m_reduce_wide(op, q, hi, lo, cov):
    k = q.bit_length()
    f = hi * ((1 << 64) % q) + lo  # the fold of the high word: below 2^(k+60) + 2^64
    assert f < (1 << (k + 60)) + (1 << 64)
    return barrett_tail(op, q, f >> (k - 2), f & M64, cov)


def check_int(op, q, x, out, cov):
    """host or device words of an integer / pseudo-Mersenne op against Python integers"""
    k = q.bit_length()
    U = 1 << k
    n = x.shape[1]
    X = [[int(v) for v in row] for row in x]
    O = [[int(v) for v in row] for row in out]
    ctx = lambda i: (op, q, [r[i] for r in X], [r[i] for r in O])
    if op == "csub":
        for i in range(n):
            a, m = X[0][i], X[1][i]
            assert O[0][i] == m_csub(a, m), ctx(i)
            cov.hit("csub", a >= m)
            cov.hit("csub at equality", a == m)
    elif op in ("add_mod", "sub_mod", "mul_mod"):
        f = {"add_mod": lambda a, b: (a + b) % q, "sub_mod": lambda a, b: (a - b) % q, "mul_mod": lambda a, b: a * b % q}[op]
        for i in range(n):
            assert O[0][i] == f(X[0][i], X[1][i]), ctx(i)
            if op == "mul_mod":
                p = X[0][i] * X[1][i]
                barrett_tail(op, q, p >> (k - 2), p & M64, cov)
    elif op in ("shoup_lazy", "shoup_mul"):
        for i in range(n):
            a, w = X[0][i], X[1][i]
            wp = (w << 64) // q
            lazy = (a * w - ((a * wp) >> 64) * q) & M64  # the word Shoup's estimate leaves: a w - floor(a wp / 2^64) q
            assert lazy < 2 * q and lazy % q == a * w % q
            assert O[0][i] == (lazy if op == "shoup_lazy" else a * w % q), ctx(i)
            cov.hit("shoup csub", lazy >= q)
    elif op in ("barrett_reduce128", "reduce_wide", "pm_reduce128"):
        c64 = ((1 << k) - q) << (64 - k)
        for i in range(n):
            hi, lo = X[0][i], X[1][i]
            assert O[0][i] == ((hi << 64) | lo) % q, ctx(i)
            if op == "barrett_reduce128":
                barrett_tail(op, q, ((hi << 64) | lo) >> (k - 2), lo, cov)
            elif op == "reduce_wide":
                m_reduce_wide(op, q, hi, lo, cov)
            if op == "pm_reduce128":
                m = (hi & 0xFFFFFFFF) * c64 + lo
                cov.hit("pm_reduce128 cy", m >> 64)
                nn = (hi >> 32) * c64 + ((m & M64) >> 32) + ((m >> 64) << 32)
                r = (nn >> (k - 32)) * (U - q) + (((nn & ((1 << (k - 32)) - 1)) << 32) | (m & 0xFFFFFFFF))
                assert r < (1 << 63) and r % q == ((hi << 64) | lo) % q
                cov.hit("pm_reduce128 csub", r >= q)
    elif op == "reduce_word":
        for i in range(n):
            assert O[0][i] == X[0][i] % q, ctx(i)
            barrett_tail(op, q, X[0][i] >> (k - 2), X[0][i], cov)
    elif op in ("reduce_cols_lazy", "reduce_cols", "pm_reduce_cols"):
        for i in range(n):
            S = X[0][i] + (X[1][i] << 30) + (X[2][i] << 60)
            r = O[0][i]
            assert r % q == S % q, ctx(i)
            if op != "pm_reduce_cols":  # the window as the code assembles it from the three columns
                sh = k - 2
                y = (X[0][i] >> sh) + (X[1][i] << (30 - sh) if sh <= 30 else X[1][i] >> (sh - 30)) + (X[2][i] << (60 - sh))
                assert y < 1 << 64
                lazy = barrett_tail(op, q, y, S & M64, cov)
            if op == "reduce_cols":
                assert r < q, ctx(i)
            elif op == "reduce_cols_lazy":
                assert r < 4 * q and r == lazy, ctx(i)
                cov.hit("reduce_cols_lazy e1 >= 0", 32 - k >= 0)
            else:
                assert 10 * r < 21 * U, ctx(i)
    elif op == "reduce_cols4":
        for i in range(n):
            S = X[0][i] + ((X[1][i] + X[2][i]) << 30) + (X[3][i] << 60)
            assert O[0][i] == S % q, ctx(i)
            m_reduce_wide(op, q, S >> 64, S & M64, cov)
    elif op in ("mac128", "mac128_split"):
        for i in range(n):
            hi, lo, a, b = (X[j][i] for j in range(4))
            s = ((hi << 64) | lo) + a * b
            assert s < 1 << 128
            assert (O[0][i], O[1][i]) == (s >> 64, s & M64), ctx(i)
            if op == "mac128":  # the device form's carries
                a0, a1, b0, b1 = a & 0xFFFFFFFF, a >> 32, b & 0xFFFFFFFF, b >> 32
                r0 = a0 * b0 + lo
                c0 = r0 >> 64
                r2 = a1 * b0 + a0 * b1 + ((r0 & M64) >> 32)
                assert r2 < 1 << 64
                r3 = (a1 * b1 + hi) & M64
                cov.hit("mac128 c0", c0)
                cov.hit("mac128 carry between the two adds", ((r3 & 0xFFFFFFFF) + (r2 >> 32) + c0) >> 32)
    elif op in ("ct_butterfly_c4", "ct_butterfly_nc", "gs_butterfly"):
        for i in range(n):
            a, b, w = X[0][i], X[1][i], X[2][i]
            xo, yo = O[0][i], O[1][i]
            if op == "gs_butterfly":
                assert xo % q == (a + b) % q and yo % q == (a - b) * w % q and xo < 2 * q and yo < 2 * q, ctx(i)
                cov.hit("gs_butterfly csub", a + b >= 2 * q)
            else:
                lim = 6 * q if op == "ct_butterfly_c4" else 8 * q
                assert xo % q == (a + b * w) % q and yo % q == (a - b * w) % q and xo < lim and yo < lim, ctx(i)
                if op == "ct_butterfly_c4":
                    cov.hit("ct_butterfly_c4 csub", a >= 4 * q)
    elif op == "canon8":
        for i in range(n):
            v = X[0][i]
            assert O[0][i] == v % q, ctx(i)
            v1 = m_csub(v, 4 * q)
            v2 = m_csub(v1, 2 * q)
            cov.hit("canon8 csub 4q", v >= 4 * q)
            cov.hit("canon8 csub 2q", v1 >= 2 * q)
            cov.hit("canon8 csub q", v2 >= q)
    elif op in ("radix_forward4", "radix_inverse4", "radix_forward_pm4", "radix_inverse_pm4"):
        fwd = "forward" in op
        lim = {"radix_forward4": 8 * q, "radix_inverse4": 2 * q, "radix_forward_pm4": 7001 * U // 1000,
               "radix_inverse_pm4": 19 * U // 8}[op]
        for i in range(n):
            xs, ws = [X[j][i] for j in range(16)], [X[16 + j][i] for j in range(15)]
            want = (forward_round_exact if fwd else inverse_round_exact)(xs, ws, q)
            got = [O[j][i] for j in range(16)]
            assert [g % q for g in got] == want and max(got) < lim, ctx(i)
    elif op == "pm_fold":
        for i in range(n):
            assert O[0][i] % q == X[0][i] % q and O[0][i] < U + (1 << 30), ctx(i)
    elif op == "pm_lazy":
        t = 63 - k
        for i in range(n):
            a, w = X[0][i], X[1][i]
            r = O[0][i]
            assert r % q == a * w % q and 8 * r < 19 * U, ctx(i)
            wt, wxt = w << t, ((w << 32) % q) << t
            low = (a & 0xFFFFFFFF) * (wt & 0xFFFFFFFF) + (a >> 32) * (wxt & 0xFFFFFFFF)
            assert low < 1 << 65
            cov.hit("pm_lazy low-sum carry", low >> 64)
    elif op in ("ct_butterfly_pm_f", "ct_butterfly_pm_n", "gs_butterfly_pm"):
        for i in range(n):
            a, b, w = X[0][i], X[1][i], X[2][i]
            xo, yo = O[0][i], O[1][i]
            if op == "gs_butterfly_pm":
                assert xo % q == (a + b) % q and yo % q == (a - b) * w % q, ctx(i)
                assert 1000 * xo < 1001 * U and 8 * yo < 19 * U, ctx(i)
            else:
                assert xo % q == (a + b * w) % q and yo % q == (a - b * w) % q, ctx(i)
                lx, ly = (3376, 4001) if op == "ct_butterfly_pm_f" else (6376, 7001)
                assert 1000 * xo < lx * U and 1000 * yo < ly * U, ctx(i)
    else:
        raise KeyError(op)


def as_ints(bits, what):
    """integer-valued doubles (bit patterns) -> Python ints"""
    d = bits.view(np.float64)
    assert np.all(np.isfinite(d)) and np.all(d == np.rint(d)) and np.all(np.abs(d) <= float(1 << 53)), what
    return [int(v) for v in d]


# ---- the fp64 forms, rounding by rounding (fractions decide every rounding) ---------------------------------------------------
def rn_bits(fr, bits):
    """fr rounded to `bits` significant bits, ties to even"""
    if fr == 0:
        return fr
    e = abs(fr.numerator).bit_length() - fr.denominator.bit_length()  # 2^(e-1) < |fr| < 2^(e+1)
    if abs(fr) < Fraction(2) ** e:
        e -= 1
    scale = Fraction(2) ** (bits - 1 - e)
    return round(fr * scale) / scale


def table_quotient(a, b):
    """(double)((long double) a / (long double) b) as the table code computes it: the quotient is rounded to the 64-bit
    mantissa of the x86 extended format first, then to a double"""
    return float(rn_bits(Fraction(a, b), 64))


def f_mul(a, b):
    return float(Fraction(a) * Fraction(b))  # Fraction -> float is correctly rounded


def f_fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def m_fp_mulmod(y, w, wq, q):
    h = f_mul(y, w)
    l = f_fma(y, w, -h)
    b = float(round(f_mul(y, wq)))  # rint: ties to even, as Python's round
    return f_fma(-b, q, h) + l


def m_fp_reduce(x, q, qinv):
    return f_fma(-float(round(f_mul(x, qinv))), q, x)


def m_fp_mulmod_any(y, e, q, qinv):
    h = f_mul(y, e)
    l = f_fma(y, e, -h)
    b = float(round(f_mul(h, qinv)))
    return f_fma(-b, q, h) + l


def half_integer(v):
    return v != round(v) and 2 * v == round(2 * v)


def check_fp(op, q, x, out, margins, cov=None):
    """device outputs of an fp64 op: integer-valued, congruent, within the bound the code's comment states -- and, for the
    primitives and the butterflies, the very double the sequence of IEEE operations in modarith.hpp gives (m_fp_*): the
    bounds alone do not tell rint from floor(x + 0.5), nor which rounded product the quotient is estimated from"""
    n = x.shape[1]
    cov = Cover() if cov is None else cov
    qd, qinv = float(q), table_quotient(1, q)
    worst = Fraction(0)
    bound_txt = ""

    def within(v, bound, i):  # bound: Fraction, in units of q
        nonlocal worst
        assert abs(v) <= bound * q, (op, q, [int(r[i]) for r in x], v, float(Fraction(abs(v), q)), float(bound))
        worst = max(worst, Fraction(abs(v), q))

    if op == "fp_mulmod":
        y, w, o = as_ints(x[0], op), [int(v) for v in x[1]], as_ints(out[0], op)
        bound_txt = "0.5 + 1.0001 |y| / 2^52"
        for i in range(n):
            assert (o[i] - y[i] * w[i]) % q == 0, (op, q, y[i], w[i], o[i])
            within(o[i], Fraction(1, 2) + Fraction(10001, 10000) * Fraction(abs(y[i]), 1 << 52), i)
            wq = table_quotient(w[i], q)
            assert o[i] == m_fp_mulmod(float(y[i]), float(w[i]), wq, qd), (op, q, y[i], w[i], o[i])
            est = f_mul(float(y[i]), wq)
            if abs(est) < 1 << 50:  # (from 2^51 on every double is a multiple of 1/2: no sign of a constructed tie)
                cov.hit("fp_mulmod estimate at a half-integer", half_integer(est))
    elif op == "fp_reduce":
        v, o = as_ints(x[0], op), as_ints(out[0], op)
        bound_txt = "0.51"
        for i in range(n):
            assert (o[i] - v[i]) % q == 0, (op, q, v[i], o[i])
            within(o[i], Fraction(51, 100), i)
            assert o[i] == m_fp_reduce(float(v[i]), qd, qinv), (op, q, v[i], o[i])
            m = f_mul(float(v[i]), qinv)
            cov.hit("fp_reduce estimate at a half-integer", half_integer(m))
            if half_integer(m):  # rint and floor(x + 0.5) part here: ties to even against ties upwards
                cov.hit("fp_reduce tie rounded down", round(m) < m)
    elif op == "fp_to_canonical":
        v = as_ints(x[0], op)
        for i in range(n):
            assert int(out[0][i]) == v[i] % q, (op, q, v[i], int(out[0][i]))
        return
    elif op == "fp_mulmod_any":
        y, e, o = as_ints(x[0], op), as_ints(x[1], op), as_ints(out[0], op)
        bound_txt = "0.97 (|y| <= q), 0.75 (|y| <= 0.51q)"
        for i in range(n):
            assert (o[i] - y[i] * e[i]) % q == 0, (op, q, y[i], e[i], o[i])
            within(o[i], Fraction(75, 100) if 100 * abs(y[i]) <= 51 * q else Fraction(97, 100), i)
            assert o[i] == m_fp_mulmod_any(float(y[i]), float(e[i]), qd, qinv), (op, q, y[i], e[i], o[i])
            # estimating from y * RN(e / q) instead of RN(y e) / q would land on the other side of a half-integer here
            h = f_mul(float(y[i]), float(e[i]))
            cov.hit("fp_mulmod_any estimate depends on which product is rounded",
                    round(f_mul(h, qinv)) != round(f_mul(float(y[i]), f_mul(float(e[i]), qinv))))
    elif op == "u52_to_double":
        assert as_ints(out[0], op) == [int(v) for v in x[0]]
        return
    elif op == "split30_d":
        v = as_ints(x[0], op)
        assert [int(a) for a in out[0]] == [a & 0x3FFFFFFF for a in v] and [int(a) for a in out[1]] == [a >> 30 for a in v]
        return
    elif op in ("ct_butterfly_fp", "ct_butterfly_fp_nr", "gs_butterfly_fp"):
        a, b, w = as_ints(x[0], op), as_ints(x[1], op), [int(v) for v in x[2]]
        xo, yo = as_ints(out[0], op), as_ints(out[1], op)
        half, eps = Fraction(1, 2), Fraction(10001, 10000)
        for i in range(n):
            fa, fb, fw, wq = float(a[i]), float(b[i]), float(w[i]), table_quotient(w[i], q)
            if op == "gs_butterfly_fp":
                want = (m_fp_reduce(fa + fb, qd, qinv), m_fp_mulmod(fa - fb, fw, wq, qd))
            else:
                mv = m_fp_mulmod(fb, fw, wq, qd)
                mu = m_fp_reduce(fa, qd, qinv) if op == "ct_butterfly_fp" else fa
                want = (mu + mv, mu - mv)
            assert (xo[i], yo[i]) == want, (op, q, a[i], b[i], w[i], xo[i], yo[i], want)
            if op == "gs_butterfly_fp":
                assert (xo[i] - a[i] - b[i]) % q == 0 and (yo[i] - (a[i] - b[i]) * w[i]) % q == 0, (op, q, a[i], b[i], w[i])
                within(xo[i], Fraction(51, 100), i)
                within(yo[i], half + eps * Fraction(abs(a[i] - b[i]), 1 << 52), i)
                bound_txt = "x': 0.51, y': 0.5 + 1.0001 |x - y| / 2^52"
            else:
                assert (xo[i] - a[i] - b[i] * w[i]) % q == 0 and (yo[i] - a[i] + b[i] * w[i]) % q == 0, (op, q, a[i], b[i], w[i])
                u = Fraction(51, 100) if op == "ct_butterfly_fp" else Fraction(abs(a[i]), q)
                v = half + eps * Fraction(abs(b[i]), 1 << 52)
                within(xo[i], min(u + v, Fraction(31, 10)), i)  # and never above the next stage's input range
                within(yo[i], min(u + v, Fraction(31, 10)), i)
                bound_txt = "min(3.1, |u| + 0.5 + 1.0001 |y| / 2^52), |u| <= 0.51 re-centred, |x| as is"
    elif op in ("radix_forward_fp4", "radix_inverse_fp4"):
        fwd = op == "radix_forward_fp4"
        bound = Fraction(31, 10) if fwd else Fraction(133, 100)
        bound_txt = "3.1 from inputs <= 3.1" if fwd else "1.33 from inputs <= 1.33"
        xs = [as_ints(x[j], op) for j in range(16)]
        ws = [[int(v) for v in x[16 + j]] for j in range(15)]
        os_ = [as_ints(out[j], op) for j in range(16)]
        for i in range(n):
            want = (forward_round_exact if fwd else inverse_round_exact)([r[i] for r in xs], [r[i] for r in ws], q)
            assert [r[i] % q for r in os_] == want, (op, q, i)
            for r in os_:
                within(r[i], bound, i)
    else:
        raise KeyError(op)
    margins.append((op, q, float(worst), bound_txt))


INT_OPS = ["csub", "add_mod", "sub_mod", "shoup_lazy", "shoup_mul", "mul_mod", "barrett_reduce128", "reduce_wide",
           "reduce_word", "reduce_cols_lazy", "reduce_cols", "reduce_cols4", "mac128", "mac128_split", "ct_butterfly_c4",
           "ct_butterfly_nc", "gs_butterfly", "canon8", "radix_forward4", "radix_inverse4"]
PM_OPS = ["pm_fold", "pm_lazy", "pm_reduce128", "pm_reduce_cols", "ct_butterfly_pm_f", "ct_butterfly_pm_n",
          "gs_butterfly_pm", "radix_forward_pm4", "radix_inverse_pm4"]
FP_OPS = ["fp_mulmod", "fp_reduce", "fp_to_canonical", "fp_mulmod_any", "u52_to_double", "split30_d", "ct_butterfly_fp",
          "ct_butterfly_fp_nr", "gs_butterfly_fp", "radix_forward_fp4", "radix_inverse_fp4"]
# fpodd is not prime: the ops that divide (a twiddle's inverse in the tie construction) skip the ties there, nothing else
INT_COVER = ["csub", "csub at equality", "shoup csub", "mac128 c0", "mac128 carry between the two adds",
             "gs_butterfly csub", "ct_butterfly_c4 csub", "canon8 csub 4q", "canon8 csub 2q", "canon8 csub q"]
PM_COVER = ["pm_lazy low-sum carry", "pm_reduce128 cy", "pm_reduce128 csub"]
BARRETT_OPS = ["barrett_reduce128", "mul_mod", "reduce_word", "reduce_wide", "reduce_cols_lazy", "reduce_cols", "reduce_cols4"]


def require_barrett_selects(cov, name):
    """The two conditional subtractions at the end of Barrett's reduction, in every op that ends in them.  The one of q is
    taken and not taken everywhere.  The one of 2q: where barrett_sup proves that the estimate is never 2 short, the model
    must never have seen it taken (the side does not exist for that op and modulus); at b60 the inputs of
    barrett_reduce128 and reduce_cols / reduce_cols_lazy must take it and leave it."""
    q = moduli()[name]
    for op in BARRETT_OPS:
        cov.require(op + " csub q")
        if barrett_sup(op, q) <= 1:
            assert cov.get((op + " csub 2q", True), 0) == 0 and cov.get((op + " csub 2q", False), 0) > 0, (op, name)
    if name == "b60":
        cov.require("barrett_reduce128 csub 2q", "reduce_cols csub 2q", "reduce_cols_lazy csub 2q")
    else:  # every other modulus of the list is next to a power of two: the side is proved away for the plain reduction
        assert barrett_sup("barrett_reduce128", q) <= 1, name


def fp_cover(q):
    """selects of the fp64 forms that the inputs of modulus q must reach on both sides (counted from the model)"""
    names = ["fp_mulmod estimate at a half-integer", "fp_reduce estimate at a half-integer", "fp_reduce tie rounded down"]
    # the two ways to estimate fp_mulmod_any's quotient differ by about q 2^-52 units; a product made to sit 1 / (2q)
    # from a half-integer can fall between them only when q^2 is well above 2^51
    if q * q > 1 << 60:
        names.append("fp_mulmod_any estimate depends on which product is rounded")
    return names


def test_op_lists_cover_the_table():
    assert sorted(INT_OPS + PM_OPS + FP_OPS) == sorted(ARITH_OPS)
    assert [ARITH_OPS[o][0] for o in INT_OPS + PM_OPS + FP_OPS] == list(range(len(ARITH_OPS)))


@functools.lru_cache(maxsize=None)
def _host_ctx():
    from ppqsflhe_amd import Context
    return Context(10, 3, 40, 60, dnum=2, device=-1)


@pytest.fixture(scope="module", autouse=True)
def _one_host_context():
    """the module's only device = -1 context: made on first use, closed when the module is done"""
    yield
    if _host_ctx.cache_info().currsize:
        _host_ctx().close()
        _host_ctx.cache_clear()


@pytest.fixture
def host():
    return _host_ctx()


@functools.lru_cache(maxsize=None)
def _host_words(op, q):
    return _host_ctx().debug_arith(op, q, cases(op, q))


_checked = {}


def host_checked(op, q):
    """host-form words of op under q, checked once against the Python model; the coverage counts of that check"""
    if (op, q) not in _checked:
        cov = Cover()
        out = _host_words(op, q)
        check_int(op, q, cases(op, q), out, cov)
        _checked[op, q] = (out, cov)
    return _checked[op, q]


def class_cover(ops, q):
    total = Cover()
    for op in ops:
        for key, cnt in host_checked(op, q)[1].items():
            total[key] = total.get(key, 0) + cnt
    return total


@pytest.mark.parametrize("name", INT_MODULI)
def test_integer_host_forms(name):
    q = moduli()[name]
    cov = class_cover(INT_OPS, q)
    cov.require(*INT_COVER)
    require_barrett_selects(cov, name)
    # the middle column of reduce_cols_lazy is shifted left for q below 2^32 only: each modulus takes its own side, and
    # test_moduli_have_the_widths_and_forms_the_ops_need holds both kinds in this list
    assert cov.get(("reduce_cols_lazy e1 >= 0", q.bit_length() <= 32), 0) > 0


@pytest.mark.parametrize("name", PM_MODULI)
def test_pseudo_mersenne_host_forms(name):
    q = moduli()[name]
    class_cover(PM_OPS, q).require(*PM_COVER)


def test_fp64_inputs_reach_both_sides_of_the_sign_select():
    """r < 0 in fp_to_canonical, from the model: x mod q clearly above q / 2 gives a negative centred remainder"""
    for name in FP_MODULI:
        q = moduli()[name]
        v = as_ints(cases("fp_to_canonical", q)[0], name)
        assert sum(1 for a in v if a % q > q // 2 + 1) > 0 and sum(1 for a in v if a % q < q // 2) > 0
        # the tie construction: operands whose exact quotient is within 1/q of a half-integer
        if is_prime(q):
            x = cases("fp_mulmod", q)
            y, w = as_ints(x[0], name), [int(a) for a in x[1]]
            ties = [abs(a) for a, b in zip(y, w) if a * b % q in ((q - 1) // 2, (q + 1) // 2)]
            assert len(ties) >= N_RANDOM // 2 and min(ties) < 1 << 8 and max(ties) > 1 << 51


def test_entry_point_refusals_and_noop(host):
    from ppqsflhe_amd import MkckksError
    q = moduli()["q0"]
    L, h = host._L, host._h
    a, b = np.zeros(32, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
    A, B = a.ctypes.data, b.ctypes.data
    add = ARITH_OPS["add_mod"][0]  # two input planes: count 4 reads 8 words, writes 4

    def rc(op, q, pin, pout, count):
        return L.mkckks_debug_arith(h, op, q, pin, pout, count)
    assert rc(add, q, A, B, 4) == 0
    assert rc(len(ARITH_OPS), q, A, B, 4) == -1          # unknown op
    assert rc(0xFFFFFFFF, q, A, B, 4) == -1
    assert rc(add, q + 1, A, B, 4) == -1                 # even
    assert rc(add, (1 << 17) - 1, A, B, 4) == -1         # not above 2^17
    assert rc(add, (1 << 60) + 1, A, B, 4) == -1         # not below 2^60
    assert rc(ARITH_OPS["fp_reduce"][0], FP_LIMIT + 1, A, B, 4) == -1        # fp64 op, q >= 5 * 2^48
    assert rc(ARITH_OPS["pm_fold"][0], moduli()["s54"], A, B, 4) == -1       # not pseudo-Mersenne
    assert rc(ARITH_OPS["pm_fold"][0], moduli()["e20"], A, B, 4) == -1
    assert rc(add, q, A, A + 8, 4) == -1                 # out inside in
    assert rc(add, q, A, A + 56, 4) == -1                # out starts on the last input word
    assert rc(add, q, A + 24, A, 4) == -1                # in starts on the last output word
    assert rc(add, q, A, A + 64, 4) == 0                 # adjacent: out right behind in
    assert rc(add, q, A + 32, A, 4) == 0                 # adjacent: in right behind out
    assert rc(ARITH_OPS["fp_reduce"][0], moduli()["tiny"], A, B, 4) == -2    # device form only
    b[:] = 7
    assert rc(add, q, A, B, 0) == 0 and np.all(b == 7)   # no-op
    assert rc(add, q, None, None, 0) == 0
    w = np.array([[1, 2], [q, 3]], dtype=np.uint64)  # a twiddle plane holds residues
    with pytest.raises(MkckksError) as ei:
        host.debug_arith("shoup_lazy", q, w)
    assert ei.value.code == -1


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    from ppqsflhe_amd import Context
    g = Context(10, 3, 40, 60, dnum=2, device=0)
    yield g
    g.close()


def _device_equals_host(gpu, ops, name):
    q = moduli()[name]
    for op in ops:
        want, _ = host_checked(op, q)
        got = gpu.debug_arith(op, q, cases(op, q))
        bad = np.argwhere(got != want)
        assert bad.size == 0, (op, name, q, [int(v) for v in cases(op, q)[:, bad[0][1]]],
                               [int(v) for v in got[:, bad[0][1]]], [int(v) for v in want[:, bad[0][1]]], len(bad))


@pytest.mark.gpu
@pytest.mark.parametrize("name", INT_MODULI)
def test_integer_device_forms_equal_host_forms(gpu, name):
    """the device words are the host words, which test_integer_host_forms holds against Python integers"""
    _device_equals_host(gpu, INT_OPS, name)
    cov = class_cover(INT_OPS, moduli()[name])
    cov.require(*INT_COVER)
    require_barrett_selects(cov, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PM_MODULI)
def test_pseudo_mersenne_device_forms_equal_host_forms(gpu, name):
    _device_equals_host(gpu, PM_OPS, name)
    class_cover(PM_OPS, moduli()[name]).require(*PM_COVER)


_margins = {}


@pytest.mark.gpu
@pytest.mark.parametrize("name", FP_MODULI)
def test_fp64_device_forms(gpu, name):
    q = moduli()[name]
    margins, cov = [], Cover()
    for op in FP_OPS:
        x = cases(op, q)
        check_fp(op, q, x, gpu.debug_arith(op, q, x), margins, cov)
    _margins[name] = margins
    cov.require(*fp_cover(q))
    lines = ["# largest |out| / q seen by tests/test_device_arith.py::test_fp64_device_forms, next to the bound (units of q)",
             f"# {'op':<20}{'modulus':<10}{'q':<20}{'max |out|/q':<16}bound"]
    for nm in FP_MODULI:
        lines += [f"{op:<22}{nm:<10}{qq:<20}{worst:<16.6f}{txt}" for op, qq, worst, txt in _margins.get(nm, [])]
    print("\n".join(lines[:2] + lines[-len(margins):]))
    path = os.environ.get("MKCKKS_ARITH_MARGINS")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.mark.gpu
def test_entry_point_on_the_device(gpu):
    from ppqsflhe_amd import MkckksError
    q = moduli()["q0"]
    assert gpu.debug_arith("add_mod", q, np.zeros((2, 0), dtype=np.uint64)).shape == (1, 0)  # no-op
    buf = gpu.to_device(np.arange(16, dtype=np.uint64))
    L, h = gpu._L, gpu._h
    assert L.mkckks_debug_arith(h, ARITH_OPS["add_mod"][0], q, buf.ptr, buf.ptr + 8, 4) == -1     # overlap
    assert L.mkckks_debug_arith(h, len(ARITH_OPS), q, buf.ptr, buf.ptr + 64, 4) == -1              # unknown op
    assert L.mkckks_debug_arith(h, ARITH_OPS["fp_reduce"][0], FP_LIMIT + 1, buf.ptr, buf.ptr + 64, 4) == -1
    assert L.mkckks_debug_arith(h, ARITH_OPS["pm_lazy"][0], moduli()["s54"], buf.ptr, buf.ptr + 64, 4) == -1
    assert L.mkckks_debug_arith(h, ARITH_OPS["add_mod"][0], q, buf.ptr, buf.ptr + 64, 4) == 0      # [0..8) -> [8..12)
    got = buf.to_host()
    assert [int(v) for v in got[8:12]] == [4, 6, 8, 10] and [int(v) for v in got[:8]] == list(range(8))
    with pytest.raises(MkckksError):
        gpu.debug_arith("shoup_lazy", q, np.array([[1], [q]], dtype=np.uint64))  # twiddle not below q
    # more elements than one grid pass (grid-stride loop) and a count that is no multiple of the block
    n = 4096 * 256 + 77
    rng = np.random.default_rng(1)
    x = rng.integers(0, q, size=(2, n), dtype=np.uint64)
    s = x[0] + x[1]  # below 2^61
    assert np.array_equal(gpu.debug_arith("add_mod", q, x)[0], np.where(s >= np.uint64(q), s - np.uint64(q), s))
    buf.free()
