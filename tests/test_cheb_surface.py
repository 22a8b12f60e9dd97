"""Chebyshev series, the host side (include/mkckks.h: "Chebyshev series"): the block rewrite and its weights, the ladder's
limbs and scales, and the refusals of the compute calls, all on a host-only context.

The Python restatements below (py_cheb_rewrite, py_cheb_weights, cheb_ladder_values) are the definitions of the header in
Python floats, integers and fractions; tests/test_cheb.py builds its expectations from them."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests.test_gpu_parity import CONFIGS
from tests.test_poly_surface import py_ladder, py_plan, py_weights

E_INVALID, E_NODEVICE = -1, -2


# ---- the definitions in Python ---------------------------------------------------------------------------------------------

def py_cheb_rewrite(coef, B, G, zero=0.0):
    """m[G][B] with sum_k c_k T_k = sum_j sum_i m[j][i] T_i T_{jB}, in the header's order; works on floats and on exact
    numbers alike (zero = the additive identity of the coefficients' type)."""
    c = list(coef) + [zero] * (B * G - len(coef))
    m = [[zero] * B for _ in range(G)]
    for j in range(G - 1, 0, -1):
        for i in range(B - 1, 0, -1):
            m[j][i] = 2 * c[j * B + i]
            c[(j - 1) * B + (B - i)] -= c[j * B + i]
        m[j][0] = c[j * B]
    for i in range(B):
        m[0][i] = c[i]
    return m


def py_cheb_weights(moduli, L, sf, coef, nl, scale):
    """(w[G][B], S_out): the rewrite, then the weights of the polynomial block formed from m instead of c."""
    p = py_plan(len(coef) - 1, nl)
    m = py_cheb_rewrite([float(c) for c in coef], p["B"], p["G"])
    flat = [v for row in m for v in row]
    assert py_plan(len(flat) - 1, nl) == p  # B * G - 1 has the plan of the degree
    return py_weights(moduli, L, sf, flat, nl, scale)


def cheb_ladder_values(u, n):
    """[T_0(u) .. T_n(u)] by the ladder rule T_k = 2 T_i T_j - T_{i-j}, i = ceil(k / 2), j = k - i, in u's own arithmetic."""
    T = [u * 0 + 1, u]
    for k in range(2, n + 1):
        i = (k + 1) // 2
        j = k - i
        assert i - j in (0, 1)
        T.append(2 * T[i] * T[j] - T[i - j])
    return T[:n + 1]


# ---- host-only context ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hosts():
    from ppqsflhe_amd import Context
    cache = {}

    def get(name):
        if name not in cache:
            a = CONFIGS[name]
            cache[name] = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=-1)
        return cache[name]

    yield get
    for g in cache.values():
        g.close()


def test_symbols_exist_in_the_library_and_the_binding():
    from ppqsflhe_amd import Context, binding
    L = binding.load_library()
    for name in ("mkckks_affine_batch", "mkckks_cheb_tensor_batch", "mkckks_cheb_ladder_batch", "mkckks_cheb_weights",
                 "mkckks_cheb_eval_batch"):
        assert hasattr(L, name) and name in binding.SYMBOLS, name
    for name in ("affine", "cheb_tensor", "cheb_ladder", "cheb_weights", "cheb_eval"):
        assert callable(getattr(Context, name)), name


def test_the_ladder_rule_is_the_three_term_recurrence():
    for u in (Fraction(3, 7), Fraction(-5, 9), Fraction(1), Fraction(0), Fraction(-1), Fraction(7, 3)):
        T = cheb_ladder_values(u, 64)
        assert T[0] == 1 and T[1] == u
        for k in range(2, 65):
            assert T[k] == 2 * u * T[k - 1] - T[k - 2], (u, k)


@pytest.mark.parametrize("degree", [2, 3, 7, 15, 16, 31, 62, 63])
def test_the_rewrite_identity_is_exact(degree):
    """Integer coefficients and rational u: sum m[j][i] T_i(u) T_j(T_B(u)) = sum c_k T_k(u), with no rounding anywhere."""
    rng = np.random.default_rng(2100 + degree)
    p = py_plan(degree, 64)
    B, G = p["B"], p["G"]
    coef = [Fraction(int(v)) for v in rng.integers(-1000, 1001, size=degree + 1)]
    coef[-1] = Fraction(17)  # the top coefficient is live
    m = py_cheb_rewrite(coef, B, G, zero=Fraction(0))
    for u in (Fraction(3, 7), Fraction(-5, 9), Fraction(1), Fraction(-1), Fraction(0), Fraction(1, 1000)):
        T = cheb_ladder_values(u, max(B, degree))
        Y = cheb_ladder_values(T[B], G - 1)  # the giants: the same ladder on y = T_B
        for j in range(G):
            assert Y[j] == T[j * B] or j * B > degree  # T_{jB} = T_j(T_B)
        want = sum(c * T[k] for k, c in enumerate(coef))
        got = sum(m[j][i] * T[i] * Y[j] for j in range(G) for i in range(B))
        assert got == want, (degree, u)


@pytest.mark.parametrize("name", ["tiny", "c5s"])
def test_cheb_weights_are_the_python_restatement_to_the_last_bit(hosts, name):
    g = hosts(name)
    rng = np.random.default_rng(2200)
    degrees = (2, 3) if name == "tiny" else (2, 3, 7, 15, 31, 63)
    seen = 0
    for degree in degrees:
        for nl in range(1, g.L):
            if py_plan(degree, nl)["nl_out"] < 1:
                continue
            coef = rng.uniform(-1, 1, size=degree + 1)
            coef[1] = 0.0
            for scale in (g.sf(g.L - nl), g.sf_big(0) / float(int(g.moduli[g.L - 1]))):
                w, s_out = g.cheb_weights(coef, nl, scale)
                want, want_s = py_cheb_weights(g.moduli, g.L, g.sf, coef, nl, scale)
                p = g.poly_plan(degree, nl)
                assert s_out == want_s == g.sf(g.L - p["nl_out"])
                assert w.shape == want.shape == (p["G"], p["B"])
                assert np.array_equal(w, want), (degree, nl)
                assert np.all(np.isfinite(w))
                seen += 1
    assert seen > 0


def test_a_zero_coefficient_gives_an_exact_zero_weight(hosts):
    g = hosts("c5s")
    nl = 12
    # degree 15: B = G = 4.  Only c_0, c_1 and c_5 live: m[1][1] = 2 c_5 and, through the rewrite, m[0][3] = -c_5
    coef = np.zeros(16)
    coef[0], coef[1], coef[5] = 0.5, -0.25, 0.125
    coef[15] = 0.0
    w, _ = g.cheb_weights(coef, nl, g.sf(g.L - nl))
    live = {(0, 0), (0, 1), (1, 1), (0, 3)}
    for j in range(4):
        for i in range(4):
            if (j, i) in live:
                assert w[j, i] != 0.0, (j, i)
            else:
                assert w[j, i] == 0.0 and not np.signbit(w[j, i]), (j, i)
    want, _ = py_cheb_weights(g.moduli, g.L, g.sf, coef, nl, g.sf(g.L - nl))
    assert np.array_equal(w, want)
    assert w[0, 3] < 0 < w[1, 1]


def test_refusals_that_need_no_device(hosts):
    from ppqsflhe_amd.binding import MkckksError
    g = hosts("tiny")
    nl, big = 4, 1 << 40  # arrays `big` bytes apart never overlap
    scale = g.sf(g.L - nl)
    coef = [0.5, 1.0, 0.0, -1.0 / 3]

    def refused(call, text, code=E_INVALID):
        with pytest.raises(MkckksError) as e:
            call()
        assert e.value.code == code and text in str(e.value), (text, str(e.value))

    ev = lambda c=coef, a=-1.0, b=1.0, ct=big, rlk=2 * big, out=3 * big, n=1, l=nl, s=scale: g.cheb_eval(ct, rlk, c, a, b, out, n, l, s)
    refused(lambda: ev(c=[0.5, 1.0]), "degree must be in [2, 63]")                     # degree 1
    refused(lambda: ev(c=[0.1] * 65), "degree must be in [2, 63]")                     # degree 64
    for n_coef in (2, 65):  # the binding's own size check is not in the way of the library's
        c_in, w_out, s_out = np.full(n_coef, 0.5), np.zeros(64), C.c_double()
        refused(lambda: g._check(g._L.mkckks_cheb_weights(g._h, c_in.ctypes.data, n_coef - 1, nl, scale, w_out.ctypes.data,
                                                          C.byref(s_out))), "degree must be in [2, 63]")
    refused(lambda: ev(a=1.0, b=1.0), "finite a < b")
    refused(lambda: ev(a=2.0, b=1.0), "finite a < b")
    refused(lambda: ev(a=np.nan), "finite a < b")
    refused(lambda: ev(b=np.inf), "finite a < b")
    refused(lambda: ev(c=[0.5, np.nan, 0.25]), "not finite")
    refused(lambda: ev(l=3, s=g.sf(g.L - 3)), "needs 4 limbs")                         # nl_out < 1
    refused(lambda: ev(a=0.25, b=4.0), "needs 4 limbs")                                # the map spends one of the 4
    refused(lambda: ev(ct=None), "null")
    refused(lambda: ev(rlk=None), "null")
    refused(lambda: ev(out=None), "null")
    refused(lambda: ev(ct=big + 8), "aligned")
    refused(lambda: ev(out=big), "overlaps")
    refused(lambda: ev(), "", code=E_NODEVICE)                                          # valid arguments: no device
    ev(n=0)                                                                             # zero ciphertexts: a no-op
    g5 = hosts("c5s")
    refused(lambda: g5.cheb_eval(big, 2 * big, coef, 0.25, 4.0, 3 * big, 1, 12, g5.sf(g5.L - 12)), "", code=E_NODEVICE)
    # the other compute calls
    refused(lambda: g.affine(big, 2 * big, 1, nl, 3.0, 5.0), "", code=E_NODEVICE)
    refused(lambda: g.affine(big, big, 1, nl, 3.0, 5.0), "", code=E_NODEVICE)            # in place is allowed
    refused(lambda: g.affine(big, big + 16, 1, nl, 3.0, 5.0), "overlaps")
    refused(lambda: g.affine(None, big, 1, nl, 3.0, 5.0), "null")
    refused(lambda: g.affine(big, 2 * big, 1, nl, 2.0 ** 200, 5.0), "does not fit")
    refused(lambda: g.affine(big, 2 * big, 1, nl, 3.0, np.nan), "not finite")
    g.affine(big, 2 * big, 0, nl, 3.0, 5.0)
    ten = lambda a=big, b=2 * big, t=3 * big, w=7.0, o=4 * big, la=nl, lb=nl, lt=nl, l=3, n=1: g.cheb_tensor(a, la, b, lb, t, lt, w, o, n, l)
    refused(lambda: ten(), "", code=E_NODEVICE)
    refused(lambda: ten(t=None), "", code=E_NODEVICE)                                   # the constant term
    refused(lambda: ten(a=None), "null")
    refused(lambda: ten(o=None), "null")
    refused(lambda: ten(la=2), "limb count")                                            # below nl
    refused(lambda: ten(lt=2), "limb count")
    refused(lambda: ten(lb=g.L + 1), "limb count")
    refused(lambda: ten(o=big), "overlaps")
    refused(lambda: ten(t=big + 8), "aligned")
    refused(lambda: ten(w=2.0 ** 200), "does not fit")
    ten(n=0)
    lad = lambda u=big, k=2 * big, o=3 * big, n=3, l=nl, c=1: g.cheb_ladder(u, k, o, c, l, n, scale)
    refused(lambda: lad(), "", code=E_NODEVICE)
    refused(lambda: lad(u=None), "null")
    refused(lambda: lad(o=big), "overlaps")
    refused(lambda: lad(n=9), "power ladder")                                           # 4 - ceil(log2 9) < 1
    refused(lambda: g.cheb_ladder(big, 2 * big, 3 * big, 1, 1, 1, -1.0), "scale")
    lad(c=0)


@pytest.mark.parametrize("name,nl,n", [("tiny", 4, 3), ("c5s", 12, 8), ("c5s", 19, 64)])
def test_the_ladder_reports_the_limbs_and_scales_of_the_power_ladder(hosts, name, nl, n):
    """A zero count is decided before a device is asked for, and the limb counts and scales are written first."""
    g = hosts(name)
    scale = g.sf(g.L - nl)
    big = 1 << 40
    nls, scales = g.cheb_ladder(big, 2 * big, 3 * big, 0, nl, n, scale)
    want_nl, want_s = py_ladder(g.moduli, nl, n, scale)
    assert nls == want_nl == [nl - (k - 1).bit_length() for k in range(1, n + 1)]
    assert scales == want_s
