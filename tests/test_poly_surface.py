"""Polynomial evaluation, the host side (include/mkckks.h: "polynomial evaluation"): the plan, the ladder's scales, the
weights and the refusals of the compute calls on a host-only context; and the header bookkeeping of the evalPoly host
(ppqsflhe_amd/host/poly.hpp) through its stand-alone self-test, plain and under AddressSanitizer + UBSan.

The Python restatements below (py_plan, py_ladder, py_weights, py_constants) are the definitions of the header in Python
floats and integers; tests/test_poly.py builds its expectations from them."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_parity import CONFIGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NODEVICE = -1, -2


# ---- the definitions in Python ---------------------------------------------------------------------------------------------

def clog2(v):
    return (v - 1).bit_length()


def py_plan(degree, nl):
    """B, G, nl_T, nl_out, relinearisations, depth, limbs of x^1 .. x^{B-1}, limbs of y^1 .. y^{G-1}."""
    B = 2
    while B * B < degree + 1:
        B *= 2
    G = -(-(degree + 1) // B)
    log_b, log_g = clog2(B), clog2(G - 1)
    nl_T = nl - log_b - log_g
    return dict(B=B, G=G, nl_T=nl_T, nl_out=nl_T - 2, n_relin=(B - 1) + (G - 2) + 1, depth=log_b + log_g + 2,
                baby_nl=[nl - clog2(i) for i in range(1, B)], giant_nl=[nl - log_b - clog2(j) for j in range(1, G)])


def py_ladder(moduli, nl, n_pow, scale):
    """Limbs and scales of z^1 .. z^n_pow: nl_k = nl_i - 1, S_k = S_i * S_j / q_{nl_i - 1} with i = ceil(k / 2), j = k - i."""
    nls, sc = {1: nl}, {1: float(scale)}
    for k in range(2, n_pow + 1):
        i = (k + 1) // 2
        j = k - i
        nls[k] = nls[i] - 1
        prod = sc[i] * sc[j]
        sc[k] = prod / float(int(moduli[nls[i] - 1]))
    return [nls[k] for k in range(1, n_pow + 1)], [sc[k] for k in range(1, n_pow + 1)]


def py_weights(moduli, L, sf, coef, nl, scale):
    """(w[G][B], S_out): w_{j,i} = c_{jB+i} * (Sigma / (S_{x^i} * S_{y^j})), Sigma = S_out * q_{nl_T-1} * q_{nl_T-2}."""
    p = py_plan(len(coef) - 1, nl)
    B, G = p["B"], p["G"]
    nlx, sx = py_ladder(moduli, nl, B, scale)
    _, sy = py_ladder(moduli, nlx[B - 1], G - 1, sx[B - 1])
    sx, sy = [1.0] + sx, [1.0] + sy  # sx[i]: scale of x^i (sx[B]: of y), sy[j]: of y^j
    s_out = sf(L - p["nl_out"])
    sigma = s_out * float(int(moduli[p["nl_T"] - 1])) * float(int(moduli[p["nl_T"] - 2]))
    w = np.zeros((G, B))
    for j in range(G):
        for i in range(B):
            k = j * B + i
            c = float(coef[k]) if k < len(coef) else 0.0
            w[j, i] = 0.0 if c == 0.0 else c * (sigma / (sx[i] * sy[j]))
    return w, s_out


def py_constants(w):
    """M[j][i] = rint(w[j][i]) as Python integers (round half to even; a double at or above 2^53 is an integer)."""
    return [[int(round(float(v))) for v in row] for row in w]


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


@pytest.mark.parametrize("name", ["tiny", "c5s"])
def test_poly_plan_is_the_python_restatement_on_every_degree_and_level(hosts, name):
    from ppqsflhe_amd.binding import MkckksError
    g = hosts(name)
    fits = 0
    for degree in range(2, 64):
        for nl in range(1, g.L + 1):
            want = py_plan(degree, nl)
            assert want["B"] in (2, 4, 8) and 2 <= want["G"] <= want["B"] and want["B"] * want["G"] >= degree + 1
            assert (want["B"] // 2) ** 2 < degree + 1 or want["B"] == 2  # B is the smallest such power of two
            if want["nl_out"] < 1:
                with pytest.raises(MkckksError) as e:
                    g.poly_plan(degree, nl)
                assert e.value.code == E_INVALID and f"needs {want['depth'] + 1} limbs" in str(e.value), (degree, nl)
                continue
            got = g.poly_plan(degree, nl)
            assert got == want, (degree, nl)
            assert got["depth"] == clog2(got["B"]) + clog2(got["G"] - 1) + 2 == nl - got["nl_out"]
            assert got["nl_T"] == min(got["baby_nl"] + got["giant_nl"])
            fits += 1
    assert fits > 0
    for degree, nl in ((1, g.L), (64, g.L), (0, g.L), (3, 0), (3, g.L + 1)):
        with pytest.raises(MkckksError) as e:
            g.poly_plan(degree, nl)
        assert e.value.code == E_INVALID, (degree, nl)


TANH15 = [0.0, 1.0, 0.0, -1.0 / 3, 0.0, 2.0 / 15, 0.0, -17.0 / 315, 0.0, 62.0 / 2835, 0.0, -1382.0 / 155925, 0.0,
          21844.0 / 6081075, 0.0, -929569.0 / 638512875]


@pytest.mark.parametrize("name", ["tiny", "c5s"])
def test_poly_weights_follow_the_ladder_scales(hosts, name):
    from ppqsflhe_amd.binding import MkckksError
    g = hosts(name)
    rng = np.random.default_rng(77)
    degrees = (2, 3) if name == "tiny" else (2, 3, 7, 15, 16, 31, 62, 63)
    for degree in degrees:
        for nl in range(1, g.L):  # below the top level: its limb and scale are the extra ones of FLEXIBLEAUTOEXT
            if py_plan(degree, nl)["nl_out"] < 1:
                continue
            coef = rng.uniform(-1, 1, size=degree + 1)
            coef[1] = 0.0
            if degree == 15:
                coef = np.array(TANH15)
            # the level's own scale and that of a rescaled fresh ciphertext
            scales = [g.sf(g.L - nl), g.sf_big(0) / float(int(g.moduli[g.L - 1]))]
            for scale in scales:
                w, s_out = g.poly_weights(coef, nl, scale)
                want, want_s = py_weights(g.moduli, g.L, g.sf, coef, nl, scale)
                p = g.poly_plan(degree, nl)
                assert s_out == want_s == g.sf(g.L - p["nl_out"])
                assert w.shape == want.shape == (p["G"], p["B"])
                # the same double operations in the same order: the bits agree; the issue's bound is relative 2^-50
                assert np.all(np.abs(w - want) <= np.abs(want) * 2.0 ** -50), (degree, nl)
                flat = w.reshape(-1)
                for k in range(flat.size):
                    if k > degree or coef[k] == 0.0:
                        assert flat[k] == 0.0 and not np.signbit(flat[k]), (degree, nl, k)
                    else:
                        assert flat[k] != 0.0
    # the top level, nl = L: the call accepts it like any other.  Its limb is the 20-bit extra one, so the ladder's scales
    # drift from the levels' (S_2 = S^2 / q_{L-1}); the weights are still the restatement's, bit for bit, whatever their size
    for degree in degrees:
        if py_plan(degree, g.L)["nl_out"] < 1:
            continue
        coef = rng.uniform(-1, 1, size=degree + 1)
        for scale in (g.sf(0), g.sf_big(0), g.sf(1)):
            w, s_out = g.poly_weights(coef, g.L, scale)
            want, want_s = py_weights(g.moduli, g.L, g.sf, coef, g.L, scale)
            assert s_out == want_s == g.sf(g.L - py_plan(degree, g.L)["nl_out"])
            assert np.array_equal(w, want), (degree, scale)
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(MkckksError) as e:
            g.poly_weights([1.0, bad, 0.5], g.L, g.sf(0))
        assert e.value.code == E_INVALID and "not finite" in str(e.value)
    with pytest.raises(MkckksError) as e:
        g.poly_weights([1.0, 0.5, 0.25], g.L, -1.0)
    assert e.value.code == E_INVALID


def test_compute_calls_need_a_device_and_refuse_null_pointers(hosts):
    """A host-only context: valid arguments give MKCKKS_E_NODEVICE, a null pointer MKCKKS_E_INVALID; nothing is dereferenced
    (the addresses below are not memory)."""
    from ppqsflhe_amd.binding import MkckksError
    g = hosts("tiny")
    nl, big = 4, 1 << 40  # arrays `big` bytes apart never overlap
    scale = g.sf(g.L - nl)
    coef = [0.5, 1.0, 0.0, -1.0 / 3]
    w, _ = g.poly_weights(coef, nl, scale)
    p = g.poly_plan(3, nl)
    calls = {
        "powers": lambda z, k, o: g.powers(z, k, o, 1, nl, 3, scale),
        "poly_eval": lambda z, k, o: g.poly_eval(z, k, coef, o, 1, nl, scale),
        "poly_tensor": lambda z, k, o: g.poly_tensor(z, p["baby_nl"], k, p["giant_nl"], w, o, 1, p["nl_T"]),
    }
    for what, call in calls.items():
        with pytest.raises(MkckksError) as e:
            call(big, 2 * big, 3 * big)
        assert e.value.code == E_NODEVICE, what
        for args in ((None, 2 * big, 3 * big), (big, None, 3 * big), (big, 2 * big, None)):
            with pytest.raises(MkckksError) as e:
                call(*args)
            assert e.value.code == E_INVALID and "null" in str(e.value), (what, args)
    # zero ciphertexts: a no-op, decided before a device is asked for
    g.powers(big, 2 * big, 3 * big, 0, nl, 3, scale)
    g.poly_eval(big, 2 * big, coef, 3 * big, 0, nl, scale)
    g.poly_tensor(big, p["baby_nl"], 2 * big, p["giant_nl"], w, 3 * big, 0, p["nl_T"])
    # and the refusals that need no device: alignment, overlap, plan, weights
    for call, code in ((lambda: g.poly_eval(big + 8, 2 * big, coef, 3 * big, 1, nl, scale), "aligned"),
                       (lambda: g.poly_eval(big, 2 * big, coef, big, 1, nl, scale), "overlaps"),
                       (lambda: g.poly_eval(big, 2 * big, coef, 3 * big, 1, 3, g.sf(g.L - 3)), "needs 4 limbs"),
                       (lambda: g.poly_tensor(big, p["baby_nl"], 2 * big, p["giant_nl"], w * 2.0 ** 200, 3 * big, 1, p["nl_T"]),
                        "does not fit")):
        with pytest.raises(MkckksError) as e:
            call()
        assert e.value.code == E_INVALID and code in str(e.value), code


# ---- the evalPoly host's header bookkeeping -----------------------------------------------------------------------------------

HOST = os.path.join(ROOT, "ppqsflhe_amd", "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")


@pytest.mark.parametrize("target", ["build/poly_selftest", "build/asan/poly_selftest"])
def test_poly_bookkeeping_plain_and_under_sanitizers(target):
    """poly.hpp through its stand-alone program (its own main, no library): plain, and compiled with
    -fsanitize=address,undefined as an executable of its own."""
    r = subprocess.run(["make", "-C", HOST, "-s", target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(HOST, *target.split("/"))], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "poly selftest ok" in r.stdout and "FAIL" not in r.stdout, r.stdout
