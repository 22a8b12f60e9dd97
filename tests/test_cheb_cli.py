"""evalPoly --cheb.  Without a GPU: the argv contract of the mode, the coefficients --function fits (against numpy's
chebinterpolate: both are the same double-precision interpolation at the Chebyshev nodes), the refusals decided from headers
and host tables (a series that does not fit the limbs, the map's extra limb, the headroom rule on a host-only session), and
the stand-alone self-test of ppqsflhe_amd/host/poly.hpp's Chebyshev part, plain and under AddressSanitizer + UBSan.  On the
GPU, one round at the "tiny" parameters: genCC -> keyGen -> relinKeyGen -> encryptModelWeights -> evalPoly --cheb -1,1
--function tanh --degree 3 -> decryptModelWeights, within the bound of tests/test_cheb.py (4 x the largest error of the CPU
chain at these parameters) of the fitted series' own value."""
import os
import re
import subprocess

import numpy as np
import pytest
from numpy.polynomial import chebyshev as npcheb

from tests.test_cheb import CHEB_BOUND, TANH3
from tests.test_cli_hosts import BIN, _weights, run, write_key_container
from tests.test_poly_cli import N, SLOTS, USAGE, tiny_cc
from tests.test_product_cli import KIND_RELIN, ct_blob, envelope
from tests.test_slot_weights_cli import ok

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppqsflhe_amd", "host")
CHEB_USAGE = "--cheb a,b (--coeffs c0,c1,...,cd | --function {invsqrt,sigmoid,tanh,exp} --degree d)"
NO_DEVICE = {"MKCKKS_DEVICE": "-1"}
FUNCS = {"invsqrt": lambda t: 1.0 / np.sqrt(t), "sigmoid": lambda t: 1.0 / (1.0 + np.exp(-t)), "tanh": np.tanh, "exp": np.exp}


def series_of(stdout):
    """The coefficients evalPoly printed for its --function fit."""
    m = re.search(r"series ([^\n]+)", stdout)
    assert m, stdout
    return np.array([float(x) for x in m.group(1).split(",")])


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    d = tmp_path_factory.mktemp("cheb_crafted")
    cc = tiny_cc(d)
    key = d / "relin.key"
    write_key_container(key, KIND_RELIN, N, 8, 4, np.zeros(4, dtype=np.uint64))
    fresh = envelope(d / "a.json", [ct_blob(limbs=5, level=0, noise_deg=2, scale=2.0 ** 80, slots=SLOTS)] * 3)
    return d, cc, key, fresh


def test_the_mode_states_its_usage(crafted):
    d, cc, key, fresh = crafted
    base = (cc, key, fresh, d / "out.json")
    for args in (("--cheb", "-1,1"), ("--cheb", "-1,1", "--function", "tanh"), ("--cheb", "-1,1", "--degree", "3"),
                 ("--cheb", "-1,1", "--coeffs", "1,2,3", "--function", "tanh", "--degree", "3"),
                 ("--cheb", "-1,1", "--coeffs", "1,2,3", "--max-abs", "2"), ("--cheb", "-1,1", "--cheb", "-1,1", "--coeffs", "1,2,3"),
                 ("--function", "tanh", "--degree", "3"), ("--coeffs", "1,2,3", "--degree", "3")):
        r = run("evalPoly", *base, *args)
        assert r.returncode == 1 and "Usage:" in r.stderr and USAGE in r.stderr and CHEB_USAGE in r.stderr, (args, r.stderr)


@pytest.mark.parametrize("fn,a,b,degree", [("invsqrt", 0.25, 4.0, 15), ("invsqrt", 0.25, 4.0, 31), ("invsqrt", 0.25, 4.0, 63),
                                           ("sigmoid", -8.0, 8.0, 31), ("tanh", -1.0, 1.0, 3), ("tanh", -4.0, 4.0, 63),
                                           ("exp", -1.0, 2.0, 15)])
def test_function_coefficients_are_numpys_interpolation(crafted, fn, a, b, degree):
    """The fit is printed before anything else is opened; the run then ends on whatever the crafted input lacks."""
    d, cc, key, fresh = crafted
    r = run("evalPoly", cc, key, fresh, d / "out.json", "--cheb", f"{a!r},{b!r}", "--function", fn, "--degree", degree)
    got = series_of(r.stdout)
    want = npcheb.chebinterpolate(lambda u: FUNCS[fn](0.5 * ((b - a) * u + (a + b))), degree)
    assert got.shape == want.shape == (degree + 1,)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{fn} on [{a}, {b}] degree {degree}: largest difference {err:.2e} of the largest coefficient")
    assert err <= 1e-12, (fn, degree, err)
    assert not os.path.exists(d / "out.json")


def test_refusals_decided_without_a_device(crafted):
    d, cc, key, fresh = crafted
    out = d / "out.json"

    def refused(args, msg, env=None):
        r = run("evalPoly", cc, key, fresh, out, *args, env=env)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stdout + r.stderr)
        assert not os.path.exists(out), args
        return r

    for bad, msg in (("1", "--cheb needs an interval a,b"), ("1,1", "--cheb needs a < b"), ("2,1", "--cheb needs a < b"),
                     ("x,1", "--cheb needs an interval a,b of two finite numbers"),
                     ("0,inf", "--cheb needs an interval a,b of two finite numbers"),
                     ("0,1,2", "--cheb needs an interval a,b of two finite numbers")):
        refused(("--cheb", bad, "--coeffs", "1,2,3"), "[evalpoly] ERROR: " + msg)
    refused(("--cheb", "0,4", "--function", "invsqrt", "--degree", "15"), "--function invsqrt needs an interval with a > 0")
    refused(("--cheb", "-1,1", "--function", "cos", "--degree", "15"), "--function: unknown function cos")
    refused(("--cheb", "-1,1", "--function", "tanh", "--degree", "64"), "--degree: the degree must be in [2, 63], got 64")
    refused(("--cheb", "-1,1", "--function", "tanh", "--degree", "1"), "--degree: the degree must be in [2, 63], got 1")
    refused(("--cheb", "-1,1", "--function", "tanh", "--degree", "x"), "--degree needs a whole number")
    refused(("--cheb", "-1,1", "--coeffs", "1,2"), "the degree must be in [2, 63], got 2 coefficient(s)")
    # the limbs: a fresh ciphertext has 5, 4 after its rescale; degree 3 needs 4 on [-1, 1] and 5 on any other interval
    refused(("--cheb", "-1,1", "--function", "tanh", "--degree", "7"),
            "[evalpoly] ERROR: degree 7 needs 5 limbs (depth 4 and one limb for the result), the input has 4 after the rescale")
    refused(("--cheb", "0.25,4", "--coeffs", "1,2,3,4"),
            "[evalpoly] ERROR: degree 3 needs 5 limbs (depth 4, the map onto [-1, 1] included, and one limb for the result), the input has 4")
    # the headroom rule, on a host-only session: Sigma is about 2^120 on limbs of 140 bits, sum |m| = 3e9 needs 151
    refused(("--cheb", "-1,1", "--coeffs", "1e9,1e9,1e9"), "[evalpoly] ERROR: no headroom: the outer sum needs", env=NO_DEVICE)
    # a series that has the headroom: the check is printed, and the run ends where it needs what a crafted key lacks
    r = run("evalPoly", cc, key, fresh, out, "--cheb", "-1,1", "--coeffs", ",".join(repr(c) for c in TANH3), env=NO_DEVICE)
    assert r.returncode == 1 and "[evalpoly] headroom: the outer sum needs" in r.stdout and "no headroom" not in r.stderr, r.stdout + r.stderr
    assert not os.path.exists(out)


ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")


@pytest.mark.parametrize("target", ["build/cheb_selftest", "build/asan/cheb_selftest"])
def test_cheb_bookkeeping_plain_and_under_sanitizers(target):
    """poly.hpp's Chebyshev part through its stand-alone program (its own main, no library): plain, and compiled with
    -fsanitize=address,undefined as an executable of its own."""
    r = subprocess.run(["make", "-C", HOST, "-s", target], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(HOST, *target.split("/"))], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "cheb selftest ok" in r.stdout and "FAIL" not in r.stdout, r.stdout


N_DENSE, N_BIAS = 300, 5


@pytest.fixture(scope="module")
def deployment(tmp_path_factory):
    d = tmp_path_factory.mktemp("cheb")
    cc = tiny_cc(d)
    rng = np.random.default_rng(2027)
    layers = [("dense", rng.uniform(-1.0, 1.0, N_DENSE)), ("bias", rng.uniform(-1.0, 1.0, N_BIAS))]
    ok(run("keyGen", cc, d / "pk", d / "sk"))
    ok(run("relinKeyGen", cc, d / "sk", d / "pk", d / "relin"))
    ok(run("encryptModelWeights", cc, d / "pk", _weights(d, "a.json", layers), d / "a.mkws"))
    return d, cc, layers


@gpu
def test_evalpoly_cheb_round_decrypts_to_the_series(deployment):
    import json
    d, cc, layers = deployment
    r = ok(run("evalPoly", cc, d / "relin", d / "a.mkws", d / "p.mkws", "--cheb", "-1,1", "--function", "tanh", "--degree", 3))
    assert "Chebyshev series on [-1, 1]" in r.stdout and "[evalpoly] headroom: the outer sum needs" in r.stdout, r.stdout
    assert "degree 3" in r.stdout and "B 2, G 2, 2 relinearisation(s), 4 -> 1 limb(s)" in r.stdout, r.stdout
    coef = series_of(r.stdout)
    assert np.abs(coef - np.array(TANH3)).max() <= 1e-12
    ok(run("decryptModelWeights", cc, d / "sk", d / "p.mkws", d / "p.json"))
    dec = json.load(open(d / "p.json"))["weights_summary"]
    series = lambda v: npcheb.chebval(v, coef)
    for li, (name, v) in enumerate(layers):
        err = np.abs(np.array(dec[li]["values"]) - series(v)).max()
        print(f"{name}: |decrypted - series(x)| = 2^{np.log2(err):.2f}, bound 2^{np.log2(CHEB_BOUND['tanh3']):.2f}")
        assert dec[li]["layer"] == name and err <= CHEB_BOUND["tanh3"], (name, err)
        assert abs(dec[li]["mean"] - series(float(np.mean(v)))) <= CHEB_BOUND["tanh3"]
        assert abs(dec[li]["std_dev"] - series(float(np.std(v)))) <= CHEB_BOUND["tanh3"]
    # the same series given as --coeffs: the same bytes
    ok(run("evalPoly", cc, d / "relin", d / "a.mkws", d / "q.mkws", "--cheb", "-1,1", "--coeffs", ",".join(repr(float(c)) for c in coef)))
    assert open(d / "p.mkws", "rb").read() == open(d / "q.mkws", "rb").read()
    # an interval that is mapped needs a limb these parameters do not have
    r = run("evalPoly", cc, d / "relin", d / "a.mkws", d / "x.mkws", "--cheb", "-2,2", "--function", "tanh", "--degree", 3)
    assert r.returncode == 1 and "degree 3 needs 5 limbs" in r.stderr and not os.path.exists(d / "x.mkws"), r.stderr
