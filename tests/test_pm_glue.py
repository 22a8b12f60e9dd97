"""The pseudo-Mersenne integer primitives of modarith.hpp (pm_lazy, pm_fold, pm_reduce128, pm_reduce_cols, csub, mac128).

Their device forms take the multiplier's carry-out and chain the multiply-adds instead of splitting words; every lazy
bound and every stored bit rests on each of them returning the same 64-bit word as the formula it replaced.

* CPU: ppqsflhe_amd/csrc/pm_glue_selftest.cpp (built under -fsanitize=address,undefined) compares the host forms word for
  word with the earlier formulas, kept verbatim in it, and with unsigned __int128 arithmetic mod q -- the reference
  context's 60-bit primes, a 55- and a 58-bit prime, boundary operands and 10^6 random operands each, both values of the
  carry seen.
* GPU (`-m gpu`): the HIP kernels that are built from these primitives against the oracle, bit for bit, at the smallest
  ring the radix kernels and the merged n-client flow serve (the reference's N = 2^14, L = 4, dnum = 2).
* The device forms themselves, one primitive at a time and at the edges of their ranges (a just below 8U, X just below
  2^(2k+6), both values of every carry), are compared word for word with the host forms in tests/test_device_arith.py.
"""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ppqsflhe_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
REF = (14, 2, 40, 60, 2)  # log_n, depth, scaling bits, first-modulus bits, dnum


def test_host_forms_return_the_words_of_the_earlier_formulas():
    r = subprocess.run(["make", "-C", CSRC, "-s", "../pm_glue_selftest_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(ROOT, "ppqsflhe_amd", "pm_glue_selftest_asan")], capture_output=True, text=True,
                       env=ENV, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    widths = sorted(int(b) for b in re.findall(r"ok q=\d+ \((\d+) bits\)", r.stdout))
    assert widths.count(60) >= 3 and 55 in widths and 58 in widths, r.stdout  # q0 + the special primes, 55, 58 bits
    m = re.search(r"ok pm glue: (\d+) primes, pm_lazy (\d+) \(carry 1: (\d+), carry 0: (\d+)\)", r.stdout)
    assert m, r.stdout
    primes, lazy, carry1, carry0 = map(int, m.groups())
    assert lazy >= primes * 10**6 and carry1 > 0 and carry0 > 0 and carry1 + carry0 == lazy


@pytest.fixture(scope="module")
def ref_pair():
    from oracle.oracle import OracleContext
    from ppqsflhe_amd import Context
    g = Context(*REF[:4], dnum=REF[4], device=0)
    o = OracleContext(*REF[:4], dnum=REF[4])
    yield g, o
    g.close()


def integer_limbs(g):
    """q0 and the special primes: the 60-bit limbs that run on the integer (pseudo-Mersenne or Shoup) instances."""
    return [l for l in range(g.D) if int(g.moduli[l]).bit_length() > 51]


def patterns(g, ids):
    rng = np.random.default_rng(5)
    x = np.zeros((3, len(ids), g.N), dtype=np.uint64)
    for j, l in enumerate(ids):
        q = int(g.moduli[l])
        x[0, j] = rng.integers(0, q, size=g.N, dtype=np.uint64)  # uniform
        x[1, j] = q - 1                                          # every residue q - 1
        x[2, j, 0::2] = q - 1                                    # alternating q - 1 / 0
    return x


@pytest.mark.gpu
def test_integer_limb_transforms_match_the_oracle(ref_pair):
    g, o = ref_pair
    ids = list(range(g.D))
    ints = integer_limbs(g)
    assert 0 in ints and all(l in ints for l in range(g.L, g.D))
    x = patterns(g, ids)
    d = g.to_device(x)
    g.ntt_forward(d, 3, g.L, with_p=True)
    fwd = d.to_host()
    g.ntt_inverse(d, 3, g.L, with_p=True)
    back = d.to_host()
    d.upload(x)
    g.ntt_inverse(d, 3, g.L, with_p=True)  # the inverse butterflies on arbitrary (not transformed) input
    inv = d.to_host()
    for p in range(3):
        for l in ints:
            assert np.array_equal(fwd[p, l], o.ntt_fwd(l, x[p, l])), ("forward", p, l)
            assert np.array_equal(inv[p, l], o.ntt_inv(l, x[p, l])), ("inverse", p, l)
    assert np.array_equal(back, x)


def sum_and_rescale(g, o, cts, evks, C, B, nl):
    d_sum = g.empty((B, 2, nl, g.N))
    g.reencrypt_sum(g.to_device(cts), g.to_device(evks), d_sum, C, B, nl)
    d_avg = g.empty((B, 2, nl - 1, g.N))
    g.rescale_mult_const(d_sum, d_avg, B, nl, 1.0 / C)
    return d_sum.to_host(), d_avg.to_host()


@pytest.fixture(scope="module")
def round_case(ref_pair):
    """3 clients x 2 ciphertexts and the oracle's chain for them (computed once, shared by the two arithmetic classes)."""
    g, o = ref_pair
    C, B, nl = 3, 2, g.L
    rng = np.random.default_rng(29)

    def rnd(ids, lead):
        out = np.empty(lead + (len(ids), g.N), dtype=np.uint64)
        for j, l in enumerate(ids):
            out[..., j, :] = rng.integers(0, int(g.moduli[l]), size=lead + (g.N,), dtype=np.uint64)
        return out

    cts = rnd(list(range(nl)) * 2, (C, B)).reshape(C, B, 2, nl, g.N)
    evks = rnd(list(range(g.D)) * (2 * g.beta), (C,)).reshape(C, g.beta, 2, g.D, g.N)
    sums, avgs = [], []
    for b in range(B):
        acc = o.reencrypt(cts[0, b], evks[0])
        for c in range(1, C):
            acc = o.eval_add(acc, o.reencrypt(cts[c, b], evks[c]))
        sums.append(acc)
        avgs.append(o.mult_factors(o.rescale(acc), o.const_factors(nl - 1, 1, 1.0 / C)))
    return cts, evks, C, B, nl, np.stack(sums), np.stack(avgs)


@pytest.mark.gpu
def test_sum_of_reencryptions_and_rescale_match_the_oracle(ref_pair, round_case):
    g, o = ref_pair
    cts, evks, C, B, nl, want_sum, want_avg = round_case
    got_sum, got_avg = sum_and_rescale(g, o, cts, evks, C, B, nl)
    assert np.array_equal(got_sum, want_sum)
    assert np.array_equal(got_avg, want_avg)


@pytest.mark.gpu
def test_shoup_instances_stay_bit_exact(ref_pair, round_case, monkeypatch):
    """MKCKKS_NO_PM=1 runs q0 and the special primes on the Shoup instances, which share csub and mac128 with the
    pseudo-Mersenne ones.  The switch is read when a context is created."""
    from ppqsflhe_amd import Context
    _, o = ref_pair
    cts, evks, C, B, nl, want_sum, want_avg = round_case
    monkeypatch.setenv("MKCKKS_NO_PM", "1")
    g2 = Context(*REF[:4], dnum=REF[4], device=0)
    try:
        got_sum, got_avg = sum_and_rescale(g2, o, cts, evks, C, B, nl)
        assert np.array_equal(got_sum, want_sum)
        assert np.array_equal(got_avg, want_avg)
    finally:
        g2.close()
