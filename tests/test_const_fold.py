"""Two constants folded into tables of the merged n-client flow.

* ModDown's scale N^-1 [(P/p_k)^-1]_{p_k} sits in the ModUp constants of the P targets (ParamSet::modup_table_pscaled):
  everything between the conversion into a P limb and k_icol_sum is linear mod p_k, so k_icol_sum only brings the inverse
  round's lazy word to its canonical residue before the integer sum over the clients.
* The packed 60-bit q_0 source of a digit "q_0 + fp64-class limbs" meets an fp64-class target as two FMA products of its
  30-bit halves (k_conv_col / k_conv_col2, SRCMODE 2).

CPU: ppqsflhe_amd/csrc/const_fold_selftest.cpp (built under -fsanitize=address,undefined) checks the tables, the host
form of the canonicalisation and the half constants against unsigned __int128 arithmetic.

GPU (`-m gpu`): every device result is compared bit for bit with the oracle's per-client chain,
FastCpuContext.reencrypt + eval_add per index.  Shapes are the smallest that reach each path: N = 2^14 with a digit of
q_0 + one fp64 source (dnum 2, 3) and q_0 + three (L = 8, dnum 2: the flagship's instance), 1 / 2 / 8 clients, 1 / 3
indices, a second client group, reduced levels with a partial last digit, maximal / alternating / zero operands, the
Shoup and the integer-only instances, 512-point rows, the weighted instance, and the flows that keep the unscaled tables.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle.oracle import FastCpuContext  # noqa: E402

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ppqsflhe_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")

PARAMS = {
    # name: (log_n, depth, scaling_bits, first_bits, dnum); L = depth + 2
    "l4d2": (14, 2, 40, 60, 2),   # digit 0 = q_0 + one fp64 source
    "l6d3": (14, 4, 40, 60, 3),
    "l8d2": (14, 6, 40, 60, 2),   # digit 0 = q_0 + three fp64 sources: the flagship's conversion instance
    "n17": (17, 2, 50, 60, 2),    # 512-point rows
}


def test_host_tables_and_forms_against_128_bit_arithmetic():
    r = subprocess.run(["make", "-C", CSRC, "-s", "../const_fold_selftest_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(ROOT, "ppqsflhe_amd", "const_fold_selftest_asan")], capture_output=True, text=True,
                       env=ENV, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert len(re.findall(r"^ok log_n=", r.stdout, re.M)) == 5, r.stdout
    m = re.search(r"ok const fold: (\d+) P limbs, scaled sums (\d+), column forms (\d+), canon pm (\d+), canon shoup (\d+), "
                  r"halves (\d+)", r.stdout)
    assert m, r.stdout
    assert all(int(v) > 0 for v in m.groups())


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
    """Device contexts by (parameter set, switches) and one oracle per parameter set, created on first use."""
    from ppqsflhe_amd import Context
    dev, ora = {}, {}

    def device(name, **env):
        key = (name, tuple(sorted(env.items())))
        if key not in dev:
            a = PARAMS[name]
            with _Env(env):
                dev[key] = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)
        return dev[key]

    def oracle(name):
        if name not in ora:
            a = PARAMS[name]
            ora[name] = FastCpuContext(a[0], a[1], a[2], a[3], dnum=a[4])
        return ora[name]

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
    """Per index, the EvalAdd chain over the clients of their re-encryptions: [B][2][nl][N]."""
    C, B = cts.shape[:2]
    out = []
    for b in range(B):
        acc = o.reencrypt(cts[0, b], evks[0])
        for c in range(1, C):
            acc = o.eval_add(acc, o.reencrypt(cts[c, b], evks[c]))
        out.append(acc)
    return np.stack(out)


_cases = {}


def case(o, name, nl, C, B):
    """Seeded inputs and their oracle result, computed once per shape and shared (read-only) by the tests."""
    key = (name, nl, C, B)
    if key not in _cases:
        rng = np.random.default_rng(9100 + 101 * nl + 17 * C + B)
        cts = rand_polys(rng, o, list(range(nl)) * 2, C * B).reshape(C, B, 2, nl, o.N)
        evks = rand_polys(rng, o, list(range(o.D)) * (2 * o.beta), C).reshape(C, o.beta, 2, o.D, o.N)
        want = oracle_chain(o, cts, evks)
        for a in (cts, evks, want):
            a.setflags(write=False)
        _cases[key] = (cts, evks, want)
    return _cases[key]


def gpu_sum(g, cts, evks, nl):
    C, B = cts.shape[:2]
    d_out = g.empty((B, 2, nl, g.N))
    g.reencrypt_sum(g.to_device(cts), g.to_device(evks), d_out, C, B, nl)
    return d_out.to_host()


def check(ctxs, name, nl, C, B, **env):
    cts, evks, want = case(ctxs.oracle(name), name, nl, C, B)
    assert np.array_equal(gpu_sum(ctxs(name, **env), cts, evks, nl), want)


@gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 2, 8])
def test_two_digits_of_two(ctxs, C, B):
    check(ctxs, "l4d2", 4, C, B)


@gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [2, 8])
def test_three_digits_of_two(ctxs, C, B):
    check(ctxs, "l6d3", 6, C, B)


@gpu
def test_q0_and_three_fp64_sources(ctxs):
    check(ctxs, "l8d2", 8, 2, 1)


@gpu
def test_second_client_group(ctxs):
    """Groups of 2 with 3 clients: the second group's sums are added to `out`."""
    check(ctxs, "l4d2", 4, 3, 1, MKCKKS_QSUM_GROUP="2")


@gpu
@pytest.mark.parametrize("name,nl", [("l6d3", 5), ("l4d2", 3), ("l8d2", 6)])
def test_reduced_level_with_a_partial_last_digit(ctxs, name, nl):
    check(ctxs, name, nl, 2, 1)


def pattern_case(o, nl, kind):
    """Two clients.  `max`: every residue of the ciphertexts and keys q - 1; `alt`: alternating 0 / q - 1; `zero`: client
    0's ciphertext all zero (its P-limb coefficients are the canonical 0) beside a random client 1, random keys."""
    key = ("pattern", id(o), nl, kind)
    if key not in _cases:
        rng = np.random.default_rng(77 + nl)
        if kind == "zero":
            cts = rand_polys(rng, o, list(range(nl)) * 2, 2).reshape(2, 1, 2, nl, o.N)
            cts[0] = 0
            evks = rand_polys(rng, o, list(range(o.D)) * (2 * o.beta), 2).reshape(2, o.beta, 2, o.D, o.N)
        else:
            mask = (np.arange(o.N) % 2 == 0) if kind == "alt" else np.ones(o.N, dtype=bool)
            cts = np.zeros((2, 1, 2, nl, o.N), dtype=np.uint64)
            evks = np.zeros((2, o.beta, 2, o.D, o.N), dtype=np.uint64)
            for l in range(nl):
                cts[:, :, :, l, mask] = int(o.moduli[l]) - 1
            for l in range(o.D):
                evks[:, :, :, l, mask] = int(o.moduli[l]) - 1
        want = oracle_chain(o, cts, evks)
        for a in (cts, evks, want):
            a.setflags(write=False)
        _cases[key] = (cts, evks, want)
    return _cases[key]


@gpu
@pytest.mark.parametrize("kind", ["max", "alt", "zero"])
@pytest.mark.parametrize("name,nl", [("l4d2", 4), ("l6d3", 6)])
def test_operand_patterns(ctxs, name, nl, kind):
    cts, evks, want = pattern_case(ctxs.oracle(name), nl, kind)
    assert np.array_equal(gpu_sum(ctxs(name), cts, evks, nl), want)


@gpu
def test_all_zero_inputs_give_zero(ctxs):
    o = ctxs.oracle("l4d2")
    cts = np.zeros((2, 1, 2, 4, o.N), dtype=np.uint64)
    evks = case(o, "l4d2", 4, 2, 1)[1]
    assert not gpu_sum(ctxs("l4d2"), cts, evks, 4).any()


@gpu
@pytest.mark.parametrize("kind", ["rand", "max", "zero"])
def test_shoup_instances(ctxs, kind):
    """MKCKKS_NO_PM=1: q_0 and the P limbs on the Shoup butterflies, whose inverse round ends below 2p."""
    o = ctxs.oracle("l6d3")
    cts, evks, want = case(o, "l6d3", 6, 2, 3) if kind == "rand" else pattern_case(o, 6, kind)
    assert np.array_equal(gpu_sum(ctxs("l6d3", MKCKKS_NO_PM="1"), cts, evks, 6), want)


@gpu
def test_integer_only(ctxs):
    """MKCKKS_NO_FP64=1: no fp64-class limb, so the call takes the per-client loop with the unscaled tables."""
    check(ctxs, "l4d2", 4, 2, 1, MKCKKS_NO_FP64="1")


@gpu
def test_512_point_rows(ctxs):
    check(ctxs, "n17", 4, 2, 1)


@gpu
def test_weighted_instance(ctxs):
    """reencrypt_wsum scales the keys (P limbs included) before the merged flow."""
    from tests.test_weighted_aggregation import device_wsum, oracle_wsum, rand_evks, scaled_evk
    from tests.test_gpu_parity import rand_ct
    name, nl, C, B = "l4d2", 4, 3, 2
    o = ctxs.oracle(name)
    rng = np.random.default_rng(59)
    cts = np.stack([rand_ct(rng, o, nl, B) for _ in range(C)])
    evks = rand_evks(rng, o, C)
    weights, sf_level = [0.3125, 2.5, 0.123456789], o.L - nl + 1
    evks_s = [scaled_evk(o, evks[c], weights[c], sf_level) for c in range(C)]
    want = np.stack([oracle_wsum(o, cts, evks_s, weights, sf_level, b) for b in range(B)])
    got, _ = device_wsum(ctxs(name), cts, evks, weights, sf_level, nl)
    assert np.array_equal(got, want)


# ---- the flows that keep the unscaled tables and the scale in their inverse column pass ------------------------------------
@gpu
def test_single_reencrypt_is_untouched(ctxs):
    g, o = ctxs("l4d2"), ctxs.oracle("l4d2")
    cts, evks, _ = case(o, "l4d2", 4, 2, 3)
    d_out = g.empty((3, 2, 4, g.N))
    g.reencrypt(g.to_device(cts[0]), g.to_device(evks[0]), d_out, 3, 4)
    got = d_out.to_host()
    for b in range(3):
        assert np.array_equal(got[b], o.reencrypt(cts[0, b], evks[0])), b


@gpu
def test_fanout_is_untouched(ctxs):
    g, o = ctxs("l4d2"), ctxs.oracle("l4d2")
    cts, evks, _ = case(o, "l4d2", 4, 2, 3)
    d_out = g.empty((2, 3, 2, 4, g.N))
    g.reencrypt_fanout(g.to_device(cts[0]), g.to_device(evks), d_out, 2, 3, 4)
    got = d_out.to_host()
    for k in range(2):
        for b in range(3):
            assert np.array_equal(got[k, b], o.reencrypt(cts[0, b], evks[k])), (k, b)


@gpu
def test_modup_digits_are_the_oracles(ctxs):
    """The `modup` entry point converts with the unscaled tables: its P limbs are the oracle's digits."""
    from oracle.oracle import OracleContext
    g = ctxs("l4d2")
    a = PARAMS["l4d2"]
    o = OracleContext(a[0], a[1], a[2], a[3], dnum=a[4])
    rng = np.random.default_rng(11)
    for nl in (4, 3):
        c1 = rand_polys(rng, g, list(range(nl)), 2)
        c1[0, :, ::5] = (np.asarray(g.moduli[:nl], dtype=np.uint64) - np.uint64(1))[:, None]
        d_dig = g.empty((2, g.num_parts(nl), nl + g.K, g.N))
        g.modup(g.to_device(c1), d_dig, 2, nl)
        dig = d_dig.to_host()
        for b in range(2):
            assert np.array_equal(dig[b], o.modup_digits(c1[b])), (nl, b)
