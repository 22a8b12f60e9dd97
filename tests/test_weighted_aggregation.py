"""Weighted aggregation on the GPU: per-client weights folded into the key switch (include/mkckks.h).

The weighted sum is DEFINED as  sum_c ReEncrypt((M_c c0_c, c1_c), M_c evk_c)  with M_c = trunc(w_c sf(sf_level) + 0.5), so
the expected residues are the oracle's EvalAdd chain over the clients of o.reencrypt on the scaled inputs: bit-exact on
every path (merged n-client flow, client groups, workspace chunks, the composition outside the merged flow).  The
precision test runs real encode / encrypt / rekeygen inputs through the weighted calls and one rescale and compares the
decoded aggregate with the plaintext weighted mean and with OpenFHE's order (per client ReEncrypt -> rescale ->
EvalMult(w_c), then EvalAdd).

Measured on an MI355X (profiles/weighted_ab.txt): err_new 2^-42.01, err_chain 2^-26.71 (the CPU oracle gives the same pair:
the device result is bit-identical to it).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.oracle import OracleContext, sample_gauss, sample_ternary  # noqa: E402
from tests.test_gpu_parity import CONFIGS, make_keys, make_rk_rand, rand_ct, rand_polys  # noqa: E402

WEIGHTS = [0.0, 1.0, 0.3125, 0.123456789, 2.5, 1.0 / 3.0, 0.07, 0.5, 0.015625]  # 0, 1 and uneven values


@pytest.fixture(scope="module")
def ctxs():
    from ppqsflhe_amd import Context
    cache = {}

    def get(name):
        if name not in cache:
            a = CONFIGS[name]
            cache[name] = (Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0),
                           OracleContext(a[0], a[1], a[2], a[3], dnum=a[4]))
        return cache[name]

    yield get
    for g, _ in cache.values():
        g.close()


def rand_evks(rng, g, C):
    return np.stack([rand_polys(rng, g, list(range(g.D)) * (2 * g.beta), 1).reshape(g.beta, 2, g.D, g.N) for _ in range(C)])


def scaled_evk(o, evk, w, sf_level):
    f = o.const_factors(o.D, sf_level, w)
    return np.stack([o.mult_factors(evk[j], f) for j in range(o.beta)])


def scaled_c0(o, ct, w, sf_level):
    out = ct.copy()
    out[0] = o.mult_factors(ct, o.const_factors(ct.shape[1], sf_level, w))[0]
    return out


def oracle_wsum(o, cts, evks_scaled, weights, sf_level, b):
    """EvalAdd chain over the clients of ReEncrypt((M_c c0, c1), M_c evk) for ciphertext index b."""
    acc = None
    for c, w in enumerate(weights):
        r = o.reencrypt(scaled_c0(o, cts[c, b], w, sf_level), evks_scaled[c])
        acc = r if acc is None else o.eval_add(acc, r)
    return acc


def device_wsum(g, cts, evks, weights, sf_level, nl):
    C, B = cts.shape[:2]
    d_evks, d_scaled = g.to_device(evks), g.empty(evks.shape)
    g.scale_evk(d_evks, d_scaled, C, weights, sf_level)
    d_out = g.empty((B, 2, nl, g.N))
    g.reencrypt_wsum(g.to_device(cts), d_scaled, d_out, C, B, nl, weights, sf_level)
    return d_out.to_host(), d_scaled


def check_wsum(g, o, nl, C, B, seed=31):
    rng = np.random.default_rng(seed)
    cts = np.stack([rand_ct(rng, g, nl, B) for _ in range(C)])
    evks = rand_evks(rng, g, C)
    weights = (WEIGHTS * 2)[:C]
    sf_level = g.L - nl + 1  # noiseScaleDeg-2 inputs at level L - nl
    got, _ = device_wsum(g, cts, evks, weights, sf_level, nl)
    evks_s = [scaled_evk(o, evks[c], weights[c], sf_level) for c in range(C)]
    for b in sorted({0, 1 % B, B - 1}):  # first chunk, and the last index (the second chunk when there is one)
        assert np.array_equal(got[b], oracle_wsum(o, cts, evks_s, weights, sf_level, b)), (nl, C, B, b)


@pytest.mark.parametrize("name,nl,C,B", [
    ("ref", 4, 3, 2),                      # merged flow: fp64 limbs + q_0 tail + P
    ("ref", 4, 9, 2),                      # second client group: the init_from_out prologue must use the plain P
    ("ref", 4, 3, 19),                     # second workspace chunk
    ("ref", 2, 2, 2), ("ref", 3, 1, 1),    # single digit, partial last digit
    ("c3", 12, 3, 1), ("c3", 11, 2, 2),    # three digits; a reduced level changes sf_level
    ("n17", 4, 3, 1),                      # 512-point rows
    ("tiny", 5, 3, 2), ("n11", 4, 2, 1), ("c5s", 20, 2, 1)])  # composition path
def test_reencrypt_wsum_matches_the_oracle(ctxs, name, nl, C, B):
    g, o = ctxs(name)
    check_wsum(g, o, nl, C, B)


@pytest.mark.parametrize("env", [{"MKCKKS_QSUM_GROUP": "2"}, {"MKCKKS_NO_PM": "1"}, {"MKCKKS_NO_FP64": "1"}])
def test_reencrypt_wsum_under_the_library_switches(ctxs, monkeypatch, env):
    from ppqsflhe_amd import Context
    _, o = ctxs("ref")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a = CONFIGS["ref"]
    g = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)
    try:
        check_wsum(g, o, 4, 3, 2)
    finally:
        g.close()


def test_reencrypt_wsum_extreme_residues(ctxs):
    """Every ciphertext and key residue q - 1, weight 1.0 (M = sf: the largest products the kernels meet)."""
    g, o = ctxs("ref")
    nl, C, B = 4, 3, 1
    cts = np.zeros((C, B, 2, nl, g.N), dtype=np.uint64)
    evks = np.zeros((C, g.beta, 2, g.D, g.N), dtype=np.uint64)
    for l in range(nl):
        cts[:, :, :, l, :] = int(g.moduli[l]) - 1
    for l in range(g.D):
        evks[:, :, :, l, :] = int(g.moduli[l]) - 1
    weights, sf_level = [1.0] * C, g.L - nl + 1
    got, _ = device_wsum(g, cts, evks, weights, sf_level, nl)
    evks_s = [scaled_evk(o, evks[c], 1.0, sf_level) for c in range(C)]
    assert np.array_equal(got[0], oracle_wsum(o, cts, evks_s, weights, sf_level, 0))


@pytest.mark.parametrize("name,nl", [("ref", 4), ("tiny", 5)])
def test_wsum_equals_plain_sum_of_host_scaled_inputs(ctxs, name, nl):
    """On the device: reencrypt_wsum(cts, scale_evk(evks)) == reencrypt_sum(cts', scale_evk(evks)), c0 scaled on the host."""
    g, o = ctxs(name)
    C, B = 3, 2
    rng = np.random.default_rng(8)
    cts = np.stack([rand_ct(rng, g, nl, B) for _ in range(C)])
    evks = rand_evks(rng, g, C)
    weights, sf_level = [0.25, 1.75, 0.0], g.L - nl + 1
    got, d_scaled = device_wsum(g, cts, evks, weights, sf_level, nl)
    cts_s = np.stack([np.stack([scaled_c0(o, cts[c, b], weights[c], sf_level) for b in range(B)]) for c in range(C)])
    d_ref = g.empty((B, 2, nl, g.N))
    g.reencrypt_sum(g.to_device(cts_s), d_scaled, d_ref, C, B, nl)
    assert np.array_equal(got, d_ref.to_host())


@pytest.mark.parametrize("name", ["tiny", "ref"])
def test_scale_evk_matches_the_oracle_on_all_limbs(ctxs, name):
    g, o = ctxs(name)
    rng = np.random.default_rng(3)
    C = 3
    evks = rand_evks(rng, g, C)
    weights = [0.0, 1.0, 0.3125]
    for sf_level in (1, g.L - 1):
        d_out = g.empty(evks.shape)
        g.scale_evk(g.to_device(evks), d_out, C, weights, sf_level)
        got = d_out.to_host()
        for c in range(C):
            assert np.array_equal(got[c], scaled_evk(o, evks[c], weights[c], sf_level)), (name, sf_level, c)
    assert not got[0].any()  # weight 0.0


@pytest.fixture(scope="module")
def wsum_terms(ctxs):
    """17 random terms at `tiny` and their products with the weight constants, computed once."""
    g, o = ctxs("tiny")
    rng = np.random.default_rng(12)
    nl, B, n = g.L, 2, 17
    terms = np.stack([rand_ct(rng, g, nl, B) for _ in range(n)])
    weights = (WEIGHTS * 2)[:n]
    sf_level = 1
    prods = np.stack([np.stack([o.mult_factors(terms[k, b], o.const_factors(nl, sf_level, weights[k])) for b in range(B)])
                      for k in range(n)])
    return terms, weights, sf_level, prods


@pytest.mark.parametrize("n_terms", [1, 3, 9, 17])  # the sums are reduced every 4 terms: below, across, many times
@pytest.mark.parametrize("first_is_sum", [False, True])
def test_eval_wsum(ctxs, wsum_terms, n_terms, first_is_sum):
    g, o = ctxs("tiny")
    terms, weights, sf_level, prods = wsum_terms
    nl, B = g.L, terms.shape[1]
    d_out = g.empty((B, 2, nl, g.N))
    g.eval_wsum(g.to_device(terms[:n_terms]), d_out, n_terms, B, nl, weights[:n_terms], sf_level, first_is_sum)
    got = d_out.to_host()
    for b in range(B):
        acc = terms[0, b] if first_is_sum else prods[0, b]
        for k in range(1, n_terms):
            acc = o.eval_add(acc, prods[k, b])
        assert np.array_equal(got[b], acc), (n_terms, first_is_sum, b)


def test_eval_wsum_in_place_on_term_zero(ctxs, wsum_terms):
    g, o = ctxs("tiny")
    terms, weights, sf_level, prods = wsum_terms
    nl, B, n = g.L, terms.shape[1], 3
    d_in = g.to_device(terms[:n])
    g.eval_wsum(d_in, d_in, n, B, nl, weights[:n], sf_level, True)
    got = d_in.to_host()[0]
    for b in range(B):
        assert np.array_equal(got[b], o.eval_add(o.eval_add(terms[0, b], prods[1, b]), prods[2, b]))


def test_aliasing_and_bad_weights_are_refused(ctxs):
    from ppqsflhe_amd import MkckksError
    g, _ = ctxs("tiny")
    nl, C, B = g.L, 2, 1
    d_evks, d_scaled = g.empty((C, g.beta, 2, g.D, g.N)), g.empty((C, g.beta, 2, g.D, g.N))
    d_cts, d_out = g.empty((C, B, 2, nl, g.N)), g.empty((B, 2, nl, g.N))
    ok = [0.5, 0.5]

    def refused(call):
        with pytest.raises(MkckksError) as ei:
            call()
        assert ei.value.code == -1

    refused(lambda: g.scale_evk(d_evks, d_evks, C, ok, 1))                       # output over input
    refused(lambda: g.scale_evk(d_evks, d_evks.ptr + 8 * g.N, C, ok, 1))         # output starting inside the input
    refused(lambda: g.reencrypt_wsum(d_cts, d_scaled, d_cts, C, B, nl, ok, 1))   # output over client 0
    refused(lambda: g.eval_wsum(d_cts, d_cts.ptr + 8 * g.N, C, B, nl, ok, 1))    # output inside the terms, not term 0
    for bad in (float("nan"), float("inf"), -float("inf"), 1e30):                # 1e30 * 2^40 does not fit 125 bits
        refused(lambda: g.scale_evk(d_evks, d_scaled, C, [0.5, bad], 1))
        refused(lambda: g.reencrypt_wsum(d_cts, d_scaled, d_out, C, B, nl, [bad, 0.5], 1))
        refused(lambda: g.eval_wsum(d_cts, d_out, C, B, nl, [0.5, bad], 1))
    refused(lambda: g.scale_evk(d_evks, d_scaled, C, ok, 1000))                  # no such scaling-factor level
    g.eval_wsum(d_cts, d_out, C, B, nl, [float("nan"), 0.5], 1, True)            # h_weights[0] is ignored with first_is_sum
    # zero counts are no-ops
    g.scale_evk(d_evks, d_scaled, 0, [], 1)
    g.reencrypt_wsum(d_cts, d_scaled, d_out, 0, B, nl, [], 1)
    g.reencrypt_wsum(d_cts, d_scaled, d_out, C, 0, nl, ok, 1)
    g.eval_wsum(d_cts, d_out, 0, B, nl, [], 1)
    g.sync()


# ---- precision: the reference's parameters, real inputs ----------------------------------------------------------------

def test_weighted_mean_precision_against_the_openfhe_order(ctxs, golden_dir):
    """Three re-keyed clients + one in-domain client, weights 5 : 3 : 2 : 7.  New order (multiply, sum, ONE rescale) on the
    device against the per-client chain ReEncrypt -> rescale -> EvalMult(w_c) -> EvalAdd on the oracle, both decoded with
    the same scale.  Required: err_new < 2^-25 (the project's bar for decoded doubles at these parameters) and
    err_new <= 2 err_chain (the factor 2 allows for the different rounding order)."""
    g, o = ctxs("ref")
    W = np.load(os.path.join(golden_dir, "e2e_weights.npz"))
    rng = np.random.default_rng(41)
    N, L, slots = g.N, g.L, g.N // 2
    vals = np.stack([W["sample_c1_param_1_values"], W["sample_c2_param_1_values"],
                     np.resize(W["sample_c1_param_0_values"], slots), np.resize(W["sample_c1_param_6_values"], slots)])
    counts = np.array([5.0, 3.0, 2.0, 7.0])
    w = counts / counts.sum()
    mean = (w[:, None] * vals).sum(axis=0)
    keys = []
    for _ in range(4):
        s, a, e = make_keys(o, rng)
        pk, sk = o.keygen(s, a, e)
        keys.append((s, pk, sk))
    tgt = 3
    cts = np.stack([o.encrypt(keys[c][1], o.encode(vals[c], o.sf_big(0), L), sample_ternary(rng, N), sample_gauss(rng, N),
                              sample_gauss(rng, N)) for c in range(4)])
    evks = np.stack([o.rekeygen(keys[c][0], keys[tgt][1], *make_rk_rand(o, rng)) for c in range(3)])
    scale = o.sf_big(0) / float(o.moduli[L - 1]) * o.sf(1)
    # the OpenFHE order on the oracle
    chain = None
    for c in range(4):
        ct = o.reencrypt(cts[c], evks[c]) if c != tgt else cts[c]
        ct = o.mult_factors(o.rescale(ct), o.const_factors(L - 1, 1, w[c]))
        chain = ct if chain is None else o.eval_add(chain, ct)
    err_chain = np.abs(o.decrypt_decode(chain, keys[tgt][2], scale) - mean).max()
    # the weighted calls on the device: [slot of the re-keyed clients' sum][the in-domain client] -> eval_wsum -> rescale
    d_scaled = g.empty(evks.shape)
    g.scale_evk(g.to_device(evks), d_scaled, 3, w[:3], 1)
    d_terms = g.empty((2, 1, 2, L, N))
    d_terms.view(2 * L * N, (1, 2, L, N)).upload(cts[tgt][None])
    g.reencrypt_wsum(g.to_device(cts[:3, None]), d_scaled, d_terms, 3, 1, L, w[:3], 1)
    d_sum = g.empty((1, 2, L, N))
    g.eval_wsum(d_terms, d_sum, 2, 1, L, [0.0, w[tgt]], 1, True)
    d_agg = g.empty((1, 2, L - 1, N))
    g.rescale(d_sum, d_agg, 1, L)
    d_m, d_vals = g.empty((1, L - 1, N)), g.empty((1, slots), dtype=np.float64)
    g.decrypt(d_agg, g.to_device(keys[tgt][2]), d_m, 1, L - 1)
    g.decode(d_m, d_vals, 1, L - 1, scale)
    err_new = np.abs(d_vals.to_host()[0] - mean).max()
    print(f"weighted mean, ref context, weights 5:3:2:7: err_new 2^{np.log2(err_new):.2f}, err_chain 2^{np.log2(err_chain):.2f}")
    # the device result is the oracle's, bit for bit, on the real inputs too
    exp = oracle_wsum(o, cts[:3, None], [scaled_evk(o, evks[c], w[c], 1) for c in range(3)], w[:3], 1, 0)
    exp = o.rescale(o.eval_add(exp, o.mult_factors(cts[tgt], o.const_factors(L, 1, w[tgt]))))
    assert np.array_equal(d_agg.to_host()[0], exp)
    assert err_new < 2.0 ** -25, (err_new, err_chain)
    assert err_new <= 2 * err_chain, (err_new, err_chain)
