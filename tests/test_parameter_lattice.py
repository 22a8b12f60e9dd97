"""The parameter ranges `mkckks_ctx_create` accepts, beyond the handful of points the feature tests are built from.

ParamSet::generate admits log_n 8..17, scaling_bits 20..59, first_bits up to 60, aux_bits 30..60, extra_bits 18..30 and
any dnum with digit size and special-prime count <= 8; from the moduli the engine picks an arithmetic class per limb
(`Context.arith`: 0 Shoup/Barrett, 1 fp64-FMA, 2 pseudo-Mersenne) and the transform kernels (radix on both passes at
log_n 12, 14, 16, 17; a generic LDS-stage pass, integer only, elsewhere).  TABLE below holds one context per region of
that space no other test creates, with the classes it must land in.

CPU (`-m "not gpu"`): the library's moduli and digit structure against the oracle's, for the table and for a sweep of
every accepted width at log_n = 12; the refusal of a digit size of 9 and of parameters whose moduli repeat.

GPU (`-m gpu`): the class assertion first, so that an entry which drifts out of its region fails instead of re-testing
the default path, then one battery per entry.  Everything is compared word for word (np.array_equal) with the oracle;
the one floating-point comparison is the decode, within the 2^-40 of test_gpu_parity.test_encode_decode_on_device: both
sides decode the same integers, so the bound does not depend on the scale.  Inputs and oracle results of the key-switch
step are computed once per entry (`ks_case`) and shared with the switch tests.

The entry points added since (plaintext products, weighted aggregation, rotations, ciphertext products, collective keys,
the share protocols, linear transforms) run on the same table in tests/test_lattice_evaluation.py; polynomial and Chebyshev
evaluation (poly_tensor, cheb_tensor, affine, the two ladders, poly_eval and cheb_eval) in tests/test_lattice_poly.py."""
import numpy as np
import pytest

from oracle.oracle import OracleContext, sample_gauss, sample_ternary
from tests.test_compact_downlink import compress, fanout_compact, prefix
from tests.test_gpu_parity import make_keys, make_rk_rand, rand_ct, rand_polys
from tests.test_reencrypt_fanout import fanout, rand_evks
from tests.test_rerandomize import exact_rerandomize, rerandomize, wide_inputs
from tests.test_threshold_decrypt import exact_share, partial_decrypt, rand_sk, wide_errors

SHOUP, FP64, PM = 0, 1, 2


def _classes(L, K, p):
    """a pseudo-Mersenne q_0, L - 1 fp64 limbs of Q, K limbs of P of class p"""
    return [PM] + [FP64] * (L - 1) + [p] * K


# name: ((log_n, depth, scaling_bits, first_bits, dnum, aux_bits, extra_bits), (L, K, alpha, beta), arith per limb)
TABLE = {
    # scaling limbs of 52..60 bits: not 2^k - c with small c, so the whole context leaves the pseudo-Mersenne class --
    # q_0 and P on Shoup next to the fp64 extra limb (N = 2^16: the integer fused key-switch kernels + an fp64 instance)
    "s51": ((12, 2, 51, 60, 2, 60, 20), (4, 2, 2, 2), [0, 0, 0, 1, 0, 0]),
    "s54": ((12, 2, 54, 60, 2, 60, 20), (4, 2, 2, 2), [0, 0, 0, 1, 0, 0]),
    "s59": ((12, 2, 59, 60, 2, 60, 20), (4, 2, 2, 2), [0, 0, 0, 1, 0, 0]),
    "s55n14": ((14, 3, 55, 60, 2, 60, 20), (5, 3, 3, 2), [0, 0, 0, 0, 1, 0, 0, 0]),
    "s56n16": ((16, 2, 56, 60, 3, 60, 20), (4, 2, 2, 2), [0, 0, 0, 1, 0, 0]),
    # fp64 limbs of other widths than 20, 40/41, 50/51 bits
    "s30": ((12, 3, 30, 60, 2, 60, 20), (5, 3, 3, 2), [2, 1, 1, 1, 1, 2, 2, 2]),
    "s21n16": ((16, 2, 21, 60, 2, 60, 20), (4, 2, 2, 2), [2, 1, 1, 1, 2, 2]),  # s20n16 is refused: REFUSED below
    "s24n17": ((17, 2, 24, 60, 2, 60, 20), (4, 2, 2, 2), [2, 1, 1, 1, 2, 2]),
    # q_0 an fp64 limb; q_0 a pseudo-Mersenne limb of 52 bits
    "f40": ((12, 2, 24, 40, 2, 60, 20), (4, 2, 2, 2), [1, 1, 1, 1, 2, 2]),
    "f45": ((12, 2, 40, 45, 2, 60, 20), (4, 2, 2, 2), [1, 1, 1, 1, 2, 2]),
    "f52": ((12, 2, 40, 52, 2, 60, 20), (4, 2, 2, 2), [2, 1, 1, 1, 2, 2]),
    # P limbs on fp64 (K = 3, K = 4 > alpha), P limbs of 55 bits; extra limbs of 18 and 30 bits.  (a45, a30e18 and al8k8
    # found the single-key key switch handing fp64-class P limbs to its integer kernels: reencrypt differed in every word)
    "a45": ((12, 2, 40, 60, 2, 45, 20), (4, 3, 2, 2), [2, 1, 1, 1, 1, 1, 1]),
    "a55": ((12, 2, 40, 60, 2, 55, 20), (4, 2, 2, 2), [2, 1, 1, 1, 2, 2]),
    "a30e18": ((12, 2, 40, 60, 2, 30, 18), (4, 4, 2, 2), [2, 1, 1, 1, 1, 1, 1, 1]),
    "e30": ((12, 2, 40, 60, 2, 60, 30), (4, 2, 2, 2), [2, 1, 1, 1, 2, 2]),
    # digit sizes 8 (one digit), 1, 5 (first size on the four-column accumulator), 8; K = 8
    "d1": ((12, 6, 40, 60, 1, 60, 20), (8, 6, 8, 1), _classes(8, 6, PM)),
    "dL": ((12, 4, 40, 60, 6, 60, 20), (6, 1, 1, 6), [2, 1, 1, 1, 1, 1, 2]),
    "al5": ((12, 8, 40, 60, 2, 60, 20), (10, 4, 5, 2), _classes(10, 4, PM)),
    "al8": ((12, 14, 40, 60, 2, 60, 20), (16, 6, 8, 2), _classes(16, 6, PM)),
    "al8k8": ((12, 14, 40, 60, 2, 48, 20), (16, 8, 8, 2), _classes(16, 8, FP64)),  # aux_bits 49 still gives K = 7
    # the deepest chain generate() accepts: L = 32 = CRT_MAX_LIMBS (decode's private digit array is full), four digits of 8
    # with K = 7; the battery's nl = L, L - 1 (a last digit of 7) and 1 cover the full level, a partial digit and one limb
    "d30": ((12, 30, 50, 60, 4, 60, 20), (32, 7, 8, 4), _classes(32, 7, PM)),
    # one pass radix and one generic (2^13, 2^15), both generic at the smallest ring: integer arithmetic only
    "r8": ((8, 3, 50, 60, 2, 60, 20), (5, 3, 3, 2), [0] * 8),
    "r13": ((13, 2, 50, 60, 2, 60, 20), (4, 2, 2, 2), [0] * 6),
    "r15": ((15, 2, 50, 60, 3, 60, 20), (4, 2, 2, 2), [0] * 6),
}
NAMES = list(TABLE)
# Accepted ranges, yet no basis: the extra limb (the first prime = 1 mod 2N above 2^(extra_bits - 1)) is a scaling limb
# once more.  s20n16 was a table entry: 786433 twice, every rescale failed with "h_invmod: not invertible".
REFUSED = {"s20n16": (16, 2, 20, 60, 2, 60, 20), "e25s24": (12, 2, 24, 60, 2, 60, 25), "e30s29n17": (17, 1, 29, 60, 2, 60, 30)}
# the arithmetic the switches fall back to, on contexts whose limb widths no other switch test has: the same bits
SWITCHED = [("s54", "MKCKKS_NO_FP64", FP64), ("f45", "MKCKKS_NO_FP64", FP64), ("a30e18", "MKCKKS_NO_FP64", FP64),
            ("al8", "MKCKKS_NO_FP64", FP64), ("f52", "MKCKKS_NO_PM", PM), ("a55", "MKCKKS_NO_PM", PM)]


def _kwargs(a):
    return dict(first_bits=a[3], dnum=a[4], aux_bits=a[5], extra_bits=a[6])


_ORACLES = {}


def oracle(name):
    if name not in _ORACLES:
        a = TABLE[name][0]
        _ORACLES[name] = OracleContext(a[0], a[1], a[2], **_kwargs(a))
    return _ORACLES[name]


# ---- CPU: parameter generation against the oracle -------------------------------------------------------------------

def _host_matches_oracle(a):
    from ppqsflhe_amd import Context
    c = Context(a[0], a[1], a[2], device=-1, **_kwargs(a))
    try:
        o = OracleContext(a[0], a[1], a[2], **_kwargs(a))
        assert np.array_equal(c.moduli, o.moduli), a
        assert len(set(c.moduli.tolist())) == c.D, a
        assert (c.N, c.L, c.K, c.alpha, c.beta) == (o.N, o.L, o.K, o.alpha, o.beta), a
        return c.L, c.K, c.alpha, c.beta
    finally:
        c.close()


@pytest.mark.parametrize("name", NAMES)
def test_table_entry_on_a_host_only_context(name):
    args, shape, arith = TABLE[name]
    assert _host_matches_oracle(args) == shape
    assert len(arith) == shape[0] + shape[1]


def test_moduli_match_the_oracle_over_every_accepted_width():
    for sbits in range(20, 60):
        _host_matches_oracle((12, 2, sbits, 60, 2, 60, 20))
    for fbits in range(41, 61):
        _host_matches_oracle((12, 2, 40, fbits, 2, 60, 20))
    for abits in range(30, 61):
        _host_matches_oracle((12, 2, 40, 60, 2, abits, 20))
    for ebits in range(18, 31):
        _host_matches_oracle((12, 2, 40, 60, 2, 60, ebits))


@pytest.mark.parametrize("name", list(REFUSED))
def test_repeated_moduli_are_refused(name):
    from ppqsflhe_amd import Context, MkckksError
    a = REFUSED[name]
    moduli = [int(q) for q in OracleContext(a[0], a[1], a[2], **_kwargs(a)).moduli]
    assert len(set(moduli)) < len(moduli)  # the reference's generator repeats a prime here
    with pytest.raises(MkckksError, match="moduli are not pairwise distinct") as ei:
        Context(a[0], a[1], a[2], device=-1, **_kwargs(a))
    assert ei.value.code == -1


def test_k8_entry_is_the_first_aux_width_with_eight_special_primes():
    a = TABLE["al8"][0]
    assert [OracleContext(a[0], a[1], a[2], **_kwargs(a[:5] + (b, 20))).K for b in (49, 48)] == [7, 8]


def test_digit_size_nine_is_refused():
    from ppqsflhe_amd import Context, MkckksError
    with pytest.raises(MkckksError):
        Context(12, 7, 40, 60, dnum=1, device=-1)  # L = 9 in one digit


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctxs():
    from ppqsflhe_amd import Context
    cache = {}

    def get(name):
        args, shape, arith = TABLE[name]
        if name not in cache:
            cache[name] = Context(args[0], args[1], args[2], device=0, **_kwargs(args))
        g = cache[name]
        # the class assertion comes first, for every test: what follows tests the region the entry was written for
        assert [int(x) for x in g.arith] == arith, (name, list(g.arith))
        assert (g.L, g.K, g.alpha, g.beta) == shape, name
        assert np.array_equal(g.moduli, oracle(name).moduli), name
        return g, oracle(name)

    yield get
    for g in cache.values():
        g.close()


def _batch(g):
    return 2 if g.N <= 1 << 14 else 1


def _extreme_polys(g, ids):
    """[3][len(ids)][N]: every residue q - 1, alternating 0 / q - 1 with periods 1 and N / 2"""
    idx = np.arange(g.N)
    x = np.zeros((3, len(ids), g.N), dtype=np.uint64)
    for pi, m in enumerate((np.ones(g.N, dtype=bool), idx % 2 == 0, (idx // (g.N // 2)) % 2 == 0)):
        for j, l in enumerate(ids):
            x[pi, j, m] = int(g.moduli[l]) - 1
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_transforms_and_rescaling(ctxs, name):
    g, o = ctxs(name)
    rng = np.random.default_rng(101)
    N, L, D = g.N, g.L, g.D
    ids = list(range(D))
    x = np.concatenate([rand_polys(rng, g, ids, 1), _extreme_polys(g, ids)])
    P = x.shape[0]
    d = g.to_device(x)
    g.ntt_forward(d, P, L, with_p=True)
    fwd = d.to_host()
    for p in range(P):
        for l in ids:
            assert np.array_equal(fwd[p, l], o.ntt_fwd(l, x[p, l])), (name, "forward", p, l)
    g.ntt_inverse(d, P, L, with_p=True)
    assert np.array_equal(d.to_host(), x), (name, "round trip")
    g.ntt_inverse(d, P, L, with_p=True)
    inv = d.to_host()
    for p in range(P):
        for l in ids:
            assert np.array_equal(inv[p, l], o.ntt_inv(l, x[p, l])), (name, "inverse", p, l)
    # rescale, rescale * constant, * constant: at the top level and at the lowest one that can be rescaled
    B = 2
    for nl in (L, 2):
        ct = rand_ct(rng, g, nl, B)
        ct[1, :, :, ::3] = (g.moduli[:nl] - np.uint64(1))[None, :, None]
        d_in, d_out = g.to_device(ct), g.empty((B, 2, nl - 1, N))
        g.rescale(d_in, d_out, B, nl)
        got = d_out.to_host()
        exp = [o.rescale(ct[b]) for b in range(B)]
        for b in range(B):
            assert np.array_equal(got[b], exp[b]), (name, "rescale", nl, b)
        level = L - (nl - 1)
        for operand in (1.0 / 3, -0.25):
            f = o.const_factors(nl - 1, level, operand)
            g.rescale_mult_const(d_in, d_out, B, nl, operand)
            got = d_out.to_host()
            for b in range(B):
                assert np.array_equal(got[b], o.mult_factors(exp[b], f)), (name, "rescale_mult_const", nl, operand, b)
            d_r = g.to_device(np.stack(exp))
            g.mult_const(d_r, B, nl - 1, operand)
            got = d_r.to_host()
            for b in range(B):
                assert np.array_equal(got[b], o.mult_factors(exp[b], f)), (name, "mult_const", nl, operand, b)


# ---- the key-switch step: inputs and oracle results once per entry --------------------------------------------------

_KS = {}


def _oracle_sum(o, cts, evks, b):
    acc = o.reencrypt(cts[0, b], evks[0])
    for c in range(1, cts.shape[0]):
        acc = o.eval_add(acc, o.reencrypt(cts[c, b], evks[c]))
    return acc


def ks_case(name):
    """reencrypt at nl = L and L - 1 (B ciphertexts, one key), reencrypt_sum with C = 3 on random inputs and with C = 2 on
    extreme ones (client 0: every residue of ciphertext and key q - 1; client 1: alternating 0 / q - 1)."""
    if name not in _KS:
        o = oracle(name)
        rng = np.random.default_rng(202)
        N, L, D = o.N, o.L, o.D
        B = _batch(o)
        case = dict(B=B, evk=rand_evks(rng, o, 1)[0])
        for nl in (L, L - 1):
            ct = rand_ct(rng, o, nl, B)
            case["ct", nl] = ct
            case["one", nl] = np.stack([o.reencrypt(ct[b], case["evk"]) for b in range(B)])
        cts, evks = np.stack([rand_ct(rng, o, L, B) for _ in range(3)]), rand_evks(rng, o, 3)
        case["cts"], case["evks"] = cts, evks
        case["sum"] = np.stack([_oracle_sum(o, cts, evks, b) for b in range(B)])
        x_cts, x_evks = np.zeros((2, 1, 2, L, N), dtype=np.uint64), np.zeros((2, o.beta, 2, D, N), dtype=np.uint64)
        idx = np.arange(N)
        for c, m in enumerate((np.ones(N, dtype=bool), (idx // 8) % 2 == 0)):
            for l in range(L):
                x_cts[c, :, :, l, m] = int(o.moduli[l]) - 1
            for l in range(D):
                x_evks[c, :, :, l, m] = int(o.moduli[l]) - 1
        case["x_cts"], case["x_evks"] = x_cts, x_evks
        case["x_sum"] = _oracle_sum(o, x_cts, x_evks, 0)[None]
        _KS[name] = case
    return _KS[name]


def run_key_switch(g, case):
    """the device's results for ks_case, keyed as the oracle's are"""
    N, L, B = g.N, g.L, case["B"]
    got = {}
    d_evk = g.to_device(case["evk"])
    for nl in (L, L - 1):
        d_ct, d_out = g.to_device(case["ct", nl]), g.empty((B, 2, nl, N))
        g.reencrypt(d_ct, d_evk, d_out, B, nl)
        got["one", nl] = d_out.to_host()
        g.reencrypt(d_ct, d_evk, d_ct, B, nl)
        got["in place", nl] = d_ct.to_host()
    d_out = g.empty((B, 2, L, N))
    g.reencrypt_sum(g.to_device(case["cts"]), g.to_device(case["evks"]), d_out, 3, B, L)
    got["sum"] = d_out.to_host()
    d_out = g.empty((1, 2, L, N))
    g.reencrypt_sum(g.to_device(case["x_cts"]), g.to_device(case["x_evks"]), d_out, 2, 1, L)
    got["x_sum"] = d_out.to_host()
    return got


def check_key_switch(name, got, case, tag):
    L = oracle(name).L
    for nl in (L, L - 1):
        assert np.array_equal(got["one", nl], case["one", nl]), (name, tag, "reencrypt", nl)
        assert np.array_equal(got["in place", nl], case["one", nl]), (name, tag, "reencrypt in place", nl)
    assert np.array_equal(got["sum"], case["sum"]), (name, tag, "reencrypt_sum")
    assert np.array_equal(got["x_sum"], case["x_sum"]), (name, tag, "reencrypt_sum, extreme residues")


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_conversions_and_key_switch(ctxs, name):
    g, o = ctxs(name)
    rng = np.random.default_rng(303)
    N, L, K, D = g.N, g.L, g.K, g.D
    B = _batch(g)
    for nl in (L, L - 1, 1):  # L - 1: a partial last digit wherever alpha does not divide it
        c1 = rand_polys(rng, g, list(range(nl)), B)
        c1[0, :, ::5] = (g.moduli[:nl] - np.uint64(1))[:, None]
        d_dig = g.empty((B, g.num_parts(nl), nl + K, N))
        g.modup(g.to_device(c1), d_dig, B, nl)
        dig = d_dig.to_host()
        for b in range(B):
            assert np.array_equal(dig[b], o.modup_digits(c1[b])), (name, "modup", nl, b)
        ids = list(range(nl)) + list(range(L, D))
        x = rand_polys(rng, g, ids, B)
        x[0, :, ::5] = (g.moduli[ids] - np.uint64(1))[:, None]
        d_md = g.empty((B, nl, N))
        g.moddown(g.to_device(x), d_md, B, nl)
        md = d_md.to_host()
        for b in range(B):
            assert np.array_equal(md[b], o.moddown(x[b])), (name, "moddown", nl, b)
    case = ks_case(name)
    check_key_switch(name, run_key_switch(g, case), case, "default")


@pytest.mark.gpu
@pytest.mark.parametrize("name,switch,absent", SWITCHED)
def test_key_switch_under_the_arithmetic_switches(ctxs, monkeypatch, name, switch, absent):
    """Switches are read once, when a context is created: the entry once more under the switch gives the default context's
    bits (and the oracle's) from the other arithmetic."""
    from ppqsflhe_amd import Context
    g, _ = ctxs(name)
    case = ks_case(name)
    want = run_key_switch(g, case)
    monkeypatch.setenv(switch, "1")
    args = TABLE[name][0]
    g2 = Context(args[0], args[1], args[2], device=0, **_kwargs(args))
    try:
        assert absent in list(g.arith) and absent not in list(g2.arith), (name, switch, list(g2.arith))
        got = run_key_switch(g2, case)
        for key in want:
            assert np.array_equal(got[key], want[key]), (name, switch, key)
        check_key_switch(name, got, case, switch)
    finally:
        g2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_newer_entry_points(ctxs, name):
    g, o = ctxs(name)
    rng = np.random.default_rng(404)
    L = g.L
    B = _batch(g)
    # fan-out into 3 key domains
    ct, evks = rand_ct(rng, g, L, B), rand_evks(rng, g, 3)
    got = fanout(g, ct, evks, L)
    for k in range(3):
        for b in range(B):
            assert np.array_equal(got[k, b], o.reencrypt(ct[b], evks[k])), (name, "fanout", k, b)
    # compact forms: Rescale(prefix) and Rescale(ReEncrypt(prefix)), down to one limb
    for nl_out in sorted({1, L - 1}):
        got = compress(g, ct, nl_out)
        for b in range(B):
            assert np.array_equal(got[b], o.rescale(prefix(ct[b], nl_out + 1))), (name, "compress", nl_out, b)
        got = fanout_compact(g, ct, evks[:2], nl_out)
        for k in range(2):
            for b in range(B):
                exp = o.rescale(o.reencrypt(prefix(ct[b], nl_out + 1), evks[k]))
                assert np.array_equal(got[k, b], exp), (name, "fanout_compact", nl_out, k, b)
    # re-randomisation with errors up to +-(2^62 - 1)
    ct2, pk, v, e0, e1 = wide_inputs(rng, g, L, 2)
    got = rerandomize(g, ct2, pk, v, e0, e1, L)
    for b in range(2):
        assert np.array_equal(got[b], exact_rerandomize(o, ct2[b], pk, v[b], e0[b], e1[b], L)), (name, "rerandomize", b)
    # partial decryption with such errors
    sk, e = rand_sk(rng, g), wide_errors(rng, g.N, 2)
    for lead in (0, 1):
        got = partial_decrypt(g, ct2, sk, e, L, lead)
        for b in range(2):
            assert np.array_equal(got[b], exact_share(o, ct2[b], sk, e[b], L, lead)), (name, "partial_decrypt", lead, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_keys_encryption_and_decoding(ctxs, name):
    g, o = ctxs(name)
    rng = np.random.default_rng(505)
    N, L, D = g.N, g.L, g.D
    s1, a1, e1 = make_keys(o, rng)
    s2, a2, e2 = make_keys(o, rng)
    pk1, sk1 = o.keygen(s1, a1, e1)
    pk2, _ = o.keygen(s2, a2, e2)
    d_pk, d_sk = g.empty((2, D, N)), g.empty((D, N))
    g.keygen(g.to_device(s1), g.to_device(a1), g.to_device(e1), d_pk, d_sk)
    assert np.array_equal(d_pk.to_host(), pk1), (name, "keygen pk")
    assert np.array_equal(d_sk.to_host(), sk1), (name, "keygen sk")
    u, r0, r1 = make_rk_rand(o, rng)
    d_evk = g.empty((g.beta, 2, D, N))
    g.rekeygen(g.to_device(s1), g.to_device(pk2), g.to_device(u), g.to_device(r0), g.to_device(r1), d_evk)
    assert np.array_equal(d_evk.to_host(), o.rekeygen(s1, pk2, u, r0, r1)), (name, "rekeygen")
    B = _batch(g)
    for nl in (L, L - 1):
        vals = rng.uniform(-0.3, 0.3, size=(B, N // 2))
        scale = o.sf_big(0) if nl == L else 2.0 ** 30
        pts = np.stack([o.encode(vals[b], scale, nl) for b in range(B)])
        v = np.stack([sample_ternary(rng, N) for _ in range(B)])
        f0 = np.stack([sample_gauss(rng, N) for _ in range(B)])
        f1 = np.stack([sample_gauss(rng, N) for _ in range(B)])
        d_ct = g.empty((B, 2, nl, N))
        g.encrypt(d_pk, g.to_device(pts), g.to_device(v), g.to_device(f0), g.to_device(f1), d_ct, B, nl)
        ct = d_ct.to_host()
        for b in range(B):
            assert np.array_equal(ct[b], o.encrypt(pk1, pts[b], v[b], f0[b], f1[b])), (name, "encrypt", nl, b)
        d_m, d_vals = g.empty((B, nl, N)), g.empty((B, N // 2), dtype=np.float64)
        g.decrypt(d_ct, d_sk, d_m, B, nl)
        m = d_m.to_host()
        for b in range(B):
            assert np.array_equal(m[b], o.decrypt_core(ct[b], sk1)), (name, "decrypt", nl, b)
        g.decode(d_m, d_vals, B, nl, scale)
        dec = d_vals.to_host()
        for b in range(B):
            err = np.abs(dec[b] - o.decrypt_decode(ct[b], sk1, scale)).max()
            assert err < 2.0 ** -40, (name, "decode", nl, b, err)
