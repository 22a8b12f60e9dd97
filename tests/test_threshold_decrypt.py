"""Threshold decryption (include/mkckks.h: mkckks_keygen_join, mkckks_partial_decrypt_batch, mkckks_fuse_shares_batch;
keyGen --join, partialDecrypt, fuseDecryptions): the common key domain is a joint key pk = (sum b_i, a) whose secret
sum s_i nobody holds; the aggregate is opened by n smudged partial decryptions that are summed.

    share_p[t][i] = INTT_i( ct[t][1][i] * sk_p[i] + (lead ? ct[t][0][i] : 0) ) + (e_p[t] mod q_i)     mod q_i
    m[t][i]       = sum_p share_p[t][i]                                                                 mod q_i

Every residue comparison is word for word.  The reference is `exact_share`: the oracle's decrypt_core of the prefix
(component 0 zeroed unless lead) plus e mod q_i in int64 floor arithmetic.

The two derived tolerances (noise rule of mkckks.h): n shares add sum e_p to the plaintext polynomial, slot k's real part
receives sum_j e_j cos(j theta_k), so the decoded values carry a Gaussian error of standard deviation
sd = sigma * sqrt(n N / 2) / scale.  (1) the measured standard deviation over the N / 2 slots lies within +-10 % of sd (the
estimate from N / 2 >= 2048 samples is good to ~2 %); (2) the largest error stays below the zero-smudging error plus 6 sd
(N / 2 <= 8192 Gaussian samples exceed 6 sd with probability < 2e-5)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_cli_hosts import BIN, _small_cc, _weights, run
from tests.test_compact_downlink import BOUND, PARAMS, _ok, _oracle, _same_bytes, prefix
from tests.test_gpu_parity import CONFIGS, make_keys, rand_ct, rand_polys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppqsflhe_amd", "host")
SYMBOLS = ("mkckks_keygen_join", "mkckks_partial_decrypt_batch", "mkckks_fuse_shares_batch")
EMAX = (1 << 62) - 1
N_PARTIES = 3


# ---- references -----------------------------------------------------------------------------------------------------

def exact_share(o, ct, sk, e, nl, lead):
    """One party's share of ct [2][nl_in][N] at its first nl limbs, in exact integer arithmetic."""
    pre = np.array(ct[:, :nl], dtype=np.uint64)
    if not lead:
        pre[0] = 0
    m = o.decrypt_core(pre, sk)
    for i in range(nl):
        q = int(o.moduli[i])
        lifted = np.mod(np.asarray(e, dtype=np.int64), np.int64(q)).astype(np.uint64)  # floor mod: in [0, q), exact
        m[i] = (m[i] + lifted) % np.uint64(q)                                           # < 2^61: no wrap
    return m


def sum_mod(o, polys):
    """sum of u64[..][nl][N] arrays limb by limb (limb ids 0 .. nl - 1); at most 8 terms below 2^61 each."""
    polys = list(polys)
    assert len(polys) <= 8
    acc = np.zeros_like(polys[0])
    for p in polys:
        acc = acc + p
    for i in range(acc.shape[-2]):
        acc[..., i, :] %= np.uint64(int(o.moduli[i]))
    return acc


def sub_mod(o, a, b):
    out = np.empty_like(a)
    for i in range(a.shape[-2]):
        q = np.uint64(int(o.moduli[i]))
        out[..., i, :] = (a[..., i, :] + (q - b[..., i, :])) % q
    return out


def join_key(o, pk_prev, s, e):
    """MultipartyKeyGen(prevPublicKey) from the oracle's keygen: (b_prev + e - a s, a) and NTT(s)."""
    pk, sk = o.keygen(s, pk_prev[1], e)  # (e - a s, a)
    out = pk.copy()
    for l in range(o.D):
        out[0, l] = (pk[0, l] + pk_prev[0, l]) % np.uint64(int(o.moduli[l]))
    return out, sk


def key_chain(o, rng, n=N_PARTIES):
    """n parties: [(s, pk, sk)]; the last pk is the joint key."""
    keys = []
    for p in range(n):
        s, a, e = make_keys(o, rng)
        pk, sk = o.keygen(s, a, e) if p == 0 else join_key(o, keys[-1][1], s, e)
        keys.append((s, pk, sk))
    return keys


def decode_poly(o, m, scale):
    """Decode of a decrypted polynomial m [nl][N] (COEFFICIENT): decrypt_decode of the ciphertext (NTT(m), 0)."""
    nl = m.shape[0]
    ct = np.zeros((2, nl, o.N), dtype=np.uint64)
    for i in range(nl):
        ct[0, i] = o.ntt_fwd(i, m[i])
    return o.decrypt_decode(ct, np.zeros((o.D, o.N), dtype=np.uint64), scale)


def noise_sd(sigma, n, N, scale):
    return sigma * np.sqrt(n * N / 2.0) / scale


_CHAINS = {}


def threshold_chain(name):
    """3 parties with a joint key, each encrypts its values under it; EvalAdd, Rescale, x 1/3 -> the aggregate at L - 1
    limbs.  Computed once per parameter set and left unchanged."""
    if name not in _CHAINS:
        from oracle.oracle import sample_gauss, sample_ternary
        o = _oracle(name)
        rng = np.random.default_rng(23)
        N, L = o.N, o.L
        vals = rng.uniform(-0.3, 0.3, size=(N_PARTIES, N // 2))
        keys = key_chain(o, rng)
        joint = keys[-1][1]
        acc = None
        for c in range(N_PARTIES):
            ct = o.encrypt(joint, o.encode(vals[c], o.sf_big(0), L), sample_ternary(rng, N), sample_gauss(rng, N),
                           sample_gauss(rng, N))
            acc = ct if acc is None else o.eval_add(acc, ct)
        agg = o.mult_factors(o.rescale(acc), o.const_factors(L - 1, 1, 1.0 / N_PARTIES))
        scale = o.sf_big(0) / float(o.moduli[L - 1]) * o.sf(1)
        sks = [k[2] for k in keys]
        zero = np.zeros(N, dtype=np.int64)
        m0 = sum_mod(o, [exact_share(o, agg, sks[p], zero, L - 1, p == 0) for p in range(N_PARTIES)])
        _CHAINS[name] = dict(o=o, keys=keys, sks=sks, sk_sum=sum_mod(o, [s[None] for s in sks])[0], agg=agg, scale=scale,
                             mean=vals.mean(axis=0), m0=m0, dec0=decode_poly(o, m0, scale))
    return _CHAINS[name]


# ---- CPU: surface and argument checks -------------------------------------------------------------------------------

def test_threshold_symbols_are_declared_bound_and_exported():
    from ppqsflhe_amd import Context, binding
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mkckks.h")).read(), flags=re.S)
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert sym in binding.SYMBOLS
        assert hasattr(binding.load_library(), sym)
    for meth in ("keygen_join", "partial_decrypt", "fuse_shares"):
        assert callable(getattr(Context, meth, None)), meth


def test_threshold_argument_checks_on_a_host_only_context():
    from ppqsflhe_amd import Context
    from ppqsflhe_amd.binding import MkckksError
    c = Context(12, 2, 40, 60, dnum=2, device=-1)
    kj, pd, fs = (getattr(c._L, s) for s in SYMBOLS)
    far = 1 << 40  # an output address far from the input's: pointers are never dereferenced
    W = 8 * c.N    # bytes of one limb polynomial
    try:
        L = c.L
        assert L >= 3
        # keygen_join(ctx, pk_prev, s, e, pk, sk)
        good = [8, 8, 8, far, 2 * far]
        for i in range(5):
            args = list(good)
            args[i] = None
            assert kj(c._h, *args) == -1, i
        assert kj(c._h, *good) == -2
        # partial_decrypt(ctx, ct, sk, e, share, n_ct, nl_in, nl, lead)
        good = [8, 8, 8, far]
        for lead in (0, 1):
            for i in range(4):
                args = list(good)
                args[i] = None
                assert pd(c._h, *args, 1, L, L, lead) == -1, i
            assert pd(c._h, *good, 1, L, 0, lead) == -1           # nl == 0
            assert pd(c._h, *good, 1, 2, 3, lead) == -1           # nl > nl_in
            assert pd(c._h, *good, 1, L + 1, 1, lead) == -1       # nl_in > L
            assert pd(c._h, *good, 1, L + 1, L + 1, lead) == -1
            assert pd(c._h, 8, 8, 8, 8, 1, L, L, lead) == -1                      # share over the ciphertext
            assert pd(c._h, 8, 8, 8, 8 + (2 * L - 1) * W, 1, L, 1, lead) == -1    # share starting inside its last limb
            assert pd(c._h, far + W, 8, 8, far, 2, L, 1, lead) == -1              # ciphertext starting inside the share
            assert pd(c._h, 8, 8, 8, 8 + 2 * L * W, 1, L, L, lead) == -2          # share right behind the ciphertext
            assert pd(c._h, *good, 1, L, L, lead) == -2
            assert pd(c._h, *good, 1, L, 1, lead) == -2
            assert pd(c._h, *good, 0, L, L, lead) == 0
        # fuse_shares(ctx, shares, m, n_parties, n_ct, nl)
        assert fs(c._h, None, far, 3, 1, L) == -1
        assert fs(c._h, 8, None, 3, 1, L) == -1
        assert fs(c._h, 8, far, 0, 1, L) == -1                    # n_parties == 0
        assert fs(c._h, 8, far, 3, 1, 0) == -1
        assert fs(c._h, 8, far, 3, 1, L + 1) == -1
        assert fs(c._h, 8, 8 + L * W, 3, 1, L) == -1              # output = shares[1]
        assert fs(c._h, 8, 8 + W, 3, 1, L) == -1                  # output starting inside shares[0]
        assert fs(c._h, far + W, far, 3, 1, L) == -1              # shares starting inside the output
        assert fs(c._h, 8, far, 3, 1, L) == -2
        assert fs(c._h, 8, 8, 3, 1, L) == -2                      # output = shares[0]
        assert fs(c._h, 8, 8 + 3 * L * W, 3, 1, L) == -2          # output right behind the shares
        assert fs(c._h, 8, far, 1, 1, 1) == -2
        assert fs(c._h, 8, far, 3, 0, L) == 0
        for call in (lambda: c.keygen_join(8, 8, 8, far, 2 * far), lambda: c.partial_decrypt(8, 8, 8, far, 1, L, 1, True),
                     lambda: c.fuse_shares(8, far, 3, 1, L)):
            with pytest.raises(MkckksError) as ei:
                call()
            assert ei.value.code == -2
        with pytest.raises(MkckksError) as ei:
            c.fuse_shares(8, far, 0, 1, L)
        assert ei.value.code == -1
    finally:
        c.close()


# ---- CPU: the protocol on the oracle alone --------------------------------------------------------------------------

def smudging(rng, N, sigma, n=N_PARTIES):
    return [np.rint(rng.normal(0.0, sigma, size=N)).astype(np.int64) for _ in range(n)]


@pytest.mark.parametrize("name", ["p12", "p14"])
def test_oracle_threshold_protocol(name):
    ch = threshold_chain(name)
    o, agg, scale, sks, mean = ch["o"], ch["agg"], ch["scale"], ch["sks"], ch["mean"]
    N, nl = o.N, agg.shape[1]
    # zero smudging: the fused polynomial is the decryption under the summed key, and decodes to the mean
    assert np.array_equal(ch["m0"], o.decrypt_core(agg, ch["sk_sum"]))
    err0 = np.abs(ch["dec0"] - mean).max()
    print(f"{name}: zero-smudging error 2^{np.log2(err0):.2f}")
    assert err0 < BOUND[name], (name, err0)
    assert np.array_equal(ch["dec0"], o.decrypt_decode(agg, ch["sk_sum"], scale))
    for sigma_bits in (10, 20):
        sigma = 2.0 ** sigma_bits
        rng = np.random.default_rng(500 + sigma_bits)
        es = smudging(rng, N, sigma)
        shares = [exact_share(o, agg, sks[p], es[p], nl, p == 0) for p in range(N_PARTIES)]
        fused = sum_mod(o, shares)
        e_sum = es[0] + es[1] + es[2]
        exp = ch["m0"].copy()
        for i in range(nl):
            q = int(o.moduli[i])
            exp[i] = (exp[i] + np.mod(e_sum, np.int64(q)).astype(np.uint64)) % np.uint64(q)
        assert np.array_equal(fused, exp), (name, sigma_bits)
        dec = decode_poly(o, fused, scale)
        sd = noise_sd(sigma, N_PARTIES, N, scale)
        # decode is linear: the decoded error against the zero-smudging decode is the decode of fused - m0 (= sum e mod q,
        # centred by the CRT interpolation).  Taken on the polynomials, because at scale 2^100 the difference of two doubles
        # near 0.3 cannot resolve an error of 2^-84
        noise = decode_poly(o, sub_mod(o, fused, ch["m0"]), scale)
        ratio = noise.std() / sd
        err = np.abs((ch["dec0"] - mean) + noise).max()  # the decoded error, the small terms added first
        print(f"{name} sigma 2^{sigma_bits}: sd 2^{np.log2(sd):.2f}, measured / rule {ratio:.4f}, largest / sd "
              f"{np.abs(noise).max() / sd:.2f}, error 2^{np.log2(err):.2f}")
        assert 0.9 < ratio < 1.1, (name, sigma_bits, ratio)
        assert err < err0 + 6 * sd, (name, sigma_bits, err, err0, sd)
        assert np.abs(dec - mean).max() < BOUND[name] + 6 * sd, (name, sigma_bits)  # and the direct decode is the mean
        # any 2 of the 3 shares are garbage (with and without the lead share)
        for pair in ((0, 1), (0, 2), (1, 2)):
            two = np.abs(decode_poly(o, sum_mod(o, [shares[p] for p in pair]), scale) - mean).max()
            assert two > 1, (name, sigma_bits, pair, two)
    for p in range(N_PARTIES):  # no single party's key opens the aggregate
        one = np.abs(o.decrypt_decode(agg, sks[p], scale) - mean).max()
        assert one > 1, (name, p, one)


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctxs():
    from oracle.oracle import OracleContext
    from ppqsflhe_amd import Context
    cache = {}

    def get(name):
        if name not in cache:
            a = CONFIGS[name] if name in CONFIGS else PARAMS[name]
            cache[name] = (Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0),
                           OracleContext(a[0], a[1], a[2], a[3], dnum=a[4]))
        return cache[name]

    yield get
    for g, _ in cache.values():
        g.close()


def rand_sk(rng, g):
    return rand_polys(rng, g, list(range(g.D)), 1)[0]


def wide_errors(rng, N, B):
    """uniform in +-2^59, with +-(2^62 - 1), 0 and +-1 planted at both ends and in the middle."""
    e = rng.integers(-2 ** 59, 2 ** 59, size=(B, N), dtype=np.int64)
    plant = np.array([EMAX, -EMAX, 0, 1, -1], dtype=np.int64)
    e[:, :5], e[:, -5:] = plant, plant[::-1]
    e[:, N // 2 - 2:N // 2 + 3] = plant
    return e


def partial_decrypt(g, ct, sk, e, nl, lead):
    B, nl_in = ct.shape[0], ct.shape[2]
    d_share = g.empty((B, nl, g.N))
    g.partial_decrypt(g.to_device(ct), g.to_device(sk), g.to_device(e, np.int64), d_share, B, nl_in, nl, lead)
    return d_share.to_host().reshape(B, nl, g.N)


def composition(g, ct, sk, e, nl, lead):
    """mkckks_rerandomize_batch(v = 0, e0 = e, e1 = 0) + mkckks_decrypt_batch on the packed prefix (component 0 zeroed
    unless lead): the device reference of the header."""
    B = ct.shape[0]
    pre = np.ascontiguousarray(ct[:, :, :nl])
    if not lead:
        pre[:, 0] = 0
    d_ct = g.to_device(pre)
    zero8, zero64 = np.zeros((B, g.N), dtype=np.int8), np.zeros((B, g.N), dtype=np.int64)
    g.rerandomize(d_ct, g.to_device(np.zeros((2, g.D, g.N), dtype=np.uint64)), g.to_device(zero8, np.int8),
                  g.to_device(e, np.int64), g.to_device(zero64, np.int64), d_ct, B, nl, nl)
    d_m = g.empty((B, nl, g.N))
    g.decrypt(d_ct, g.to_device(sk), d_m, B, nl)
    return d_m.to_host().reshape(B, nl, g.N)


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("name,nl_in,nl", [
    ("c1", 3, 3), ("ref", 4, 4), ("ref", 4, 3), ("c3", 12, 12), ("c3", 11, 2), ("c3", 2, 1), ("c5s", 20, 20),
    ("tiny", 5, 5), ("n17", 4, 4), ("n11", 4, 4)])
def test_partial_decrypt_matches_the_oracle(ctxs, name, nl_in, nl, lead):
    g, o = ctxs(name)
    rng = np.random.default_rng(700 + 17 * nl_in + nl + lead)
    B = 3
    ct, sk, e = rand_ct(rng, g, nl_in, B), rand_sk(rng, g), wide_errors(rng, g.N, B)
    got = partial_decrypt(g, ct, sk, e, nl, lead)
    for b in range(B):
        assert np.array_equal(got[b], exact_share(o, ct[b], sk, e[b], nl, lead)), (name, nl_in, nl, lead, b)
    if name == "c3":
        assert np.array_equal(got, composition(g, ct, sk, e, nl, lead)), (name, nl_in, nl, lead)


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl", [("c3", 12), ("ref", 4)])
def test_partial_decrypt_extreme_residues(ctxs, name, nl):
    """Every word of ct and sk at q_i - 1, every error at +-(2^62 - 1)."""
    g, o = ctxs(name)
    B = 2
    ct = np.empty((B, 2, nl, g.N), dtype=np.uint64)
    sk = np.empty((g.D, g.N), dtype=np.uint64)
    for l in range(nl):
        ct[:, :, l] = int(g.moduli[l]) - 1
    for l in range(g.D):
        sk[l] = int(g.moduli[l]) - 1
    e = np.stack([np.full(g.N, EMAX, dtype=np.int64), np.full(g.N, -EMAX, dtype=np.int64)])
    for lead in (0, 1):
        got = partial_decrypt(g, ct, sk, e, nl, lead)
        for b in range(B):
            assert np.array_equal(got[b], exact_share(o, ct[b], sk, e[b], nl, lead)), (name, lead, b)


def device_shares(g, ct, sks, es, nl):
    """shares u64[n_parties][B][nl][N] on the device, party 0 leading."""
    n, B, nl_in = len(sks), ct.shape[0], ct.shape[2]
    d_shares, d_ct = g.empty((n, B, nl, g.N)), g.to_device(ct)
    for p in range(n):
        g.partial_decrypt(d_ct, g.to_device(sks[p]), g.to_device(es[p], np.int64), d_shares.view(p * B * nl * g.N, (B, nl, g.N)),
                          B, nl_in, nl, p == 0)
    return d_shares


@pytest.mark.gpu
@pytest.mark.parametrize("n_parties", [3, 9])
@pytest.mark.parametrize("name,nl", [("c3", 2), ("ref", 4)])
def test_fuse_shares(ctxs, name, nl, n_parties):
    g, o = ctxs(name)
    rng = np.random.default_rng(60 + nl + n_parties)
    B, N = 2, g.N
    ct = rand_ct(rng, g, nl, B)
    sks = [rand_sk(rng, g) for _ in range(n_parties)]
    sk_sum = sks[0].copy()
    for s in sks[1:]:  # pairwise: 9 terms of 60 bits would wrap
        sk_sum = sk_sum + s
        for l in range(g.D):
            sk_sum[l] %= np.uint64(int(g.moduli[l]))
    d_m = g.empty((B, nl, N))
    g.decrypt(g.to_device(ct), g.to_device(sk_sum), d_m, B, nl)
    plain = d_m.to_host().reshape(B, nl, N)
    zeros = [np.zeros((B, N), dtype=np.int64)] * n_parties
    errs = [rng.integers(-2 ** 58, 2 ** 58, size=(B, N), dtype=np.int64) for _ in range(n_parties)]  # the sum fits int64
    for es in (zeros, errs):
        exp = plain.copy()
        e_sum = np.sum(es, axis=0, dtype=np.int64)
        for i in range(nl):
            q = int(g.moduli[i])
            exp[:, i] = (exp[:, i] + np.mod(e_sum, np.int64(q)).astype(np.uint64)) % np.uint64(q)
        d_shares = device_shares(g, ct, sks, es, nl)
        shares = d_shares.to_host()
        g.fuse_shares(d_shares, d_m, n_parties, B, nl)
        assert np.array_equal(d_m.to_host().reshape(B, nl, N), exp), (name, n_parties)
        assert np.array_equal(d_shares.to_host(), shares)  # inputs unchanged
        g.fuse_shares(d_shares, d_shares.view(0, (B, nl, N)), n_parties, B, nl)  # into shares[0]
        after = d_shares.to_host().reshape(n_parties, B, nl, N)
        assert np.array_equal(after[0], exp), (name, n_parties)
        assert np.array_equal(after[1:], shares.reshape(n_parties, B, nl, N)[1:])


def device_keygen_join(g, pk_prev, s, e):
    d_pk, d_sk = g.empty((2, g.D, g.N)), g.empty((g.D, g.N))
    g.keygen_join(g.to_device(pk_prev), g.to_device(s), g.to_device(e), d_pk, d_sk)
    return d_pk.to_host().reshape(2, g.D, g.N), d_sk.to_host().reshape(g.D, g.N)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c1", "c3", "n11"])
def test_keygen_join(ctxs, name):
    from oracle.oracle import sample_gauss, sample_ternary
    g, o = ctxs(name)
    rng = np.random.default_rng(90)
    N, L = g.N, g.L
    s, a, e = make_keys(o, rng)
    keys = [(s,) + tuple(o.keygen(s, a, e))]
    for _ in range(2):
        s, _, e = make_keys(o, rng)
        pk, sk = device_keygen_join(g, keys[-1][1], s, e)
        exp_pk, exp_sk = join_key(o, keys[-1][1], s, e)
        assert np.array_equal(pk, exp_pk) and np.array_equal(sk, exp_sk), name
        keys.append((s, pk, sk))
    # in place on the public key
    d_pk, d_sk = g.to_device(keys[1][1]), g.empty((g.D, N))
    g.keygen_join(d_pk, g.to_device(keys[2][0]), g.to_device(e), d_pk, d_sk)
    assert np.array_equal(d_pk.to_host().reshape(2, g.D, N), keys[2][1])
    # the sum of the three sk decrypts an encryption under the joint key
    vals = rng.uniform(-0.3, 0.3, size=N // 2)
    ct = o.encrypt(keys[-1][1], o.encode(vals, o.sf_big(0), L), sample_ternary(rng, N), sample_gauss(rng, N), sample_gauss(rng, N))
    sk_sum = sum_mod(o, [k[2][None] for k in keys])[0]
    err = np.abs(o.decrypt_decode(ct, sk_sum, o.sf_big(0)) - vals).max()
    assert err < 2.0 ** -20, (name, err)
    assert np.abs(o.decrypt_decode(ct, keys[-1][2], o.sf_big(0)) - vals).max() > 1


@pytest.mark.gpu
def test_partial_decrypt_call_properties(ctxs):
    """The strided prefix = the packed prefix; inputs are not written; a poisoned tail after the output stays intact; empty
    calls write nothing; a batch larger than one workspace chunk (MKCKKS_CHUNK = 16); wrong overlaps are refused."""
    from ppqsflhe_amd.binding import MkckksError
    g, o = ctxs("c3")
    rng = np.random.default_rng(78)
    nl_in, B, N = 11, 2, g.N
    ct, sk, e = rand_ct(rng, g, nl_in, B), rand_sk(rng, g), wide_errors(rng, g.N, B)
    full = partial_decrypt(g, ct, sk, e, nl_in, 1)
    d_ct, d_sk, d_e = g.to_device(ct), g.to_device(sk), g.to_device(e, np.int64)
    POISON = 0xA5A5A5A5A5A5A5A5
    for nl in (2, 5):
        words, pad = B * nl * N, 2 * N
        d_big = g.to_device(np.full(words + pad, POISON, dtype=np.uint64))
        d_out = d_big.view(0, (B, nl, N))
        g.partial_decrypt(d_ct, d_sk, d_e, d_out, B, nl_in, nl, 1)
        strided = d_out.to_host().reshape(B, nl, N)
        assert np.all(d_big.to_host()[words:] == POISON)
        assert np.array_equal(strided, partial_decrypt(g, prefix(ct, nl), sk, e, nl, 1)), nl
        assert np.array_equal(strided, full[:, :nl]), nl  # limb by limb the same arithmetic
        d_out.upload(np.full(strided.shape, POISON, dtype=np.uint64))
        g.partial_decrypt(d_ct, d_sk, d_e, d_out, 0, nl_in, nl, 1)
        assert np.all(d_out.to_host() == POISON)
    assert np.array_equal(d_ct.to_host().reshape(ct.shape), ct) and np.array_equal(d_sk.to_host().reshape(sk.shape), sk)
    assert np.array_equal(d_e.to_host().reshape(e.shape), e)
    d_shares = g.to_device(np.full((3, B, 2, N), 7, dtype=np.uint64))
    for call in (lambda: g.partial_decrypt(d_ct, d_sk, d_e, d_ct, B, nl_in, 2, 1),
                 lambda: g.partial_decrypt(d_ct, d_sk, d_e, d_ct.view(N, (N,)), B, nl_in, nl_in, 0),
                 lambda: g.fuse_shares(d_shares, d_shares.view(B * 2 * N, (B, 2, N)), 3, B, 2),
                 lambda: g.fuse_shares(d_shares, d_shares.view(N, (N,)), 3, B, 2)):
        with pytest.raises(MkckksError) as ei:
            call()
        assert ei.value.code == -1
    assert np.array_equal(d_ct.to_host().reshape(ct.shape), ct) and np.all(d_shares.to_host() == 7)
    g.fuse_shares(d_shares, d_shares, 3, 0, 2)
    assert np.all(d_shares.to_host() == 7)
    # more ciphertexts than one chunk, on the small ring
    g2, o2 = ctxs("ref")
    B2, nl2 = 19, 3
    ct, sk, e = rand_ct(rng, g2, nl2, B2), rand_sk(rng, g2), wide_errors(rng, g2.N, B2)
    for lead in (0, 1):
        got = partial_decrypt(g2, ct, sk, e, nl2, lead)
        for b in range(B2):
            assert np.array_equal(got[b], exact_share(o2, ct[b], sk, e[b], nl2, lead)), (lead, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl", [("c3", 12), ("ref", 4)])
@pytest.mark.parametrize("env", [{"MKCKKS_GENERIC_NTT": "1"}, {"MKCKKS_NO_FP64": "1"}, {"MKCKKS_NO_PM": "1"}, {"MKCKKS_CHUNK": "1"}])
def test_partial_decrypt_under_the_library_switches(ctxs, monkeypatch, env, name, nl):
    """Switches are read once, when a context is created: a fresh context under each must give the same bits."""
    from ppqsflhe_amd import Context
    _, o = ctxs(name)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    a = CONFIGS[name]
    g = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)
    try:
        rng = np.random.default_rng(43 + nl)
        B = 2
        ct, sk, e = rand_ct(rng, g, nl, B), rand_sk(rng, g), wide_errors(rng, g.N, B)
        for lead in (0, 1):
            got = partial_decrypt(g, ct, sk, e, nl, lead)
            for b in range(B):
                assert np.array_equal(got[b], exact_share(o, ct[b], sk, e[b], nl, lead)), (name, env, lead, b)
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["p14", "p12"])
def test_threshold_decryption_on_the_device(ctxs, name):
    """The chain of the CPU test with device-sampled errors (sigma 2^20, two stream bases): partial_decrypt x 3 ->
    fuse_shares -> decode.  The mean within the CPU test's bound (zero-smudging error + 6 sd); shares from the two bases
    differ in every limb, yet fuse and decode alike within twice that bound."""
    g, o = ctxs(name)
    ch = threshold_chain(name)
    agg, scale, sks, mean = ch["agg"], ch["scale"], ch["sks"], ch["mean"]
    nl, N, sigma = agg.shape[1], g.N, 2.0 ** 20
    d_agg = g.to_device(agg[None])
    # the zero-smudging error of the bound is the device's own decode of the zero-error shares: the oracle's decode of the
    # same polynomial rounds differently in its last bits, more than 6 sd at p12
    d_m, d_vals = g.empty((1, nl, N)), g.empty((1, N // 2), dtype=np.float64)
    g.fuse_shares(device_shares(g, agg[None], sks, [np.zeros((1, N), dtype=np.int64)] * N_PARTIES, nl), d_m, N_PARTIES, 1, nl)
    assert np.array_equal(d_m.to_host().reshape(nl, N), ch["m0"])
    g.decode(d_m, d_vals, 1, nl, scale)
    err0 = np.abs(d_vals.to_host().reshape(N // 2) - mean).max()
    assert err0 < BOUND[name], (name, err0)
    bound = err0 + 6 * noise_sd(sigma, N_PARTIES, N, scale)
    key = np.random.default_rng(4).bytes(32)
    outs = []
    for base in (0, 3000):
        d_shares = g.empty((N_PARTIES, 1, nl, N))
        es = []
        for p in range(N_PARTIES):
            d_e = g.empty((1, N), np.int64)
            g.sample_gauss_wide(d_e, N, sigma, key, base + p)
            g.partial_decrypt(d_agg, g.to_device(sks[p]), d_e, d_shares.view(p * nl * N, (1, nl, N)), 1, nl, nl, p == 0)
            es.append(d_e.to_host().reshape(N))
        shares = d_shares.to_host().reshape(N_PARTIES, nl, N)
        for p in range(N_PARTIES):
            assert np.array_equal(shares[p], exact_share(o, agg, sks[p], es[p], nl, p == 0)), (name, base, p)
        d_m, d_vals = g.empty((1, nl, N)), g.empty((1, N // 2), dtype=np.float64)
        g.fuse_shares(d_shares, d_m, N_PARTIES, 1, nl)
        assert np.array_equal(d_m.to_host().reshape(nl, N), sum_mod(o, list(shares)))
        g.decode(d_m, d_vals, 1, nl, scale)
        vals = d_vals.to_host().reshape(N // 2)
        err = np.abs(vals - mean).max()
        print(f"{name} base {base}: error 2^{np.log2(err):.2f}, bound 2^{np.log2(bound):.2f}")
        assert err < bound, (name, base, err, bound)
        outs.append((shares, vals))
    for p in range(N_PARTIES):
        for l in range(nl):
            assert not np.array_equal(outs[0][0][p, l], outs[1][0][p, l]), (p, l)
    assert np.abs(outs[0][1] - outs[1][1]).max() < 2 * bound


# ---- CPU: the hosts' argument and file checks (no device is reached) ------------------------------------------------

HDR = "<4sIIIIIIIdII"  # hostlib.hpp BlobHeader: magic, version, kind, ring, limbs, parts, level, noise_deg, scale, slots, reserved
KIND_CT, KIND_SK, KIND_SHARE = 1, 3, 6


def share_blob(N, L, nl, lead, kind=KIND_SHARE, parts=1, fill=1):
    import struct
    hdr = struct.pack(HDR, b"MKCK", 1, kind, N, nl, parts, L - nl, 2, 2.0 ** 40, N // 2, int(lead))
    return hdr + np.full(parts * nl * N, fill, dtype=np.uint64).tobytes()


def share_file(path, blob):
    """a JSON envelope with one layer: mean, std_dev and one values ciphertext position, all holding `blob`."""
    import base64
    b64 = base64.b64encode(blob).decode()
    path.write_text(json.dumps({"weights_summary": [{"layer": "l", "shape": [3], "mean": b64, "std_dev": b64, "values": [b64]}]}))
    return path


def test_threshold_command_line_errors(tmp_path):
    """Every misuse: exit 1 with its message, nothing written."""
    from tests.test_cli_hosts import write_key_container
    cc = _small_cc(tmp_path)
    moduli = json.load(open(cc))["mkckks_cc"]["moduli"]
    N, L = 1 << 14, len(moduli)
    out = tmp_path / "out.json"
    msg = "[pdecrypt] ERROR: --smudge-bits needs an integer in [6, 56]"
    for bits in ("5", "57", "x"):
        for extra in ([], ["--lead"]):
            r = run("partialDecrypt", cc, "sk", "in", out, *extra, "--smudge-bits", bits)
            assert r.returncode == 1 and msg in r.stderr, (bits, r.stdout + r.stderr)
            assert not os.path.exists(out), bits
    for tail in (["--smudge-bits"], ["--lead", "--lead"], ["--smudge-bits", "20", "--smudge-bits", "20"], ["--led"]):
        r = run("partialDecrypt", cc, "sk", "in", out, *tail)
        assert r.returncode == 1 and "Usage:" in r.stderr and not os.path.exists(out), tail
    # keyGen --join: a missing file, and files that are no public key
    pk, sk = tmp_path / "pk", tmp_path / "sk"
    not_keys = {"missing": tmp_path / "nokey", "cc": cc, "text": tmp_path / "text", "secret": tmp_path / "seckey",
                "ring": tmp_path / "ringkey", "short": tmp_path / "shortkey"}
    not_keys["text"].write_text("not a key\n")
    write_key_container(not_keys["secret"], KIND_SK, N, 1, 1, np.zeros(N, dtype=np.uint64))
    write_key_container(not_keys["ring"], 2, N // 2, 1, 2, np.zeros(N, dtype=np.uint64))
    not_keys["short"].write_bytes(b"MKCK\x01\x00\x00\x00")
    for name, path in not_keys.items():
        r = run("keyGen", cc, pk, sk, "--join", path)
        assert r.returncode == 1 and f"[keyGen] ERROR: Failed to load public key from {path}" in r.stderr, (name, r.stdout + r.stderr)
        assert not os.path.exists(pk) and not os.path.exists(sk), name
    for args in ((cc, pk, sk, "--join"), (cc, pk, sk, "--joint", "x"), (cc, pk, sk, "x", "--join")):
        r = run("keyGen", *args)
        assert r.returncode == 1 and "Usage:" in r.stderr and not os.path.exists(pk), args
    # fuseDecryptions
    files = {
        "lead": share_file(tmp_path / "lead.json", share_blob(N, L, L - 1, True)),
        "lead2": share_file(tmp_path / "lead2.json", share_blob(N, L, L - 1, True)),
        "main": share_file(tmp_path / "main.json", share_blob(N, L, L - 1, False)),
        "main2": share_file(tmp_path / "main2.json", share_blob(N, L, L - 1, False)),
        "low": share_file(tmp_path / "low.json", share_blob(N, L, L - 2, False)),
        "ct": share_file(tmp_path / "ct.json", share_blob(N, L, L - 1, 0, kind=KIND_CT, parts=2)),
        "big": share_file(tmp_path / "big.json", share_blob(N, L, L - 1, False, fill=max(moduli))),
        "cut": share_file(tmp_path / "cut.json", share_blob(N, L, L - 1, False)[:-8]),
    }
    cases = [
        (("main", "main2"), "[fuse] ERROR: need exactly one lead share per ciphertext (position 0 has 0)"),
        (("main",), "[fuse] ERROR: need exactly one lead share per ciphertext (position 0 has 0)"),
        (("lead", "main", "lead2"), "[fuse] ERROR: need exactly one lead share per ciphertext (position 0 has 2)"),
        (("lead", "low"), "shares differ in layers, shapes, levels or scales"),
        (("lead", "ct"), "not a mkckks share blob"),
        (("ct", "main"), "not a mkckks share blob"),
        (("lead", "big"), "share: residue not below its modulus"),
        (("lead", "cut"), "share blob has the wrong size"),
    ]
    for names, msg in cases:
        r = run("fuseDecryptions", cc, *(files[n] for n in names), out)
        assert r.returncode == 1 and "[fuse] ERROR: " in r.stderr and msg in r.stderr, (names, r.stdout + r.stderr)
        assert not os.path.exists(out), names
    r = run("fuseDecryptions", cc, files["lead"], tmp_path / "nofile.json", out)
    assert r.returncode == 1 and "[fuse] ERROR: Could not open share file" in r.stderr and not os.path.exists(out)
    r = run("fuseDecryptions", cc, out)
    assert r.returncode == 1 and "Usage:" in r.stderr
    r = run("fuseDecryptions", cc, files["lead"], files["main"], out, env={"MKCKKS_DECRYPT_NOISE": "loud"})
    assert r.returncode == 1 and "MKCKKS_DECRYPT_NOISE must be" in r.stderr and not os.path.exists(out)


def test_share_selftest_plain_and_under_asan_ubsan():
    """The share-blob parser on truncated, oversized, wrong-kind, wrong-ring and non-canonical blobs: a stand-alone program,
    plain and under AddressSanitizer + UBSan.  A sanitizer report aborts the process (non-zero exit)."""
    r = subprocess.run(["make", "-C", HOST, "-s", "build/share_selftest", "share-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    for exe in (os.path.join(BIN, "share_selftest"), os.path.join(BIN, "asan", "share_selftest")):
        r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, (exe, r.stdout[-2000:] + r.stderr[-2000:])
        assert "ok share selftest" in r.stdout and "FAIL" not in r.stderr, exe
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, exe
        for case in ("truncated payload", "oversized by one byte", "ciphertext blob", "wrong ring", "non-canonical word"):
            assert f"ok {case}" in r.stdout, (exe, case)


# ---- GPU: through the binaries --------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_threshold_round_through_the_binaries(tmp_path):
    """N = 2^14, MKWS.  Key chain keyGen / keyGen --join x 2; two clients encrypt under the joint key, a third under a
    stand-alone key of its own with a re-encryption key to the joint key; serverRound; partialDecrypt x 3; fuseDecryptions."""
    import struct
    from tests.test_cli_hosts import read_key_container
    from tests.test_seeded_ciphertexts import read_mkws
    tmp, ext, N = tmp_path, "mkws", 1 << 14
    cc = _small_cc(tmp)
    rng = np.random.default_rng(808)
    vals = [[("dense", rng.uniform(-0.3, 0.3, 2 * 8192 + 300)), ("bias", rng.uniform(-0.3, 0.3, 4))] for _ in range(3)]
    mean = [np.mean([np.asarray(vals[c][li][1]) for c in range(3)], axis=0) for li in range(2)]
    r0 = _ok(run("keyGen", cc, tmp / "pk0", tmp / "sk0"))
    for p in (1, 2):
        r = _ok(run("keyGen", cc, tmp / f"pk{p}", tmp / f"sk{p}", "--join", tmp / f"pk{p - 1}"))
        assert f"[keyGen] Public and Private keys generated, joined to {tmp / f'pk{p - 1}'}" in r.stdout
    rx = _ok(run("keyGen", cc, tmp / "pkx", tmp / "skx"))  # the third client's own, stand-alone key
    # without --join: today's messages and formats; a joined key has the same containers
    for r in (r0, rx):
        assert "[keyGen] Public and Private keys generated\n" in r.stdout and "joined" not in r.stdout
    kinds = [read_key_container(tmp / f"pk{p}")[:4] for p in ("0", "1", "2", "x")]
    assert all(k == kinds[0] and k[0] == 2 and k[3] == 2 for k in kinds), kinds
    assert len({os.path.getsize(tmp / f"sk{p}") for p in ("0", "1", "2", "x")}) == 1
    a = [read_key_container(tmp / f"pk{p}")[4][1] for p in range(3)]
    assert np.array_equal(a[0], a[1]) and np.array_equal(a[0], a[2])  # one `a` along the chain
    joint = tmp / "pk2"
    for c, key in ((0, joint), (1, joint), (2, tmp / "pkx")):
        _ok(run("encryptModelWeights", cc, key, _weights(tmp, f"w{c}.json", vals[c]), tmp / f"enc{c}.{ext}"))
    _ok(run("REkeyGen", cc, tmp / "skx", joint, tmp / "rkx"))
    agg = tmp / f"agg.{ext}"
    _ok(run("serverRound", cc, agg, "-", tmp / f"enc0.{ext}", "-", tmp / f"enc1.{ext}", tmp / "rkx", tmp / f"enc2.{ext}"))
    # a plain decryptModelWeights round under the stand-alone key: as before
    _ok(run("decryptModelWeights", cc, tmp / "skx", tmp / f"enc2.{ext}", tmp / "own.json"))
    own = json.load(open(tmp / "own.json"))["weights_summary"]
    for li in range(2):
        assert np.abs(np.array(own[li]["values"]) - np.asarray(vals[2][li][1])).max() < BOUND["p14"], li
    sigma_bits = {0: 20, 1: 10, 2: 20}
    for p, extra in ((0, ["--lead"]), (1, ["--smudge-bits", "10"]), (2, [])):
        r = _ok(run("partialDecrypt", cc, tmp / f"sk{p}", agg, tmp / f"sh{p}.{ext}", *extra))
        assert f"{'lead ' if p == 0 else ''}share(s), smudged at sigma 2^{sigma_bits[p]}\n" in r.stdout, r.stdout
    n_blobs = len(read_mkws(agg)[1])
    heads = []
    for p in range(3):
        blobs = read_mkws(tmp / f"sh{p}.{ext}")[1]
        assert len(blobs) == n_blobs
        heads.append([struct.unpack(HDR, b[:48]) for b in blobs])
        for h, b in zip(heads[-1], blobs):
            assert h[2] == KIND_SHARE and h[3] == N and h[5] == 1 and h[10] == (1 if p == 0 else 0) and len(b) == 48 + 8 * h[4] * N
    assert [h[4:10] for h in heads[0]] == [h[4:10] for h in heads[1]] == [h[4:10] for h in heads[2]]
    scale = heads[0][0][8]
    sd = np.sqrt(sum(4.0 ** b for b in sigma_bits.values()) * N / 2.0) / scale  # the noise rule with each share's own sigma
    _ok(run("fuseDecryptions", cc, *(tmp / f"sh{p}.{ext}" for p in range(3)), tmp / "fused.json"))
    fused = json.load(open(tmp / "fused.json"))["weights_summary"]
    for li in range(2):
        assert fused[li]["layer"] == vals[0][li][0] and fused[li]["shape"] == [len(mean[li])]
        err = np.abs(np.array(fused[li]["values"]) - mean[li]).max()
        print(f"layer {li}: error 2^{np.log2(err):.2f}, 6 sd = 2^{np.log2(6 * sd):.2f}")
        assert err < BOUND["p14"] + 6 * sd, (li, err)
    # the order of the share files does not matter
    _ok(run("fuseDecryptions", cc, *(tmp / f"sh{p}.{ext}" for p in (2, 0, 1)), tmp / "fused_b.json"))
    assert _same_bytes(tmp / "fused.json", tmp / "fused_b.json")
    # two of the three shares, and one party's key alone: garbage, not the mean
    _ok(run("fuseDecryptions", cc, tmp / f"sh0.{ext}", tmp / f"sh1.{ext}", tmp / "two.json"))
    two = json.load(open(tmp / "two.json"))["weights_summary"]
    assert np.abs(np.array(two[0]["values"]) - mean[0]).max() > 1
    _ok(run("decryptModelWeights", cc, tmp / "sk0", agg, tmp / "one.json"))
    one = json.load(open(tmp / "one.json"))["weights_summary"]
    assert np.abs(np.array(one[0]["values"]) - mean[0]).max() > 1
    # a second share of the same file is drawn afresh
    _ok(run("partialDecrypt", cc, tmp / "sk2", agg, tmp / f"sh2b.{ext}"))
    assert not _same_bytes(tmp / f"sh2.{ext}", tmp / f"sh2b.{ext}")
    # a share file is no ciphertext file, and the other way round
    r = run("partialDecrypt", cc, tmp / "sk0", tmp / f"sh1.{ext}", tmp / "bad.mkws")
    assert r.returncode == 1 and "[pdecrypt] ERROR: not a mkckks ciphertext blob" in r.stderr and not os.path.exists(tmp / "bad.mkws")
    r = run("fuseDecryptions", cc, tmp / f"sh0.{ext}", agg, tmp / "bad.json")
    assert r.returncode == 1 and "not a mkckks share blob" in r.stderr and not os.path.exists(tmp / "bad.json")
