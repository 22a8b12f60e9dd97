"""Compact distribution ciphertexts (include/mkckks.h: mkckks_compress_batch, mkckks_reencrypt_fanout_compact_batch;
serverRound --back-limbs, changeCipherDomain --limbs): what goes back to a client is only ever decrypted, so the back leg
is written at k limbs instead of the aggregate's L - 1.

Recipe (prefix(ct, m) = the first m limbs of both components): cut the aggregate to k + 1 limbs while it is at
noiseScaleDeg 2, key-switch at that level, rescale last:  out = Rescale(ReEncrypt(prefix(agg, k + 1), evk)).

Decrypt tolerance of the compact path -- measured with `measure_chain` below on the CPU oracle (3 clients, values uniform
in +-0.3, max error over all N/2 slots against the plaintext mean, seeds 0..5 per parameter set):

    parameters                     compact k = 1          compact k = 2          full back leg          compact / full
    N=2^12, depth 10, 50-bit       2^-38.22 .. 2^-37.69   2^-38.24 .. 2^-37.71   2^-39.87 .. 2^-39.38   2.2 .. 4.2
    N=2^14, depth 2, 40-bit        2^-26.01 .. 2^-25.75   2^-26.07 .. 2^-25.84   2^-27.72 .. 2^-27.17   2.3 .. 3.6

(k = 1 and k = 2 are alike: the closing rescale's rounding dominates both.)  Bounds = 4 x the largest value seen:
2^-35.69 at (12, 10, 50) and 2^-23.75 at (14, 2, 40) -- BOUND below; the margin is for the seed-to-seed spread of a
maximum over N/2 near-Gaussian errors and for the CLI drawing its own randomness.  Separately the compact chain must stay
within 16 x of the full back leg's error on the same inputs (the other order -- rescale, cut, key switch -- measured
34-243 x over six runs).

Headroom (constant slot vectors, every slot = A, so the whole magnitude sits in coefficient 0), 50-bit scaling: k = 1 holds
|values| < 2^(58-50) = 256; A = 250 decrypts at k = 1 (error 2^-38.33 .. 2^-37.62 over seeds 0..5), A = 10^4 decrypts at
k = 2 (2^-36.42 .. 2^-36.19; the full leg gives 2^-36.68 there) and wraps at k = 1 (error 2^13.3).  HEADROOM_BOUND = 4 x the
largest value seen, per case."""
import json
import os
import re
import struct

import numpy as np
import pytest

from tests.test_cli_hosts import _small_cc, _weights, run
from tests.test_gpu_parity import CONFIGS, make_keys, make_rk_rand, rand_ct
from tests.test_reencrypt_fanout import rand_evks
from tests.test_seeded_ciphertexts import read_mkws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mkckks_compress_batch", "mkckks_reencrypt_fanout_compact_batch")
PARAMS = {"p12": (12, 10, 50, 60, 3), "p14": (14, 2, 40, 60, 2)}  # p14 = tests.test_cli_hosts._small_cc
BOUND = {"p12": 4 * 2.0 ** -37.69, "p14": 4 * 2.0 ** -25.75}      # 4 x the largest measured error (docstring)
HEADROOM_BOUND = {(250.0, 1): 4 * 2.0 ** -37.62, (1.0e4, 2): 4 * 2.0 ** -36.19}


# ---- CPU: surface and argument checks -------------------------------------------------------------------------------

def test_compact_symbols_are_declared_bound_and_exported():
    from ppqsflhe_amd import Context, binding
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mkckks.h")).read(), flags=re.S)
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert sym in binding.SYMBOLS
        assert hasattr(binding.load_library(), sym)
    assert callable(getattr(Context, "compress", None))
    assert callable(getattr(Context, "reencrypt_fanout_compact", None))


def test_compact_argument_checks_on_a_host_only_context():
    from ppqsflhe_amd import Context
    from ppqsflhe_amd.binding import MkckksError
    c = Context(12, 2, 40, 60, dnum=2, device=-1)
    comp, fan = (getattr(c._L, s) for s in SYMBOLS)
    far = 1 << 40  # an output address far from the input's: pointers are never dereferenced
    try:
        L = c.L
        assert L >= 3
        # compress(ctx, in, out, n_ct, nl_in, nl_out)
        assert comp(c._h, None, far, 1, L, 1) == -1
        assert comp(c._h, 8, None, 1, L, 1) == -1
        assert comp(c._h, 8, far, 1, L, 0) == -1          # nl_out == 0
        assert comp(c._h, 8, far, 1, L, L) == -1          # nl_out >= nl_in
        assert comp(c._h, 8, far, 1, 2, 3) == -1
        assert comp(c._h, 8, far, 1, L + 1, 1) == -1      # nl_in > L
        assert comp(c._h, 8, 8, 1, L, 1) == -1            # output over input
        assert comp(c._h, 8, 8 + 8 * c.N, 1, L, 1) == -1  # output starting inside the input
        assert comp(c._h, 8, far, 1, L, 1) == -2
        assert comp(c._h, 8, far, 1, L, L - 1) == -2
        assert comp(c._h, 8, far, 0, L, 1) == 0
        # fanout_compact(ctx, ct, evks, out, n_keys, n_ct, nl_in, nl_out)
        assert fan(c._h, None, 8, far, 1, 1, L, 1) == -1
        assert fan(c._h, 8, None, far, 1, 1, L, 1) == -1
        assert fan(c._h, 8, 8, None, 1, 1, L, 1) == -1
        assert fan(c._h, 8, 8, far, 1, 1, L, 0) == -1
        assert fan(c._h, 8, 8, far, 1, 1, L, L) == -1
        assert fan(c._h, 8, 8, far, 1, 1, L + 1, 1) == -1
        assert fan(c._h, 8, 8, 8, 1, 1, L, 1) == -1
        assert fan(c._h, far + 8 * c.N, 8, far, 2, 1, L, 1) == -1  # input starting inside the second key's output
        assert fan(c._h, 8, 8, far, 1, 1, L, 1) == -2
        assert fan(c._h, 8, 8, far, 0, 1, L, 1) == 0
        assert fan(c._h, 8, 8, far, 1, 0, L, 1) == 0
        for call in (lambda: c.compress(8, far, 1, L, 1), lambda: c.reencrypt_fanout_compact(8, 8, far, 1, 1, L, 1)):
            with pytest.raises(MkckksError) as ei:
                call()
            assert ei.value.code == -2
    finally:
        c.close()


# ---- CPU: the recipe on the oracle ----------------------------------------------------------------------------------

def _oracle(name):
    from oracle.oracle import OracleContext
    a = PARAMS[name]
    return OracleContext(a[0], a[1], a[2], a[3], dnum=a[4])


def _chain_inputs(o, rng, vals):
    """3 clients' worth of a round on the oracle: encrypt vals[c] under client c, re-encrypt clients 0, 1 into client 2's
    domain, sum, EvalMult(., 1/3) -> the aggregate (L - 1 limbs, noiseScaleDeg 2), its scaling factor, the key client 2 ->
    client 0 and client 0's secret key."""
    from oracle.oracle import sample_gauss, sample_ternary
    N, L, n = o.N, o.L, len(vals)
    keys = []
    for _ in range(n):
        s, a, e = make_keys(o, rng)
        pk, sk = o.keygen(s, a, e)
        keys.append((s, pk, sk))
    tgt = n - 1
    acc = None
    for c in range(n):
        pt = o.encode(vals[c], o.sf_big(0), L)
        ct = o.encrypt(keys[c][1], pt, sample_ternary(rng, N), sample_gauss(rng, N), sample_gauss(rng, N))
        if c != tgt:
            ct = o.reencrypt(ct, o.rekeygen(keys[c][0], keys[tgt][1], *make_rk_rand(o, rng)))
        acc = ct if acc is None else o.eval_add(acc, ct)
    agg = o.mult_factors(o.rescale(acc), o.const_factors(L - 1, 1, 1.0 / n))
    scale = o.sf_big(0) / float(o.moduli[L - 1]) * o.sf(1)
    rk_back = o.rekeygen(keys[tgt][0], keys[0][1], *make_rk_rand(o, rng))
    return agg, scale, rk_back, keys[0][2]


def _compact(o, agg, scale, rk_back, k):
    """Rescale(ReEncrypt(prefix(agg, k + 1))) and its scaling factor."""
    return o.rescale(o.reencrypt(np.ascontiguousarray(agg[:, :k + 1]), rk_back)), scale / float(o.moduli[k])


def measure_chain(name, seed, ks=(1, 2)):
    """max |decrypted - mean| over all slots: {k: error of the compact chain}, error of the full back leg."""
    o = _oracle(name)
    rng = np.random.default_rng(seed)
    vals = rng.uniform(-0.3, 0.3, size=(3, o.N // 2))
    mean = vals.mean(axis=0)
    agg, scale, rk_back, sk0 = _chain_inputs(o, rng, vals)
    full = np.abs(o.decrypt_decode(o.reencrypt(agg, rk_back), sk0, scale) - mean).max()
    errs = {}
    for k in ks:
        ct, sc = _compact(o, agg, scale, rk_back, k)
        assert ct.shape == (2, k, o.N)
        errs[k] = np.abs(o.decrypt_decode(ct, sk0, sc) - mean).max()
    return errs, full


@pytest.mark.parametrize("name", ["p12", "p14"])
def test_oracle_compact_chain_decrypts_to_the_mean(name):
    errs, full = measure_chain(name, 11)
    for k, e in errs.items():
        print(f"{name} k={k}: compact 2^{np.log2(e):.2f}, full 2^{np.log2(full):.2f}, ratio {e / full:.2f}")
        assert e < BOUND[name], (name, k, e)
        assert e < 16 * full, (name, k, e, full)  # "compaction costs about two bits"; the wrong order costs 34-243 x


def test_oracle_headroom_rule_is_sharp():
    """(12, 10, 50): k = 1 holds |values| < 256.  Constant vectors put the whole magnitude into coefficient 0."""
    o = _oracle("p12")
    for A, k, good in ((250.0, 1, True), (1.0e4, 2, True), (1.0e4, 1, False)):
        rng = np.random.default_rng(int(A) + k)
        vals = np.full((3, o.N // 2), A)
        agg, scale, rk_back, sk0 = _chain_inputs(o, rng, vals)
        ct, sc = _compact(o, agg, scale, rk_back, k)
        err = np.abs(o.decrypt_decode(ct, sk0, sc) - A).max()
        print(f"A={A} k={k}: error 2^{np.log2(err):.2f}")
        if good:
            assert err < HEADROOM_BOUND[(A, k)], (A, k, err)
        else:
            assert err > 1.0, (A, k, err)


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctxs():
    from oracle.oracle import OracleContext
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


def prefix(ct, m):
    return np.ascontiguousarray(ct[..., :m, :])


def compress(g, ct, nl_out):
    B, nl_in = ct.shape[0], ct.shape[2]
    d_out = g.empty((B, 2, nl_out, g.N))
    g.compress(g.to_device(ct), d_out, B, nl_in, nl_out)
    return d_out.to_host()


def fanout_compact(g, ct, evks, nl_out):
    n_keys, B, nl_in = evks.shape[0], ct.shape[0], ct.shape[2]
    d_out = g.empty((n_keys, B, 2, nl_out, g.N))
    g.reencrypt_fanout_compact(g.to_device(ct), g.to_device(evks), d_out, n_keys, B, nl_in, nl_out)
    return d_out.to_host()


def check_fanout_compact(g, o, ct, evks, nl_out, tag):
    got = fanout_compact(g, ct, evks, nl_out)
    for k in range(evks.shape[0]):
        for b in range(ct.shape[0]):
            exp = o.rescale(o.reencrypt(prefix(ct[b], nl_out + 1), evks[k]))
            assert np.array_equal(got[k, b], exp), (tag, nl_out, k, b)


def _limb_pairs(L):
    """(nl_in, nl_out): nl_in = L and L - 1; nl_out = 1, 2, 3 and nl_in - 1."""
    out = []
    for nl_in in (L, L - 1):
        for nl_out in sorted({1, 2, 3, nl_in - 1}):
            if 1 <= nl_out < nl_in:
                out.append((nl_in, nl_out))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "ref", "c3", "n17", "n11"])
def test_compress_matches_the_oracle(ctxs, name):
    g, o = ctxs(name)
    B = 3 if g.N <= 1 << 14 else 2
    for nl_in, nl_out in _limb_pairs(g.L):
        rng = np.random.default_rng(100 * nl_in + nl_out)
        ct = rand_ct(rng, g, nl_in, B)
        got = compress(g, ct, nl_out)
        for b in range(B):
            assert np.array_equal(got[b], o.rescale(prefix(ct[b], nl_out + 1))), (name, nl_in, nl_out, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl_in,nl_out,n_keys,B", [
    ("tiny", 5, 1, 3, 2), ("tiny", 4, 2, 2, 2),
    ("ref", 4, 1, 3, 3), ("ref", 3, 2, 2, 2),
    ("c3", 11, 1, 3, 2), ("c3", 11, 2, 2, 2),
    ("c3", 11, 4, 2, 1),   # 5 limbs: two digits
    ("c3", 12, 1, 2, 1),
    ("c5s", 19, 1, 2, 2),
    ("c5s", 19, 7, 2, 1),  # 8 limbs: a full digit and a one-limb second digit
    ("n17", 4, 2, 2, 1), ("n17", 4, 1, 2, 1),
    ("n11", 4, 1, 2, 2), ("n11", 4, 3, 2, 2)])
def test_fanout_compact_matches_the_oracle_chain(ctxs, name, nl_in, nl_out, n_keys, B):
    g, o = ctxs(name)
    rng = np.random.default_rng(2000 + 31 * nl_in + 7 * nl_out + n_keys)
    check_fanout_compact(g, o, rand_ct(rng, g, nl_in, B), rand_evks(rng, g, n_keys), nl_out, name)


@pytest.mark.gpu
def test_fanout_compact_n17_at_its_real_limb_structure():
    """N = 2^17, L = 20, dnum = 3 (alpha = K = 7): 19 -> 1, every word against the oracle chain."""
    from oracle.oracle import OracleContext
    from ppqsflhe_amd import Context
    g, o = Context(17, 18, 50, 60, dnum=3, device=0), OracleContext(17, 18, 50, 60, dnum=3)
    try:
        rng = np.random.default_rng(1719)
        check_fanout_compact(g, o, rand_ct(rng, g, 19, 1), rand_evks(rng, g, 2), 1, "n17-real")
    finally:
        g.close()


def _composition(g, d_evks, ct, n_keys, nl_out):
    """packed prefix copy -> reencrypt_fanout -> rescale, on the device."""
    B, nl = ct.shape[0], nl_out + 1
    d_pre = g.to_device(prefix(ct, nl))
    d_ks = g.empty((n_keys, B, 2, nl, g.N))
    g.reencrypt_fanout(d_pre, d_evks, d_ks, n_keys, B, nl)
    d_out = g.empty((n_keys * B, 2, nl_out, g.N))
    g.rescale(d_ks, d_out, n_keys * B, nl)
    return d_out.to_host().reshape(n_keys, B, 2, nl_out, g.N)


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl_in,nl_out,n_keys,B", [
    ("ref", 3, 1, 9, 19),    # more keys than one group, more ciphertexts than one chunk
    ("ref", 3, 2, 9, 19),
    ("c3", 11, 1, 7, 16)])   # the real back leg at its real batch
def test_fanout_compact_equals_the_composition_on_the_device(ctxs, name, nl_in, nl_out, n_keys, B):
    g, _ = ctxs(name)
    rng = np.random.default_rng(13 * n_keys + B + nl_out)
    ct, evks = rand_ct(rng, g, nl_in, B), rand_evks(rng, g, n_keys)
    d_evks = g.to_device(evks)
    d_out = g.empty((n_keys, B, 2, nl_out, g.N))
    g.reencrypt_fanout_compact(g.to_device(ct), d_evks, d_out, n_keys, B, nl_in, nl_out)
    assert np.array_equal(d_out.to_host(), _composition(g, d_evks, ct, n_keys, nl_out)), name


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl_in", [("c3", 11), ("ref", 3)])
def test_compact_extreme_residues(ctxs, name, nl_in):
    """Maximal operands (the pattern of test_fanout_extreme_residues): every residue q - 1, all 0, alternating."""
    g, o = ctxs(name)
    B, n_keys = 3, 2
    idx = np.arange(g.N)
    ct = np.zeros((B, 2, nl_in, g.N), dtype=np.uint64)
    evks = np.zeros((n_keys, g.beta, 2, g.D, g.N), dtype=np.uint64)
    for b, m in ((0, np.ones(g.N, dtype=bool)), (2, (idx // 8) % 2 == 0)):  # ciphertext 1 stays all 0
        for l in range(nl_in):
            ct[b, :, l, m] = int(g.moduli[l]) - 1
    for k in range(n_keys):
        m = np.ones(g.N, dtype=bool) if k == 0 else ((idx // (1 << (3 * k))) % 2 == 0)
        for l in range(g.D):
            evks[k, :, :, l, m] = int(g.moduli[l]) - 1
    for nl_out in (1, 2):
        check_fanout_compact(g, o, ct, evks, nl_out, name + "-extreme")
        got = compress(g, ct, nl_out)
        for b in range(B):
            assert np.array_equal(got[b], o.rescale(prefix(ct[b], nl_out + 1))), (name, nl_out, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl_in", [("c3", 11), ("ref", 3)])
@pytest.mark.parametrize("env", [{"MKCKKS_FANOUT_GROUP": "1"}, {"MKCKKS_FANOUT_GROUP": "3"}, {"MKCKKS_CHUNK": "1"},
                                 {"MKCKKS_GENERIC_NTT": "1"}, {"MKCKKS_NO_PM": "1"}, {"MKCKKS_NO_FP64": "1"}])
def test_compact_under_the_library_switches(ctxs, monkeypatch, env, name, nl_in):
    """Switches are read once, when a context is created: a fresh context under each must give the oracle's bits (at two
    limbs MKCKKS_NO_FP64 takes the per-key path, the default the fused one)."""
    from ppqsflhe_amd import Context
    _, o = ctxs(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a = CONFIGS[name]
    g = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)
    try:
        rng = np.random.default_rng(66 + nl_in)
        ct, evks = rand_ct(rng, g, nl_in, 2), rand_evks(rng, g, 4)
        for nl_out in (1, 2):
            check_fanout_compact(g, o, ct, evks, nl_out, (name, env))
        got = compress(g, ct, 1)
        for b in range(2):
            assert np.array_equal(got[b], o.rescale(prefix(ct[b], 2))), (name, env, b)
    finally:
        g.close()


@pytest.mark.gpu
def test_compact_call_properties(ctxs):
    """Two calls give the same bits; the input is not written (the limbs beyond the prefix included); overlap is refused;
    empty calls write nothing; words of the output array beyond the result are untouched."""
    from ppqsflhe_amd.binding import MkckksError
    g, _ = ctxs("c3")
    nl_in, nl_out, n_keys, B = 11, 1, 3, 2
    rng = np.random.default_rng(4343)
    ct, evks = rand_ct(rng, g, nl_in, B), rand_evks(rng, g, n_keys)
    d_ct, d_evks = g.to_device(ct), g.to_device(evks)
    POISON = 0xA5A5A5A5A5A5A5A5
    out_words, pad = n_keys * B * 2 * nl_out * g.N, 4 * g.N
    d_big = g.to_device(np.full(out_words + pad, POISON, dtype=np.uint64))
    d_out = d_big.view(0, (n_keys, B, 2, nl_out, g.N))
    g.reencrypt_fanout_compact(d_ct, d_evks, d_out, n_keys, B, nl_in, nl_out)
    first = d_out.to_host()
    assert np.all(d_big.to_host()[out_words:] == POISON)
    g.reencrypt_fanout_compact(d_ct, d_evks, d_out, n_keys, B, nl_in, nl_out)
    assert np.array_equal(d_out.to_host(), first)
    assert np.array_equal(d_ct.to_host(), ct)
    c_words = B * 2 * nl_out * g.N
    d_cbig = g.to_device(np.full(c_words + pad, POISON, dtype=np.uint64))
    d_c = d_cbig.view(0, (B, 2, nl_out, g.N))
    g.compress(d_ct, d_c, B, nl_in, nl_out)
    c_first = d_c.to_host()
    assert np.all(d_cbig.to_host()[c_words:] == POISON)
    g.compress(d_ct, d_c, B, nl_in, nl_out)
    assert np.array_equal(d_c.to_host(), c_first)
    assert np.array_equal(d_ct.to_host(), ct)
    # overlap: output over the input, output inside the limbs beyond the prefix
    in_words = B * 2 * nl_in * g.N
    for call in (lambda: g.reencrypt_fanout_compact(d_ct, d_evks, d_ct, 1, B, nl_in, nl_out),
                 lambda: g.reencrypt_fanout_compact(d_ct, d_evks, d_ct.view(in_words - g.N, (g.N,)), 1, B, nl_in, nl_out),
                 lambda: g.compress(d_ct, d_ct, B, nl_in, nl_out),
                 lambda: g.compress(d_ct, d_ct.view(in_words - g.N, (g.N,)), B, nl_in, nl_out)):
        with pytest.raises(MkckksError) as ei:
            call()
        assert ei.value.code == -1
    assert np.array_equal(d_ct.to_host(), ct)
    # empty calls leave the output alone
    d_out.upload(np.full(first.shape, POISON, dtype=np.uint64))
    g.reencrypt_fanout_compact(d_ct, d_evks, d_out, 0, B, nl_in, nl_out)
    g.reencrypt_fanout_compact(d_ct, d_evks, d_out, n_keys, 0, nl_in, nl_out)
    g.compress(d_ct, d_out, 0, nl_in, nl_out)
    assert np.all(d_out.to_host() == POISON)


@pytest.mark.gpu
@pytest.mark.parametrize("nl_out", [1, 2])
def test_client_decrypts_and_decodes_a_compact_ciphertext(ctxs, nl_out):
    """Client end at 1 and 2 limbs: decrypt + decode on the device against the oracle's decrypt_decode (the decode tolerance
    of tests/test_gpu_parity.py, 2^-40)."""
    g, o = ctxs("ref")
    rng = np.random.default_rng(500 + nl_out)
    vals = rng.uniform(-0.3, 0.3, size=(3, o.N // 2))
    agg, scale, rk_back, sk0 = _chain_inputs(o, rng, vals)
    nl_in = agg.shape[1]
    got = fanout_compact(g, agg[None], rk_back[None], nl_out)[0, 0]
    exp, sc = _compact(o, agg, scale, rk_back, nl_out)
    assert np.array_equal(got, exp) and nl_in == g.L - 1
    d_m, d_vals = g.empty((1, nl_out, g.N)), g.empty((1, g.N // 2), dtype=np.float64)
    g.decrypt(g.to_device(got[None]), g.to_device(sk0), d_m, 1, nl_out)
    g.decode(d_m, d_vals, 1, nl_out, sc)
    ref = o.decrypt_decode(exp, sk0, sc)
    assert np.abs(d_vals.to_host()[0] - ref).max() < 2.0 ** -40
    assert np.abs(ref - vals.mean(axis=0)).max() < BOUND["p14"]


# ---- GPU: the distribution leg of serverRound -----------------------------------------------------------------------

def _ok(r):
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _same_bytes(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


def _round_inputs(tmp_path, n, ext, seed):
    """n clients with keys and encrypted weights, inbound keys towards client n-1, one back key per other client."""
    cc = _small_cc(tmp_path)
    rng = np.random.default_rng(seed)
    vals = [[("dense", rng.uniform(-0.3, 0.3, 2 * 8192 + 300)), ("bias", rng.uniform(-0.3, 0.3, 4))] for _ in range(n)]
    for c in range(n):
        _ok(run("keyGen", cc, tmp_path / f"pk{c}", tmp_path / f"sk{c}"))
        _ok(run("encryptModelWeights", cc, tmp_path / f"pk{c}", _weights(tmp_path, f"w{c}.json", vals[c]),
                tmp_path / f"enc{c}.{ext}"))
    target = n - 1
    args, back_keys = ["-", tmp_path / f"enc{target}.{ext}"], []
    for c in range(n - 1):
        _ok(run("REkeyGen", cc, tmp_path / f"sk{c}", tmp_path / f"pk{target}", tmp_path / f"rk{c}"))
        _ok(run("REkeyGen", cc, tmp_path / f"sk{target}", tmp_path / f"pk{c}", tmp_path / f"rkback{c}"))
        args += [tmp_path / f"rk{c}", tmp_path / f"enc{c}.{ext}"]
        back_keys.append(tmp_path / f"rkback{c}")
    back_keys.append("-")  # the target client: already in its own domain
    return cc, vals, args, back_keys


def _blobs(path, ext):
    """every ciphertext container of an envelope, as raw bytes"""
    import base64
    if ext == "mkws":
        return [bytes(b) for b in read_mkws(path)[1]]
    out = []
    for lay in json.load(open(path))["weights_summary"]:
        out += [base64.b64decode(x) for x in [lay["mean"], lay["std_dev"], *lay["values"]]]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ext", ["json", "mkws"])
def test_server_round_back_limbs(tmp_path, ext):
    """A 4-client round with --back rk0 f0 rk1 f1 rk2 f2 - f3 --back-limbs 1: every file equals changeCipherDomain --limbs 1
    on the aggregate file, carries 1-limb blobs of 48 + 16 N bytes, and decrypts to the mean under its own key only."""
    n, N, L = 4, 1 << 14, 4
    cc, vals, args, back_keys = _round_inputs(tmp_path, n, ext, 600 + len(ext))

    def back(tag):
        return [x for c in range(n) for x in (back_keys[c], tmp_path / f"{tag}{c}.{ext}")]

    _ok(run("serverRound", cc, tmp_path / f"plain.{ext}", *args, "--back", *back("full")[:-2]))
    r = _ok(run("serverRound", cc, tmp_path / f"agg.{ext}", *args, "--back", *back("for"), "--back-limbs", "1"))
    assert re.search(r"\[round\] back leg: 4 keys x \d+ ciphertexts in \S+ ms -> \S+ ciphertexts/s, 3 key\(s\) uploaded, 1 limbs",
                     r.stdout), r.stdout
    assert _same_bytes(tmp_path / f"agg.{ext}", tmp_path / f"plain.{ext}")  # the aggregate is never compacted
    _ok(run("serverRound", cc, tmp_path / f"aggL.{ext}", *args, "--back", *back("loop"), "--back-limbs", "1",
            env={"MKCKKS_BACK_LOOP": "1"}))
    _ok(run("serverRound", cc, tmp_path / f"aggS.{ext}", *args, "--back", *back("sync"), "--back-limbs", "1",
            env={"MKCKKS_SYNC_IO": "1"}))
    lines = [" ".join(map(str, [tmp_path / f"r{rd}.{ext}", *args, "--back", *back(f"r{rd}_"), "--back-limbs", "1"]))
             for rd in range(2)]
    (tmp_path / "rounds.txt").write_text("\n".join(lines) + "\n")
    rr = _ok(run("serverRound", cc, "--rounds", tmp_path / "rounds.txt"))
    assert re.findall(r"(\d+) key\(s\) uploaded, 1 limbs", rr.stdout) == ["3", "0"]
    mean = [np.mean([np.asarray(vals[c][li][1]) for c in range(n)], axis=0) for li in range(2)]
    for c in range(n):
        f = tmp_path / f"for{c}.{ext}"
        _ok(run("changeCipherDomain", cc, back_keys[c], tmp_path / f"agg.{ext}", tmp_path / f"ref{c}.{ext}", "--limbs", "1"))
        for other in (f"ref{c}", f"loop{c}", f"sync{c}", f"r0_{c}", f"r1_{c}"):
            assert _same_bytes(f, tmp_path / f"{other}.{ext}"), (c, other)
        blobs = _blobs(f, ext)
        assert len(blobs) == (2 + 3) + (2 + 1)  # per layer: mean, std_dev, values (3 ciphertexts of 8192 slots; 1)
        for b in blobs:
            assert len(b) == 48 + 16 * N
            magic, ver, kind, ring, limbs, parts, level, deg = struct.unpack_from("<4s7I", b, 0)
            assert (magic, kind, ring, limbs, parts, level, deg) == (b"MKCK", 1, N, 1, 2, L - 1, 1)
        if c < n - 1:  # the same leg without the flag: L - 1 limbs
            assert len(_blobs(tmp_path / f"full{c}.{ext}", ext)[0]) == 48 + 16 * (L - 1) * N
        _ok(run("decryptModelWeights", cc, tmp_path / f"sk{c}", f, tmp_path / f"dec{c}.json"))
        dec = json.load(open(tmp_path / f"dec{c}.json"))["weights_summary"]
        for li in range(2):
            assert np.abs(np.array(dec[li]["values"]) - mean[li]).max() < BOUND["p14"], (c, li)
        wrong = run("decryptModelWeights", cc, tmp_path / f"sk{(c + 1) % n}", f, tmp_path / f"bad{c}.json")
        if wrong.returncode == 0:
            bad = json.load(open(tmp_path / f"bad{c}.json"))["weights_summary"]
            assert np.abs(np.array(bad[0]["values"]) - mean[0]).max() > 1.0, c


@pytest.mark.gpu
def test_server_round_back_limbs_argument_errors(tmp_path):
    """--back-limbs 0, 3 on a 3-limb aggregate, a missing value, and - in --back without --back-limbs: exit 1, no back file,
    no aggregate file; changeCipherDomain --limbs refuses the same."""
    n = 3
    cc, _, args, back_keys = _round_inputs(tmp_path, n, "mkws", 31)
    outs = [tmp_path / f"o{c}.mkws" for c in range(n)]
    back = [x for c in range(n) for x in (back_keys[c], outs[c])]
    for tail in (["--back", *back, "--back-limbs", "0"], ["--back", *back, "--back-limbs", "3"],
                 ["--back", *back, "--back-limbs"], ["--back", *back]):
        r = run("serverRound", cc, tmp_path / "agg.mkws", *args, *tail)
        assert r.returncode == 1, (tail[-2:], r.stdout + r.stderr)
        assert not any(os.path.exists(o) for o in outs) and not os.path.exists(tmp_path / "agg.mkws"), tail[-2:]
        if tail[-1] in ("0", "3") or tail[-1] == outs[-1]:
            assert "[round] ERROR" in r.stderr, r.stderr
    _ok(run("serverRound", cc, tmp_path / "agg.mkws", *args, "--back", *back, "--back-limbs", "2"))
    for c in range(n):
        _ok(run("changeCipherDomain", cc, back_keys[c], tmp_path / "agg.mkws", tmp_path / f"ref{c}.mkws", "--limbs", "2"))
        assert _same_bytes(outs[c], tmp_path / f"ref{c}.mkws"), c
    for bad_args in ((back_keys[0], tmp_path / "agg.mkws", tmp_path / "x.mkws", "--limbs", "3"),
                     (back_keys[0], tmp_path / "agg.mkws", tmp_path / "x.mkws", "--limbs", "0"),
                     (back_keys[0], outs[0], tmp_path / "x.mkws", "--limbs", "1")):  # input at noiseScaleDeg 1
        r = run("changeCipherDomain", cc, *bad_args)
        assert r.returncode == 1 and "[recrypt] ERROR" in r.stderr, r.stdout + r.stderr
        assert not os.path.exists(tmp_path / "x.mkws")
