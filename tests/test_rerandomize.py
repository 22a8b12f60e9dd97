"""HRA-secure re-encryption (include/mkckks.h: mkckks_sample_gauss_wide, mkckks_rerandomize_batch; changeCipherDomain
--hra, serverRound --hra-back): cc->ReEncrypt(ct, reKey, publicKey) = re-randomise with an encryption of zero under the
source domain's public key, errors from a wide Gaussian, then the key switch.

    out[t][0][i] = ct[t][0][i] + pk[0][i] * NTT_i(v_t) + NTT_i(e0_t)   mod q_i
    out[t][1][i] = ct[t][1][i] + pk[1][i] * NTT_i(v_t) + NTT_i(e1_t)   mod q_i

The outputs are canonical residues, so every GPU comparison is word for word.  Two references: the oracle's
encrypt(pk, 0, v, e0, e1) + eval_add for errors that fit int32, and `exact_rerandomize` below for 62-bit errors (the error
is reduced mod q_i in exact int64 arithmetic, transformed by the oracle's ntt_fwd and added; b * V comes from the oracle's
encrypt with zero errors).

Noise (CPU oracle, chain of tests/test_compact_downlink.py with 3 clients): the mask adds e0 + e1 * s under the target's
key, standard deviation sigma * sqrt(1 + h) per coefficient (h = non-zero coefficients of s); measured 0.970 .. 1.013 of
that; the test allows +-10 % for the correlation between the coefficients of e1 * s."""
import copy
import os
import re

import numpy as np
import pytest

from tests.test_cli_hosts import _small_cc, run
from tests.test_compact_downlink import (BOUND, PARAMS, _chain_inputs, _compact, _ok, _oracle, _round_inputs, _same_bytes,
                                         prefix)
from tests.test_gpu_parity import CONFIGS, make_keys, rand_ct, rand_polys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mkckks_sample_gauss_wide", "mkckks_rerandomize_batch")
KEY = bytes(range(32))
EMAX = (1 << 62) - 1


# ---- CPU: surface and argument checks -------------------------------------------------------------------------------

def test_rerandomize_symbols_are_declared_bound_and_exported():
    from ppqsflhe_amd import Context, binding
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mkckks.h")).read(), flags=re.S)
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert sym in binding.SYMBOLS
        assert hasattr(binding.load_library(), sym)
    assert callable(getattr(Context, "sample_gauss_wide", None))
    assert callable(getattr(Context, "rerandomize", None))


def test_rerandomize_argument_checks_on_a_host_only_context():
    from ppqsflhe_amd import Context
    from ppqsflhe_amd.binding import MkckksError
    c = Context(12, 2, 40, 60, dnum=2, device=-1)
    samp, rr = (getattr(c._L, s) for s in SYMBOLS)
    far = 1 << 40  # an output address far from the input's: pointers are never dereferenced
    try:
        L = c.L
        assert L >= 3
        # sample_gauss_wide(ctx, out, count, sigma, key, sid)
        assert samp(c._h, None, 8, 2.0 ** 20, KEY, 0) == -1
        assert samp(c._h, 8, 8, 2.0 ** 20, None, 0) == -1
        for sigma in (2.0 ** 6 * (1 - 2.0 ** -50), 1.0, 0.0, -2.0 ** 20, 2.0 ** 56 * (1 + 2.0 ** -50), float("inf"), float("nan")):
            assert samp(c._h, 8, 8, sigma, KEY, 0) == -1, sigma
        for sigma in (2.0 ** 6, 2.0 ** 20, 2.0 ** 56):
            assert samp(c._h, 8, 8, sigma, KEY, 0) == -2, sigma
        assert samp(c._h, 8, 0, 2.0 ** 20, KEY, 0) == 0
        # rerandomize(ctx, ct, pk, v, e0, e1, out, n_ct, nl_in, nl)
        good = [8, 8, 8, 8, 8, far]
        for i in range(6):
            args = list(good)
            args[i] = None
            assert rr(c._h, *args, 1, L, L) == -1, i
        assert rr(c._h, *good, 1, L, 0) == -1            # nl == 0
        assert rr(c._h, *good, 1, 2, 3) == -1            # nl > nl_in
        assert rr(c._h, *good, 1, L + 1, 1) == -1        # nl_in > L
        assert rr(c._h, *good, 1, L + 1, L + 1) == -1
        assert rr(c._h, 8, 8, 8, 8, 8, 8, 1, L, L - 1) == -1              # output over input with nl_in != nl
        assert rr(c._h, 8, 8, 8, 8, 8, 8 + 8 * c.N, 1, L, L) == -1        # output starting inside the input
        assert rr(c._h, 8, 8, 8, 8, 8, 8 + 8 * c.N, 1, L, 1) == -1
        assert rr(c._h, far + 8 * c.N, 8, 8, 8, 8, far, 2, L, 1) == -1    # input starting inside the output
        assert rr(c._h, *good, 1, L, L) == -2
        assert rr(c._h, *good, 1, L, 1) == -2
        assert rr(c._h, 8, 8, 8, 8, 8, 8, 1, L, L) == -2                  # in place
        assert rr(c._h, *good, 0, L, L) == 0
        assert rr(c._h, 8, 8, 8, 8, 8, 8, 0, L, L) == 0
        for call in (lambda: c.rerandomize(8, 8, 8, 8, 8, far, 1, L, 1), lambda: c.sample_gauss_wide(8, 8, 2.0 ** 20, KEY)):
            with pytest.raises(MkckksError) as ei:
                call()
            assert ei.value.code == -2
        with pytest.raises(MkckksError) as ei:
            c.sample_gauss_wide(8, 8, 32.0, KEY)
        assert ei.value.code == -1
    finally:
        c.close()


def test_hra_command_line_errors(tmp_path):
    """Every misuse of the new switches: exit 1 with its message, nothing written (no device is reached)."""
    cc = _small_cc(tmp_path)
    out = tmp_path / "out.mkws"
    cases = [
        (("rk", "in", out, "--hra", tmp_path / "nokey"), "[recrypt] ERROR: Failed to load public key from"),
        (("rk", "in", out, "--limbs", "1", "--hra", tmp_path / "nokey"), "[recrypt] ERROR: Failed to load public key from"),
        (("rk", "in", out, "--hra", "pk", "--hra-sigma-bits", "5"), "[recrypt] ERROR: --hra-sigma-bits needs an integer in [6, 56]"),
        (("rk", "in", out, "--hra", "pk", "--hra-sigma-bits", "57"), "[recrypt] ERROR: --hra-sigma-bits needs an integer in [6, 56]"),
        (("rk", "in", out, "--hra", "pk", "--hra-sigma-bits", "x"), "[recrypt] ERROR: --hra-sigma-bits needs an integer in [6, 56]"),
        (("-", "in", out, "--hra", "pk"), "[recrypt] ERROR: --hra with - as the re-encryption key needs --limbs"),
        (("rk", "in", out, "--hra"), "Usage:"),
        (("rk", "in", out, "--hra-sigma-bits", "20"), "Usage:"),
    ]
    for args, msg in cases:
        r = run("changeCipherDomain", cc, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stdout + r.stderr)
        assert not os.path.exists(out), args
    for tail in (["--hra-back", "pk"], ["--hra-back", "pk", "--hra-sigma-bits", "20"], ["--hra-sigma-bits", "20"]):
        r = run("serverRound", cc, out, "-", "in", *tail)  # no --back list
        assert r.returncode == 1 and "Usage:" in r.stderr, (tail, r.stdout + r.stderr)
        assert not os.path.exists(out), tail


# ---- CPU: the noise of the re-randomisation on the oracle -----------------------------------------------------------

def exact_rerandomize(o, ct, pk, v, e0, e1, nl):
    """first nl limbs of ct [2][nl_in][N] + Enc_pk(0; v, e0, e1) for int64 errors, in exact integer arithmetic."""
    N = o.N
    zero_e = np.zeros(N, dtype=np.int32)
    z = o.encrypt(pk, np.zeros((nl, N), dtype=np.uint64), v, zero_e, zero_e)  # (b V, a V)
    out = np.empty((2, nl, N), dtype=np.uint64)
    for comp, e in ((0, e0), (1, e1)):
        for i in range(nl):
            q = int(o.moduli[i])
            lifted = np.mod(np.asarray(e, dtype=np.int64), np.int64(q)).astype(np.uint64)  # floor mod: in [0, q), exact
            s = (ct[comp, i] + z[comp, i]) % np.uint64(q)                                   # < 2^61: no wrap
            out[comp, i] = (s + o.ntt_fwd(i, lifted)) % np.uint64(q)
    return out


def wide_errors(rng, n, sigma):
    e = np.rint(rng.normal(0.0, sigma, size=n)).astype(np.int64)
    assert np.abs(e).max() < 2 ** 31  # the oracle's encrypt takes int32
    return e


_CHAINS = {}


def hra_chain(name):
    """The chain of test_compact_downlink (seed 11) plus the target domain's keys: the helper draws its key material first,
    so a copy of the generator taken before the call re-derives it."""
    if name not in _CHAINS:
        o = _oracle(name)
        rng = np.random.default_rng(11)
        vals = rng.uniform(-0.3, 0.3, size=(3, o.N // 2))
        rng_keys = copy.deepcopy(rng)
        agg, scale, rk_back, sk0 = _chain_inputs(o, rng, vals)
        tgt = None
        for _ in range(3):
            s, a, e = make_keys(o, rng_keys)
            tgt = (s,) + tuple(o.keygen(s, a, e))  # (ternary secret, pk, sk) of the last client = the aggregate's domain
        _CHAINS[name] = dict(o=o, rng=rng, mean=vals.mean(axis=0), agg=agg, scale=scale, rk_back=rk_back, sk0=sk0, tgt=tgt)
    return _CHAINS[name]


def centred(m, q):
    m = m.astype(np.int64)
    return np.where(m > q // 2, m - q, m)


@pytest.mark.parametrize("sigma_bits", [20, 28])
@pytest.mark.parametrize("name", ["p12", "p14"])
def test_oracle_hra_noise_and_precision(name, sigma_bits):
    from oracle.oracle import sample_ternary
    ch = hra_chain(name)
    o, agg, scale, rk_back, sk0 = ch["o"], ch["agg"], ch["scale"], ch["rk_back"], ch["sk0"]
    s_tgt, pk_tgt, sk_tgt = ch["tgt"]
    rng = np.random.default_rng(1000 + sigma_bits)
    sigma, nl = 2.0 ** sigma_bits, agg.shape[1]
    v, e0, e1 = sample_ternary(rng, o.N), wide_errors(rng, o.N, sigma), wide_errors(rng, o.N, sigma)
    rr = o.eval_add(agg, o.encrypt(pk_tgt, np.zeros((nl, o.N), dtype=np.uint64), v, e0, e1))
    assert np.array_equal(rr, exact_rerandomize(o, agg, pk_tgt, v, e0, e1, nl))
    # the added noise under the target's key, limb 0
    q0 = int(o.moduli[0])
    d = centred((o.decrypt_core(rr, sk_tgt)[0] + np.uint64(q0) - o.decrypt_core(agg, sk_tgt)[0]) % np.uint64(q0), q0)
    h = int(np.count_nonzero(s_tgt))
    ratio = d.std() / (sigma * np.sqrt(1.0 + h))
    print(f"{name} sigma 2^{sigma_bits}: added noise std / (sigma sqrt(1 + h)) = {ratio:.4f} (h = {h})")
    assert 0.9 < ratio < 1.1, (name, sigma_bits, ratio)
    mean = ch["mean"]
    plain = np.abs(o.decrypt_decode(o.reencrypt(agg, rk_back), sk0, scale) - mean).max()
    full = np.abs(o.decrypt_decode(o.reencrypt(rr, rk_back), sk0, scale) - mean).max()
    ct, sc = _compact(o, rr, scale, rk_back, 1)
    compact = np.abs(o.decrypt_decode(ct, sk0, sc) - mean).max()
    print(f"{name} sigma 2^{sigma_bits}: full leg 2^{np.log2(plain):.2f} -> 2^{np.log2(full):.2f} with HRA, "
          f"HRA + compact k = 1: 2^{np.log2(compact):.2f}")
    assert full < 2 * plain, (name, sigma_bits, full, plain)
    assert compact < BOUND[name], (name, sigma_bits, compact)


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


def rand_pk(rng, g):
    return rand_polys(rng, g, list(range(g.D)) * 2, 1).reshape(2, g.D, g.N)


def rerandomize(g, ct, pk, v, e0, e1, nl, in_place=False):
    B, nl_in = ct.shape[0], ct.shape[2]
    d_ct = g.to_device(ct)
    d_out = d_ct if in_place else g.empty((B, 2, nl, g.N))
    g.rerandomize(d_ct, g.to_device(pk), g.to_device(v, np.int8), g.to_device(e0, np.int64), g.to_device(e1, np.int64), d_out,
                  B, nl_in, nl)
    return d_out.to_host().reshape(B, 2, nl, g.N)


def narrow_inputs(rng, g, nl_in, B):
    from oracle.oracle import sample_ternary
    v = np.stack([sample_ternary(rng, g.N) for _ in range(B)])
    e0 = rng.integers(-2 ** 31, 2 ** 31, size=(B, g.N), dtype=np.int64)
    e1 = rng.integers(-2 ** 31, 2 ** 31, size=(B, g.N), dtype=np.int64)
    e0[:, :2], e1[:, :2] = [-2 ** 31, 2 ** 31 - 1], [2 ** 31 - 1, -2 ** 31]
    return rand_ct(rng, g, nl_in, B), rand_pk(rng, g), v, e0, e1


def wide_inputs(rng, g, nl_in, B, signs=(1, -1)):
    """e uniform in +-2^59 with planted extremes; v all +1 (item 0), all -1 (item 1), ternary after that."""
    from oracle.oracle import sample_ternary
    v = np.stack([np.full(g.N, signs[b], dtype=np.int8) if b < len(signs) else sample_ternary(rng, g.N) for b in range(B)])
    e0 = rng.integers(-2 ** 59, 2 ** 59, size=(B, g.N), dtype=np.int64)
    e1 = rng.integers(-2 ** 59, 2 ** 59, size=(B, g.N), dtype=np.int64)
    plant = np.array([EMAX, -EMAX, 0, 1, -1], dtype=np.int64)
    e0[:, :5], e1[:, -5:] = plant, plant[::-1]
    e0[:, g.N // 2 + 3], e1[:, g.N // 2 - 3] = -EMAX, EMAX
    return rand_ct(rng, g, nl_in, B), rand_pk(rng, g), v, e0, e1


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl_in,nl,B", [
    ("c1", 3, 3, 3), ("ref", 4, 4, 3), ("ref", 3, 3, 3),
    ("c3", 12, 12, 3), ("c3", 11, 11, 3), ("c3", 11, 2, 3), ("c3", 12, 12, 1),
    ("c5s", 20, 20, 3), ("tiny", 5, 5, 3), ("n17", 4, 4, 3), ("n11", 4, 4, 3)])
def test_rerandomize_matches_the_oracle(ctxs, name, nl_in, nl, B):
    """Errors that fit int32: the oracle's encrypt of zero, added with eval_add."""
    g, o = ctxs(name)
    rng = np.random.default_rng(300 + 17 * nl_in + nl + B)
    ct, pk, v, e0, e1 = narrow_inputs(rng, g, nl_in, B)
    got = rerandomize(g, ct, pk, v, e0, e1, nl)
    zero = np.zeros((nl, g.N), dtype=np.uint64)
    for b in range(B):
        exp = o.eval_add(prefix(ct[b], nl), o.encrypt(pk, zero, v[b], e0[b].astype(np.int32), e1[b].astype(np.int32)))
        assert np.array_equal(got[b], exp), (name, nl_in, nl, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl,B", [("c1", 3, 3), ("ref", 4, 3), ("n11", 4, 3), ("c3", 12, 1)])
def test_rerandomize_wide_errors_are_exact(ctxs, name, nl, B):
    """62-bit errors against exact integers (the fp64-class limbs hold 53 bits: the lift must not go through them)."""
    g, o = ctxs(name)
    rng = np.random.default_rng(900 + nl)
    for signs in ((1, -1),) if B > 1 else ((1,), (-1,)):
        ct, pk, v, e0, e1 = wide_inputs(rng, g, nl, B, signs)
        got = rerandomize(g, ct, pk, v, e0, e1, nl)
        for b in range(B):
            assert np.array_equal(got[b], exact_rerandomize(o, ct[b], pk, v[b], e0[b], e1[b], nl)), (name, signs, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl", [("c3", 12), ("ref", 4)])
def test_rerandomize_extreme_residues(ctxs, name, nl):
    """Every word of ct and pk at q_i - 1, every |e| at the bound 2^62 - 1."""
    g, o = ctxs(name)
    B = 2
    ct = np.empty((B, 2, nl, g.N), dtype=np.uint64)
    pk = np.empty((2, g.D, g.N), dtype=np.uint64)
    for l in range(nl):
        ct[:, :, l] = int(g.moduli[l]) - 1
    for l in range(g.D):
        pk[:, l] = int(g.moduli[l]) - 1
    v = np.stack([np.full(g.N, 1, dtype=np.int8), np.full(g.N, -1, dtype=np.int8)])
    e0 = np.stack([np.full(g.N, EMAX, dtype=np.int64), np.full(g.N, -EMAX, dtype=np.int64)])
    e1 = -e0
    got = rerandomize(g, ct, pk, v, e0, e1, nl)
    for b in range(B):
        assert np.array_equal(got[b], exact_rerandomize(o, ct[b], pk, v[b], e0[b], e1[b], nl)), (name, b)


@pytest.mark.gpu
def test_rerandomize_call_properties(ctxs):
    """In place = out of place; the strided prefix = the packed prefix; inputs are not written; a batch larger than one
    workspace chunk (MKCKKS_CHUNK = 16); empty calls write nothing; a wrong overlap is refused."""
    from ppqsflhe_amd.binding import MkckksError
    g, o = ctxs("c3")
    rng = np.random.default_rng(77)
    nl_in, B = 11, 2
    ct, pk, v, e0, e1 = wide_inputs(rng, g, nl_in, B)
    out = rerandomize(g, ct, pk, v, e0, e1, nl_in)
    assert np.array_equal(rerandomize(g, ct, pk, v, e0, e1, nl_in, in_place=True), out)
    for b in range(B):
        assert np.array_equal(out[b], exact_rerandomize(o, ct[b], pk, v[b], e0[b], e1[b], nl_in)), b
    d_ct, d_pk = g.to_device(ct), g.to_device(pk)
    d_v, d_e0, d_e1 = g.to_device(v, np.int8), g.to_device(e0, np.int64), g.to_device(e1, np.int64)
    POISON = 0xA5A5A5A5A5A5A5A5
    for nl in (2, 5):
        words, pad = B * 2 * nl * g.N, 2 * g.N
        d_big = g.to_device(np.full(words + pad, POISON, dtype=np.uint64))
        d_out = d_big.view(0, (B, 2, nl, g.N))
        g.rerandomize(d_ct, d_pk, d_v, d_e0, d_e1, d_out, B, nl_in, nl)
        strided = d_out.to_host()
        assert np.all(d_big.to_host()[words:] == POISON)
        assert np.array_equal(strided, rerandomize(g, prefix(ct, nl), pk, v, e0, e1, nl)), nl
        assert np.array_equal(strided, out[:, :, :nl]), nl  # limb by limb the same arithmetic
        d_out.upload(np.full(strided.shape, POISON, dtype=np.uint64))
        g.rerandomize(d_ct, d_pk, d_v, d_e0, d_e1, d_out, 0, nl_in, nl)
        assert np.all(d_out.to_host() == POISON)
    assert np.array_equal(d_ct.to_host(), ct) and np.array_equal(d_pk.to_host(), pk)
    assert np.array_equal(d_e0.to_host(), e0) and np.array_equal(d_v.to_host(), v)
    for call in (lambda: g.rerandomize(d_ct, d_pk, d_v, d_e0, d_e1, d_ct, B, nl_in, 2),
                 lambda: g.rerandomize(d_ct, d_pk, d_v, d_e0, d_e1, d_ct.view(g.N, (g.N,)), B, nl_in, nl_in)):
        with pytest.raises(MkckksError) as ei:
            call()
        assert ei.value.code == -1
    assert np.array_equal(d_ct.to_host(), ct)
    # more ciphertexts than one chunk, on the small ring
    g2, o2 = ctxs("ref")
    B2, nl2 = 19, 3
    ct, pk, v, e0, e1 = wide_inputs(rng, g2, nl2, B2)
    got = rerandomize(g2, ct, pk, v, e0, e1, nl2)
    for b in range(B2):
        assert np.array_equal(got[b], exact_rerandomize(o2, ct[b], pk, v[b], e0[b], e1[b], nl2)), b


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl", [("c3", 12), ("ref", 4)])
@pytest.mark.parametrize("env", [{"MKCKKS_GENERIC_NTT": "1"}, {"MKCKKS_NO_FP64": "1"}, {"MKCKKS_NO_PM": "1"}, {"MKCKKS_CHUNK": "1"}])
def test_rerandomize_under_the_library_switches(ctxs, monkeypatch, env, name, nl):
    """Switches are read once, when a context is created: a fresh context under each must give the same bits."""
    from ppqsflhe_amd import Context
    _, o = ctxs(name)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    a = CONFIGS[name]
    g = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)
    try:
        rng = np.random.default_rng(41 + nl)
        B = 2
        ct, pk, v, e0, e1 = wide_inputs(rng, g, nl, B)
        got = rerandomize(g, ct, pk, v, e0, e1, nl)
        for b in range(B):
            assert np.array_equal(got[b], exact_rerandomize(o, ct[b], pk, v[b], e0[b], e1[b], nl)), (name, env, b)
    finally:
        g.close()


# ---- GPU: the sampler -----------------------------------------------------------------------------------------------

def rotl(v, c):
    return (v << np.uint32(c)) | (v >> np.uint32(32 - c))


def chacha20_blocks(key, counters, n0, n1, n2):
    """RFC 8439 block function, vectorised over blocks: -> uint32[len(counters)][16] (restated from
    tests/test_decode_flood.py)."""
    kw = np.frombuffer(key, dtype="<u4")
    nb = len(counters)
    s = [np.full(nb, w, dtype=np.uint32) for w in (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)]
    s += [np.full(nb, w, dtype=np.uint32) for w in kw]
    s += [np.asarray(counters, dtype=np.uint32), np.asarray(n0, dtype=np.uint32) * np.ones(nb, np.uint32),
          np.full(nb, n1, dtype=np.uint32), np.full(nb, n2, dtype=np.uint32)]
    x = [w.copy() for w in s]

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl(x[d], 16)
        x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl(x[b], 12)
        x[a] += x[b]; x[d] ^= x[a]; x[d] = rotl(x[d], 8)
        x[c] += x[d]; x[b] ^= x[c]; x[b] = rotl(x[b], 7)
    with np.errstate(over="ignore"):
        for _ in range(10):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        return np.stack([x[i] + s[i] for i in range(16)], axis=1)


def stream_normals(key, sid, count):
    """z of elements i < count of stream sid: component i % 2 of pair k = i / 2 (sampler_kernels.hpp: words 2(k%4),
    2(k%4)+1 of block k/4, nonce (block >> 32, sid, 0), Box-Muller on 53-bit uniforms)."""
    pairs = (count + 1) // 2
    k = np.arange(pairs, dtype=np.uint64)
    b = k >> np.uint64(2)
    blk = chacha20_blocks(key, (b & np.uint64(0xFFFFFFFF)).astype(np.uint32), (b >> np.uint64(32)).astype(np.uint32),
                          sid, 0).astype(np.uint64)
    j = (k & np.uint64(3)).astype(np.int64)
    r = np.arange(pairs)
    w0 = blk[r, 4 * j] | (blk[r, 4 * j + 1] << np.uint64(32))
    w1 = blk[r, 4 * j + 2] | (blk[r, 4 * j + 3] << np.uint64(32))
    u1 = ((w0 >> np.uint64(11)) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = (w1 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    rad = np.sqrt(-2.0 * np.log(u1))
    return np.stack([rad * np.cos(2 * np.pi * u2), rad * np.sin(2 * np.pi * u2)], axis=1).reshape(-1)[:count]


def gauss_wide(g, count, sigma, key, sid):
    d = g.empty((count,), np.int64)
    g.sample_gauss_wide(d, count, sigma, key, sid)
    return d.to_host()


@pytest.mark.gpu
def test_sample_gauss_wide_is_the_documented_stream(ctxs):
    """Element i = rint(sigma z_i) of the ChaCha20 + Box-Muller stream; a pure function of (key, sid, i).  Tolerance: 0.5
    for the rounding + sigma |z| 2^-35, the relative tolerance tests/test_decode_flood.py uses for this stream's normals
    (the device's log / sincospi against numpy's)."""
    g, _ = ctxs("c1")
    n, sid = 65536, 5
    key = np.random.default_rng(8).bytes(32)
    for sigma in (2.0 ** 6, 2.0 ** 20, 2.0 ** 30):
        a = gauss_wide(g, n, sigma, key, sid)
        assert np.array_equal(a, gauss_wide(g, n, sigma, key, sid))
        assert np.array_equal(a[:1000], gauss_wide(g, 1000, sigma, key, sid))
        assert np.array_equal(a[:999], gauss_wide(g, 999, sigma, key, sid))  # odd count: the last pair is cut
        assert not np.array_equal(a[:1000], gauss_wide(g, 1000, sigma, key, sid + 1))
        assert not np.array_equal(a[:1000], gauss_wide(g, 1000, sigma, bytes(32), sid))
        z = stream_normals(key, sid, n)
        diff = np.abs(a.astype(np.float64) - sigma * z)
        allowed = 0.5 + sigma * np.abs(z) * 2.0 ** -35
        print(f"sigma 2^{np.log2(sigma):.0f}: max (|got - sigma z| - allowed) = {(diff - allowed).max():.3g}")
        assert np.all(diff <= allowed), (sigma, (diff - allowed).max())
    d = g.empty((8,), np.int64).upload(np.full(8, 123, dtype=np.int64))
    g.sample_gauss_wide(d, 0, 2.0 ** 20, key, sid)
    assert np.all(d.to_host() == 123)


@pytest.mark.gpu
@pytest.mark.parametrize("sigma_bits", [20, 50])
def test_sample_gauss_wide_moments(ctxs, sigma_bits):
    g, _ = ctxs("c1")
    n, sigma, sid = 65536, 2.0 ** sigma_bits, 40
    a = gauss_wide(g, n, sigma, KEY, sid).astype(np.float64)
    b = gauss_wide(g, n, sigma, KEY, sid + 1).astype(np.float64)
    corr = float(np.corrcoef(a, b)[0, 1])
    print(f"sigma 2^{sigma_bits}: mean/sigma {a.mean() / sigma:.4g}, std/sigma {a.std() / sigma:.5f}, max/sigma "
          f"{np.abs(a).max() / sigma:.3f}, corr(sid, sid + 1) {corr:.4g}")
    assert abs(a.mean()) < 5 * sigma / np.sqrt(n)
    assert abs(a.std() / sigma - 1) < 0.02
    assert np.abs(a).max() <= 8.7 * sigma
    assert abs(corr) < 5 / np.sqrt(n)


# ---- GPU: end to end on the device ----------------------------------------------------------------------------------

def device_mask(g, B, sigma, key, stream_base):
    """v, e0, e1 of B ciphertexts: streams stream_base + 3t, + 3t + 1, + 3t + 2 (the hosts' numbering)."""
    N = g.N
    d_v, d_e0, d_e1 = g.empty((B, N), np.int8), g.empty((B, N), np.int64), g.empty((B, N), np.int64)
    for t in range(B):
        g.sample_ternary(d_v.view(t * N, (N,)), N, key, stream_base + 3 * t)
        g.sample_gauss_wide(d_e0.view(t * N, (N,)), N, sigma, key, stream_base + 3 * t + 1)
        g.sample_gauss_wide(d_e1.view(t * N, (N,)), N, sigma, key, stream_base + 3 * t + 2)
    return d_v, d_e0, d_e1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["p14", "p12"])  # the parameters of `ref`, and a deep chain at the ring size of `c1`
def test_hra_back_leg_on_the_device(ctxs, name):
    """aggregate -> rerandomize (device-sampled mask, sigma 2^20) -> reencrypt_fanout / reencrypt_fanout_compact (k = 1) ->
    decrypt -> decode: the mean within the bounds of the CPU chain; two stream bases give ciphertexts that differ in every
    limb of both components and decode alike."""
    g, o = ctxs(name)
    ch = hra_chain(name)
    agg, scale, rk_back, sk0, mean = ch["agg"], ch["scale"], ch["rk_back"], ch["sk0"], ch["mean"]
    pk_tgt = ch["tgt"][1]
    nl, N = agg.shape[1], g.N
    d_agg, d_pk, d_evk, d_sk = g.to_device(agg[None]), g.to_device(pk_tgt), g.to_device(rk_back[None]), g.to_device(sk0)
    key = np.random.default_rng(3).bytes(32)
    outs = []
    for base in (0, 3000):
        d_v, d_e0, d_e1 = device_mask(g, 1, 2.0 ** 20, key, base)
        d_rr = g.empty((1, 2, nl, N))
        g.rerandomize(d_agg, d_pk, d_v, d_e0, d_e1, d_rr, 1, nl, nl)
        rr = d_rr.to_host()
        assert np.array_equal(rr[0], exact_rerandomize(o, agg, pk_tgt, d_v.to_host()[0], d_e0.to_host()[0], d_e1.to_host()[0], nl))
        d_pre = g.empty((1, 2, 2, N))  # the compact leg re-randomises the 2-limb prefix only
        g.rerandomize(d_agg, d_pk, d_v, d_e0, d_e1, d_pre, 1, nl, 2)
        assert np.array_equal(d_pre.to_host(), rr[:, :, :2])
        d_full, d_comp = g.empty((1, 1, 2, nl, N)), g.empty((1, 1, 2, 1, N))
        g.reencrypt_fanout(d_rr, d_evk, d_full, 1, 1, nl)
        g.reencrypt_fanout_compact(d_pre, d_evk, d_comp, 1, 1, 2, 1)
        vals = []
        for d_ct, m, sc in ((d_full, nl, scale), (d_comp, 1, scale / float(o.moduli[1]))):
            d_m, d_vals = g.empty((1, m, N)), g.empty((1, N // 2), dtype=np.float64)
            g.decrypt(d_ct, d_sk, d_m, 1, m)
            g.decode(d_m, d_vals, 1, m, sc)
            vals.append(d_vals.to_host()[0])
            err = np.abs(vals[-1] - mean).max()
            print(f"{name} base {base}, {m} limbs: error 2^{np.log2(err):.2f}")
            assert err < BOUND[name], (name, base, m, err)
        outs.append((rr[0], d_full.to_host()[0, 0], d_comp.to_host()[0, 0], vals))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        for comp in range(2):
            for l in range(a.shape[1]):
                assert not np.array_equal(a[comp, l], b[comp, l]), (comp, l)
    for va, vb in zip(outs[0][3], outs[1][3]):
        assert np.abs(va - vb).max() < 2 * BOUND[name]


# ---- GPU: through the binaries --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hra_round(tmp_path_factory):
    """3 clients (N = 2^14, the ring of tests/test_cli_hosts.py), one plain round with its back leg, as the baseline."""
    import json
    tmp = tmp_path_factory.mktemp("hra")
    n, ext = 3, "mkws"
    cc, vals, args, back_keys = _round_inputs(tmp, n, ext, 4711)

    def back(tag):
        return [x for c in range(n) for x in (back_keys[c], tmp / f"{tag}{c}.{ext}")]

    _ok(run("serverRound", cc, tmp / f"agg.{ext}", *args, "--back", *back("plain")[:-2]))
    mean = [np.mean([np.asarray(vals[c][li][1]) for c in range(n)], axis=0) for li in range(2)]

    def decrypts_to_the_mean(c, path):
        _ok(run("decryptModelWeights", cc, tmp / f"sk{c}", path, str(path) + ".dec.json"))
        dec = json.load(open(str(path) + ".dec.json"))["weights_summary"]
        for li in range(2):
            err = np.abs(np.array(dec[li]["values"]) - mean[li]).max()
            assert err < BOUND["p14"], (c, path, li, err)

    return dict(tmp=tmp, n=n, ext=ext, cc=cc, args=args, back_keys=back_keys, back=back, check=decrypts_to_the_mean)


@pytest.mark.gpu
def test_change_cipher_domain_hra(hra_round):
    h = hra_round
    tmp, ext, cc, tgt = h["tmp"], h["ext"], h["cc"], h["n"] - 1
    agg, rk, pk = tmp / f"agg.{ext}", h["back_keys"][0], tmp / f"pk{tgt}"
    _ok(run("changeCipherDomain", cc, rk, agg, tmp / f"ccd_plain.{ext}"))
    assert _same_bytes(tmp / f"ccd_plain.{ext}", tmp / f"plain0.{ext}")  # without --hra: today's bytes
    outs = []
    for i, extra in enumerate(([], ["--hra-sigma-bits", "24"])):
        out = tmp / f"ccd_hra{i}.{ext}"
        r = _ok(run("changeCipherDomain", cc, rk, agg, out, "--hra", pk, *extra))
        assert f"re-randomised at sigma 2^{extra[1] if extra else 20}" in r.stdout, r.stdout
        h["check"](0, out)
        outs.append(out)
    assert not _same_bytes(outs[0], outs[1]) and not _same_bytes(outs[0], tmp / f"plain0.{ext}")
    assert os.path.getsize(outs[0]) == os.path.getsize(tmp / f"plain0.{ext}")
    comp = []
    for i in range(2):
        out = tmp / f"ccd_hra_k1_{i}.{ext}"
        _ok(run("changeCipherDomain", cc, rk, agg, out, "--limbs", "1", "--hra", pk))
        comp.append(out)
    assert not _same_bytes(comp[0], comp[1])
    h["check"](0, comp[0])
    r = run("changeCipherDomain", cc, rk, agg, tmp / f"bad.{ext}", "--hra", rk)  # a file that is no public key
    assert r.returncode == 1 and "[recrypt] ERROR: Failed to load public key" in r.stderr and not os.path.exists(tmp / f"bad.{ext}")


@pytest.mark.gpu
@pytest.mark.parametrize("limbs", [None, 1])
def test_server_round_hra_back(hra_round, limbs):
    h = hra_round
    tmp, ext, cc, n = h["tmp"], h["ext"], h["cc"], h["n"]
    pk = tmp / f"pk{n - 1}"
    tag = "k1" if limbs else "full"
    for i in range(2):
        back = h["back"](f"hra_{tag}{i}_")
        tail = (["--back", *back, "--back-limbs", "1"] if limbs else ["--back", *back[:-2]]) + ["--hra-back", pk]
        if i:
            tail += ["--hra-sigma-bits", "20"]
        env = {"MKCKKS_BACK_LOOP": "1"} if i else None  # the per-key loop reads the same buffer
        r = _ok(run("serverRound", cc, tmp / f"agg_{tag}{i}.{ext}", *h["args"], *tail, env=env))
        assert re.search(r"\[round\] back leg: .*key\(s\) uploaded" + (", 1 limbs" if limbs else "") +
                         r", re-randomised at sigma 2\^20\n", r.stdout), r.stdout
        assert _same_bytes(tmp / f"agg_{tag}{i}.{ext}", tmp / f"agg.{ext}")  # the aggregate file never changes
    for c in range(n - 1):
        a, b = (tmp / f"hra_{tag}{i}_{c}.{ext}" for i in range(2))
        assert not _same_bytes(a, b), c
        assert os.path.getsize(a) == os.path.getsize(b)
        if not limbs:
            assert not _same_bytes(a, tmp / f"plain{c}.{ext}") and os.path.getsize(a) == os.path.getsize(tmp / f"plain{c}.{ext}")
        h["check"](c, a)
    if limbs:  # the target's own file: no key switch, no mask -- the two runs agree
        a, b = (tmp / f"hra_{tag}{i}_{n - 1}.{ext}" for i in range(2))
        assert _same_bytes(a, b)
        h["check"](n - 1, a)
    r = run("serverRound", cc, tmp / f"x.{ext}", *h["args"], "--back", *h["back"]("x")[:-2], "--hra-back", pk, "--hra-sigma-bits", "57")
    assert r.returncode == 1 and "[round] ERROR: --hra-sigma-bits" in r.stderr and not os.path.exists(tmp / f"x.{ext}")
