"""t-of-n threshold decryption (include/mkckks.h: mkckks_share_key, mkckks_combine_key_shares, mkckks_lagrange_at_zero;
shareKey, combineKeyShares, partialDecrypt --parties): every party Shamir-shares its secret key once per key epoch, party j
keeps sigma_j = sum_i f_i(j), and any set T of at least t parties decrypts with lambda_j^T sigma_j in the place of sk_j.

    share[p][i][c] = sk[i][c] + sum_{k=1}^{t-1} r_k[i][c] (p + 1)^k        mod q_i,   r_k = sample_uniform(key, stream + k - 1)
    out[i][c]      = sum_{j<m} w[j][i] in[j][i][c]                          mod q_i
    lambda_j^T     = prod_{m in T, m != j} m (m - j)^-1                     mod q_l

The reference of every residue is exact integer arithmetic in this file (Python ints in numpy object arrays, pow(x, -1, q)
for inverses); comparisons are word for word.  The only tolerances are the two noise bounds of
tests/test_threshold_decrypt.py's docstring with n := |T| (the Lagrange factor multiplies the key share, not the error),
and BOUND["p14"] of tests/test_compact_downlink.py for the decoded mean of the command-line round."""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests.test_cli_hosts import BIN, _small_cc, _weights, run
from tests.test_compact_downlink import BOUND, _ok, _same_bytes
from tests.test_gpu_parity import CONFIGS, rand_polys
from tests.test_threshold_decrypt import exact_share, noise_sd, sum_mod, threshold_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppqsflhe_amd", "host")
SYMBOLS = ("mkckks_share_key", "mkckks_combine_key_shares", "mkckks_lagrange_at_zero")
KEY = bytes(range(7, 39))
INVALID, NODEVICE = -1, -2


# ---- references: Python ints ---------------------------------------------------------------------------------------------

def lagrange(T, j, q):
    """lambda_j^T at 0 mod q."""
    lam = 1
    for m in T:
        if m != j:
            lam = lam * m * pow(m - j, -1, q) % q
    return lam


def obj(a):
    return np.asarray(a).astype(object)


def shamir_ref(sk, rs, moduli, n):
    """shares [n][nl][W] of sk [nl][W] with coefficient polynomials rs [t - 1][nl][W] (r_1 first): Horner in Python ints."""
    nl = sk.shape[0]
    out = np.empty((n,) + sk.shape, dtype=np.uint64)
    for i in range(nl):
        q = int(moduli[i])
        s, r = obj(sk[i]), [obj(x[i]) for x in rs]
        for p in range(n):
            acc = 0
            for rk in reversed(r):
                acc = (acc + rk) * (p + 1) % q
            out[p, i] = ((acc + s) % q).astype(np.uint64)
    return out


def wsum_ref(inp, w, moduli):
    """sum_j w[j][i] inp[j][i] mod q_i in Python ints; inp [m][nl][W], w [m][nl]."""
    m, nl = inp.shape[:2]
    out = np.empty(inp.shape[1:], dtype=np.uint64)
    for i in range(nl):
        q = int(moduli[i])
        acc = 0
        for j in range(m):
            acc = acc + obj(inp[j, i]) * int(w[j][i])
        out[i] = (acc % q).astype(np.uint64)
    return out


def scale_ref(poly, lam, moduli):
    """lam[i] * poly[i] mod q_i over the limbs lam covers; the further limbs (P) stay zero."""
    out = np.zeros_like(poly)
    for i, l in enumerate(lam):
        out[i] = (obj(poly[i]) * int(l) % int(moduli[i])).astype(np.uint64)
    return out


# ---- CPU: surface, Lagrange coefficients, argument checks ---------------------------------------------------------------

def test_key_sharing_symbols_are_declared_bound_and_exported():
    from ppqsflhe_amd import Context, binding
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mkckks.h")).read(), flags=re.S)
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert sym in binding.SYMBOLS
        assert hasattr(binding.load_library(), sym)
    assert re.search(r"#define\s+MKCKKS_MAX_PARTIES\s+64\b", hdr)
    for meth in ("share_key", "combine_key_shares", "lagrange_at_zero"):
        assert callable(getattr(Context, meth, None)), meth
    assert "t-of-n is out of scope" not in open(os.path.join(ROOT, "include", "mkckks.h")).read()


SETS = [(1,), (1, 2), (1, 3), (2, 3), (1, 2, 3), (2, 5, 64), tuple(range(1, 10))]


@pytest.mark.parametrize("params", [(14, 2, 40, 60, 2), (12, 10, 50, 60, 3)])
def test_lagrange_at_zero_on_a_host_only_context(params):
    from ppqsflhe_amd import Context
    from ppqsflhe_amd.binding import MkckksError
    c = Context(params[0], params[1], params[2], params[3], dnum=params[4], device=-1)
    try:
        L, moduli = c.L, [int(q) for q in c.moduli[:c.L]]
        for T in SETS:
            got = c.lagrange_at_zero(T)
            assert got.shape == (len(T), L) and got.dtype == np.uint64
            for a, j in enumerate(T):
                for l, q in enumerate(moduli):
                    assert int(got[a, l]) == lagrange(T, j, q), (T, j, l)
        # sum_j lambda_j F(j) = F(0) for a random polynomial of degree t - 1, |T| = t and t + 1
        rng = np.random.default_rng(5)
        for t, pool in ((1, (4, 9)), (2, (1, 3, 64)), (3, (2, 5, 7, 64)), (9, tuple(range(3, 13)))):
            for T in (pool[:t], pool[:t + 1]):
                lam = c.lagrange_at_zero(T)
                for l, q in enumerate(moduli):
                    coef = [int(rng.integers(0, q)) for _ in range(t)]
                    F = lambda x: sum(cf * x ** k for k, cf in enumerate(coef)) % q
                    assert sum(int(lam[a, l]) * F(j) for a, j in enumerate(T)) % q == F(0), (t, T, l)
        for bad in ((0,), (1, 0), (65,), (1, 65), (2, 2), (1, 2, 1), ()):
            with pytest.raises(MkckksError) as ei:
                c.lagrange_at_zero(bad)
            assert ei.value.code == INVALID, bad
        out = np.zeros(L, dtype=np.uint64)
        one = np.array([1], dtype=np.uint32)
        assert c._L.mkckks_lagrange_at_zero(c._h, None, 1, out.ctypes.data) == INVALID
        assert c._L.mkckks_lagrange_at_zero(c._h, one.ctypes.data, 1, None) == INVALID
    finally:
        c.close()


def test_key_sharing_argument_checks_on_a_host_only_context():
    """Every refusal is MKCKKS_E_INVALID; what passes the checks ends in MKCKKS_E_NODEVICE.  Pointers are never dereferenced."""
    from ppqsflhe_amd import Context
    from ppqsflhe_amd.binding import MkckksError
    c = Context(12, 2, 40, 60, dnum=2, device=-1)
    sh, cb = c._L.mkckks_share_key, c._L.mkckks_combine_key_shares
    far, W = 1 << 40, 8 * c.N
    try:
        L = c.L
        # share_key(ctx, sk, shares, nl, n_parties, threshold, key, stream_id)
        assert sh(c._h, 8, far, L, 3, 2, KEY, 0) == NODEVICE
        assert sh(c._h, 8, far, 1, 1, 1, KEY, 0) == NODEVICE
        assert sh(c._h, 8, far, L, 64, 64, KEY, 2 ** 32 - 64) == NODEVICE
        assert sh(c._h, 8, far, L, 3, 1, KEY, 2 ** 32 - 1) == NODEVICE          # threshold 1: stream_id + 0
        assert sh(c._h, None, far, L, 3, 2, KEY, 0) == INVALID
        assert sh(c._h, 8, None, L, 3, 2, KEY, 0) == INVALID
        assert sh(c._h, 8, far, L, 3, 2, None, 0) == INVALID
        assert sh(c._h, 8, far, 0, 3, 2, KEY, 0) == INVALID
        assert sh(c._h, 8, far, L + 1, 3, 2, KEY, 0) == INVALID
        assert sh(c._h, 8, far, L, 3, 0, KEY, 0) == INVALID                     # threshold 0
        assert sh(c._h, 8, far, L, 3, 4, KEY, 0) == INVALID                     # threshold > n_parties
        assert sh(c._h, 8, far, L, 0, 0, KEY, 0) == INVALID
        assert sh(c._h, 8, far, L, 65, 2, KEY, 0) == INVALID                    # n_parties > MKCKKS_MAX_PARTIES
        assert sh(c._h, 8, far, L, 3, 2, KEY, 2 ** 32 - 1) == INVALID           # stream_id + threshold - 1 wraps
        assert sh(c._h, 8, far, L, 64, 64, KEY, 2 ** 32 - 63) == INVALID
        assert sh(c._h, 8, 8, L, 3, 2, KEY, 0) == INVALID                       # shares over the key
        assert sh(c._h, 8, 8 + L * W - 8, L, 3, 2, KEY, 0) == INVALID           # shares starting in the key's last limb read
        assert sh(c._h, far + W, far, L, 3, 2, KEY, 0) == INVALID               # key starting inside the shares
        assert sh(c._h, 8, 8 + L * W, L, 3, 2, KEY, 0) == NODEVICE              # shares right behind the limbs read
        assert sh(c._h, far + 3 * L * W, far, L, 3, 2, KEY, 0) == NODEVICE      # key right behind the shares
        # combine_key_shares(ctx, in, w, out, m, nl)
        ones = np.ones((4, L), dtype=np.uint64)
        wp = ones.ctypes.data
        assert cb(c._h, 8, wp, far, 4, L) == NODEVICE
        assert cb(c._h, 8, wp, 8, 4, L) == NODEVICE                             # out = in[0]
        assert cb(c._h, 8, wp, 8 + 4 * L * W, 4, L) == NODEVICE                 # out right behind the inputs
        assert cb(c._h, 8, wp, far, 1, 1) == NODEVICE
        assert cb(c._h, None, wp, far, 4, L) == INVALID
        assert cb(c._h, 8, None, far, 4, L) == INVALID
        assert cb(c._h, 8, wp, None, 4, L) == INVALID
        assert cb(c._h, 8, wp, far, 0, L) == INVALID                            # m == 0
        assert cb(c._h, 8, wp, far, 4, 0) == INVALID
        assert cb(c._h, 8, wp, far, 4, L + 1) == INVALID
        assert cb(c._h, 8, wp, 8 + L * W, 4, L) == INVALID                      # out = in[1]
        assert cb(c._h, 8, wp, 8 + W, 4, L) == INVALID                          # out starting inside in[0]
        assert cb(c._h, far + W, wp, far, 4, L) == INVALID                      # inputs starting inside out
        for j, i in ((0, 0), (3, L - 1)):                                       # a weight at its modulus, and above
            for v in (int(c.moduli[i]), 2 ** 64 - 1):
                w = ones.copy()
                w[j, i] = v
                assert cb(c._h, 8, w.ctypes.data, far, 4, L) == INVALID, (j, i, v)
        w = ones.copy()
        w[:] = c.moduli[:L] - np.uint64(1)
        assert cb(c._h, 8, w.ctypes.data, far, 4, L) == NODEVICE                # q - 1 is a weight
        for call, code in ((lambda: c.share_key(8, far, L, 3, 2, KEY), NODEVICE),
                           (lambda: c.combine_key_shares(8, ones, far, 4, L), NODEVICE),
                           (lambda: c.share_key(8, far, L, 3, 4, KEY), INVALID),
                           (lambda: c.combine_key_shares(8, ones[:0], far, 0, L), INVALID)):
            with pytest.raises(MkckksError) as ei:
                call()
            assert ei.value.code == code
    finally:
        c.close()


# ---- CPU: the protocol on the oracle alone: the reference of everything below -------------------------------------------

def test_oracle_t_of_n_protocol():
    """3 parties, 2-of-3: each sk_i shared in Python ints, sigma_j = sum_i f_i(j); for every T of at least 2 parties the
    zero-error shares made with lambda_j sigma_j sum to the decryption under sum sk_i, word for word; one party does not."""
    ch = threshold_chain("p14")
    o, agg, sks, m0 = ch["o"], ch["agg"], ch["sks"], ch["m0"]
    N, L, nl = o.N, o.L, agg.shape[1]
    moduli = [int(q) for q in o.moduli[:L]]
    rng = np.random.default_rng(91)
    n, t = 3, 2
    sigma = []
    dealt = []
    for i in range(n):
        r1 = np.stack([rng.integers(0, q, size=N, dtype=np.uint64) for q in moduli])
        dealt.append(shamir_ref(sks[i][:L], [r1], moduli, n))
    for j in range(n):
        s = np.zeros((o.D, N), dtype=np.uint64)
        s[:L] = wsum_ref(np.stack([dealt[i][j] for i in range(n)]), np.ones((n, L), dtype=np.uint64), moduli)
        sigma.append(s)
    zero = np.zeros(N, dtype=np.int64)

    def fused(T):
        parts = []
        for j in T:
            key = scale_ref(sigma[j - 1], [lagrange(T, j, q) for q in moduli], moduli)
            parts.append(exact_share(o, agg, key, zero, nl, j == min(T)))
        return sum_mod(o, parts)

    for T in ((1, 2), (1, 3), (2, 3), (1, 2, 3)):
        assert np.array_equal(fused(T), m0), T
    for T in ((1,), (2,), (3,)):  # below the threshold
        assert not np.array_equal(fused(T), m0), T
    for j in range(n):  # a combined share is not the party's key, and not the joint key
        assert not np.array_equal(sigma[j][:L], sks[j][:L]) and not np.array_equal(sigma[j][:L], ch["sk_sum"][:L])


# ---- CPU: the stand-alone selftest and the hosts' usage lines -----------------------------------------------------------

def test_keyshare_selftest_plain_and_under_asan_ubsan():
    """The key-share parser on truncated, oversized, wrong-kind, wrong-ring, out-of-range and non-canonical blobs, and
    mkckks_lagrange_at_zero on a host-only context against 128-bit arithmetic: a stand-alone program, plain and under
    AddressSanitizer + UBSan.  A sanitizer report aborts the process (non-zero exit)."""
    r = subprocess.run(["make", "-C", HOST, "-s", "build/keyshare_selftest", "keyshare-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    for exe in (os.path.join(BIN, "keyshare_selftest"), os.path.join(BIN, "asan", "keyshare_selftest")):
        r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, (exe, r.stdout[-2000:] + r.stderr[-2000:])
        assert "ok keyshare selftest" in r.stdout and "FAIL" not in r.stderr, exe
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, exe
        for case in ("truncated trailer", "truncated payload", "oversized by one byte", "share blob of kind 6", "wrong ring",
                     "threshold 0", "threshold > n_parties", "to_party 0", "to_party > n_parties", "non-canonical word",
                     "lagrange {1}", "lagrange {1,2}", "lagrange {2,5,64}", "lagrange duplicates refused"):
            assert f"ok {case}" in r.stdout, (exe, case)


@pytest.mark.parametrize("prog,usage,argvs", [
    ("shareKey", "<cc_path> <privkey_path> <n_parties> <threshold> <party_index> <out_prefix>",
     [(), ("cc", "sk", "3", "2", "1"), ("cc", "sk", "3", "2", "1", "out", "extra"), ("cc", "sk", "x", "2", "1", "out")]),
    ("combineKeyShares", "<cc_path> <out> <share_1> [<share_2> ...]", [(), ("cc",), ("cc", "out")]),
    ("partialDecrypt", "<cc_path> <privkey_path> <input_encfile> <share_out> [--lead] [--smudge-bits <s>] [--parties i,j,...]",
     [(), ("cc", "sk", "in"), ("cc", "sk", "in", "out", "--parties"), ("cc", "sk", "in", "out", "--parties", "1,2", "--parties", "1,2")]),
])
def test_key_sharing_usage_lines(tmp_path, prog, usage, argvs):
    for argv in argvs:
        r = run(prog, *argv)
        assert r.returncode == 1 and "Usage:" in r.stderr and usage in r.stderr, (prog, argv, r.stdout + r.stderr)
    assert not os.listdir(tmp_path)


# ---- GPU ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctxs():
    from ppqsflhe_amd import Context
    cache = {}

    def get(name):
        if name not in cache:
            a = CONFIGS[name]
            cache[name] = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)
        return cache[name]

    yield get
    for g in cache.values():
        g.close()


def rand_sk(rng, g):
    return rand_polys(rng, g, list(range(g.D)), 1)[0]


def device_share_key(g, sk, nl, n, t, key=KEY, sid=0):
    d_shares = g.empty((n, nl, g.N))
    g.share_key(g.to_device(sk), d_shares, nl, n, t, key, sid)
    return d_shares.to_host()


def device_coefficients(g, nl, t, key=KEY, sid=0):
    """r_1 .. r_{t-1} by their definition: sample_uniform(1 poly, nl, Q only) of streams sid .. sid + t - 2."""
    rs = []
    for k in range(1, t):
        d = g.empty((1, nl, g.N))
        g.sample_uniform(d, 1, nl, False, key, sid + k - 1)
        rs.append(d.to_host()[0])
    return rs


NT = [(1, 1), (3, 1), (3, 2), (5, 3), (9, 9), (17, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,t", NT)
@pytest.mark.parametrize("name", ["tiny", "n11", "c1", "ref"])
def test_share_key_matches_the_definition(ctxs, name, n, t):
    g = ctxs(name)
    rng = np.random.default_rng(300 + 10 * n + t)
    sk = rand_sk(rng, g)
    sid = 2 ** 32 - t if (n, t) == (5, 3) else 40 * n  # once at the last stream ids that fit
    for nl in (g.L, 1):
        rs = device_coefficients(g, nl, t, sid=sid)
        got = device_share_key(g, sk, nl, n, t, sid=sid)
        assert np.array_equal(got, shamir_ref(sk[:nl], rs, g.moduli, n)), (name, n, t, nl)
        if t == 1:
            assert all(np.array_equal(got[p], sk[:nl]) for p in range(n))  # the degenerate sharing


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "ref"])
def test_share_key_party_grouping_does_not_matter(ctxs, name):
    """Share p is the same whether 3 or 17 parties are dealt (one party group or three); inputs and a poisoned tail stay."""
    g = ctxs(name)
    rng = np.random.default_rng(17)
    sk, nl, N = rand_sk(rng, g), g.L, g.N
    POISON = 0xA5A5A5A5A5A5A5A5
    for t in (2, 3):
        few, many = device_share_key(g, sk, nl, 3, t), device_share_key(g, sk, nl, 17, t)
        assert np.array_equal(few, many[:3]), (name, t)
        assert not np.array_equal(device_share_key(g, sk, nl, 3, t, sid=1), few)
        assert not np.array_equal(device_share_key(g, sk, nl, 3, t, key=bytes(32)), few)
    d_sk = g.to_device(sk)
    d_big = g.to_device(np.full(9 * nl * N + 2 * N, POISON, dtype=np.uint64))
    g.share_key(d_sk, d_big.view(0, (9, nl, N)), nl, 9, 3, KEY, 0)
    out = d_big.to_host()
    assert np.all(out[9 * nl * N:] == POISON) and np.array_equal(out[:9 * nl * N].reshape(9, nl, N), device_share_key(g, sk, nl, 9, 3))
    assert np.array_equal(d_sk.to_host(), sk)


def composition(g, sk, nl, n, t, key=KEY, sid=0):
    """The sharing from the public entry points: t - 1 sample_uniform polynomials in HBM, then per party one
    combine_key_shares of (sk, r_1 .. r_{t-1}) with weights (p + 1)^k."""
    N = g.N
    d_ops = g.empty((t, nl, N))
    d_ops.view(0, (nl, N)).upload(sk[:nl])
    for k in range(1, t):
        g.sample_uniform(d_ops.view(k * nl * N, (1, nl, N)), 1, nl, False, key, sid + k - 1)
    d_out = g.empty((n, nl, N))
    for p in range(n):
        w = [[pow(p + 1, k, int(g.moduli[i])) for i in range(nl)] for k in range(t)]
        g.combine_key_shares(d_ops, w, d_out.view(p * nl * N, (nl, N)), t, nl)
    return d_out.to_host(), d_ops.to_host()


@pytest.mark.gpu
def test_share_key_at_the_production_ring(ctxs):
    """"c3" (N = 2^16, nl = 12, fp64-class and 60-bit limbs), n = 3, t = 2: all words against the device composition, 4096
    sampled positions per limb against Python ints."""
    g = ctxs("c3")
    rng = np.random.default_rng(8)
    nl, n, t = 12, 3, 2
    assert g.L == nl
    sk = rand_sk(rng, g)
    got = device_share_key(g, sk, nl, n, t)
    comp, ops = composition(g, sk, nl, n, t)
    assert np.array_equal(got, comp)
    pos = np.sort(rng.choice(g.N, size=4096, replace=False))
    pos[:2], pos[-2:] = (0, 1), (g.N - 2, g.N - 1)
    ref = shamir_ref(sk[:nl][:, pos], [ops[1][:, pos]], g.moduli, n)
    assert np.array_equal(got[:, :, pos], ref)


def device_combine(g, inp, w, in_place=False):
    m, nl = inp.shape[:2]
    d_in = g.to_device(inp)
    d_out = d_in.view(0, (nl, g.N)) if in_place else g.empty((nl, g.N))
    g.combine_key_shares(d_in, w, d_out, m, nl)
    return d_out.to_host(), d_in.to_host()


def rand_weights(rng, g, m, nl):
    return np.stack([rng.integers(0, int(g.moduli[i]), size=m, dtype=np.uint64) for i in range(nl)], axis=1)


@pytest.mark.gpu
@pytest.mark.parametrize("name,m", [("tiny", 1), ("tiny", 4), ("tiny", 5), ("tiny", 9), ("tiny", 64), ("ref", 5), ("c5s", 17)])
def test_combine_key_shares_matches_python_ints(ctxs, name, m):
    """Random inputs and weights; m = 17 at "c5s" (L = 20) crosses both chunk limits of one launch (16 inputs, 16 limbs)."""
    g = ctxs(name)
    rng = np.random.default_rng(50 + m)
    for nl in (g.L, 1):
        inp = rand_polys(rng, g, list(range(nl)), m)
        w = rand_weights(rng, g, m, nl)
        exp = wsum_ref(inp, w, g.moduli)
        out, after = device_combine(g, inp, w)
        assert np.array_equal(out, exp) and np.array_equal(after, inp), (name, m, nl)
        out, after = device_combine(g, inp, w, in_place=True)  # d_out == d_in
        assert np.array_equal(out, exp) and np.array_equal(after[1:], inp[1:]), (name, m, nl)
        ones = np.ones((m, nl), dtype=np.uint64)
        assert np.array_equal(device_combine(g, inp, ones)[0], wsum_ref(inp, ones, g.moduli))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "c5s"])
def test_combine_key_shares_extreme_operands(ctxs, name):
    """Every input word q - 1 and every weight q - 1, m = 9: the sum is 9 mod q."""
    g = ctxs(name)
    m, nl = 9, g.L
    qm1 = (g.moduli[:nl] - np.uint64(1)).astype(np.uint64)
    inp = np.broadcast_to(qm1[None, :, None], (m, nl, g.N)).copy()
    w = np.broadcast_to(qm1[None, :], (m, nl)).copy()
    out, _ = device_combine(g, inp, w)
    assert np.array_equal(out, wsum_ref(inp, w, g.moduli)) and np.all(out == 9)


@pytest.mark.gpu
def test_key_sharing_refusals_on_the_device(ctxs):
    """A refused call writes nothing."""
    from ppqsflhe_amd.binding import MkckksError
    g = ctxs("tiny")
    nl, N = g.L, g.N
    d_in = g.to_device(np.full((4, nl, N), 7, dtype=np.uint64))
    d_out = g.to_device(np.full((4, nl, N), 9, dtype=np.uint64))
    ones = np.ones((4, nl), dtype=np.uint64)
    big = ones.copy()
    big[2, nl - 1] = g.moduli[nl - 1]
    for call in (lambda: g.combine_key_shares(d_in, big, d_out, 4, nl),
                 lambda: g.combine_key_shares(d_in, ones[:0], d_out, 0, nl),
                 lambda: g.combine_key_shares(d_in, ones, d_in.view(nl * N, (nl, N)), 4, nl),
                 lambda: g.combine_key_shares(d_in, ones, d_in.view(N, (N,)), 4, nl),
                 lambda: g.share_key(d_in, d_out, nl, 4, 5, KEY),
                 lambda: g.share_key(d_in, d_out, nl, 4, 0, KEY),
                 lambda: g.share_key(d_in, d_out, nl + 1, 1, 1, KEY),
                 lambda: g.share_key(d_in, d_out, nl, 4, 2, KEY, 2 ** 32 - 1),
                 lambda: g.share_key(d_in, d_in, nl, 4, 2, KEY),
                 lambda: g.share_key(d_in, d_in.view(N // 2, (N,)), 1, 1, 1, KEY)):
        with pytest.raises(MkckksError) as ei:
            call()
        assert ei.value.code == INVALID
    assert np.all(d_in.to_host() == 7) and np.all(d_out.to_host() == 9)


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{"MKCKKS_NO_FP64": "1"}, {"MKCKKS_NO_PM": "1"}])
def test_key_sharing_under_the_library_switches(ctxs, monkeypatch, env):
    """Switches are read once, when a context is created: a fresh context under each gives the bits of the default one and
    of the definition ("tiny": share_key n = 5, t = 3; combine_key_shares m = 5)."""
    from ppqsflhe_amd import Context
    g0 = ctxs("tiny")
    rng = np.random.default_rng(29)
    sk, nl = rand_sk(rng, g0), g0.L
    inp, w = rand_polys(rng, g0, list(range(nl)), 5), rand_weights(rng, g0, 5, nl)
    base_shares, base_sum = device_share_key(g0, sk, nl, 5, 3), device_combine(g0, inp, w)[0]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    a = CONFIGS["tiny"]
    g = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)
    try:
        assert np.array_equal(g.moduli, g0.moduli)
        got = device_share_key(g, sk, nl, 5, 3)
        assert np.array_equal(got, base_shares), env
        assert np.array_equal(got, shamir_ref(sk[:nl], device_coefficients(g, nl, 3), g.moduli, 5)), env
        got = device_combine(g, inp, w)[0]
        assert np.array_equal(got, base_sum) and np.array_equal(got, wsum_ref(inp, w, g.moduli)), env
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ref", "c1"])
def test_t_of_n_decryption_on_the_device(ctxs, name):
    """n = 5, t = 3, everything on the device: keygen / keygen_join, share_key per party, sigma_j by combine_key_shares with
    weights 1, a batch encrypted under the joint key.  With zero errors every T of at least 3 parties fuses to
    decrypt_batch(ct, sum sk_i) word for word and 2 parties do not; with smudging at sigma = 2^20 and |T| = 3 the decoded
    error obeys the two noise bounds with n := 3."""
    from oracle.oracle import sample_gauss, sample_ternary
    g = ctxs(name)
    rng = np.random.default_rng(404)
    N, L, D, n, t, B = g.N, g.L, g.D, 5, 3, 2
    a = rand_sk(rng, g)
    d_pk, sks = None, []
    for p in range(n):
        d_new, d_sk = g.empty((2, D, N)), g.empty((D, N))
        d_s, d_e = g.to_device(sample_ternary(rng, N)), g.to_device(sample_gauss(rng, N))
        if p == 0:
            g.keygen(d_s, g.to_device(a), d_e, d_new, d_sk)
        else:
            g.keygen_join(d_pk, d_s, d_e, d_new, d_sk)
        d_pk = d_new
        sks.append(d_sk)
    # sigma_j = sum_i f_i(j): dealt[i] u64[n][L][N], regrouped by receiver
    d_dealt = g.empty((n, n, L, N))
    for i in range(n):
        g.share_key(sks[i], d_dealt.view(i * n * L * N, (n, L, N)), L, n, t, rng.bytes(32), 0)
    dealt = d_dealt.to_host()
    ones = np.ones((n, L), dtype=np.uint64)
    sigma = []
    for j in range(n):
        d_in = g.to_device(np.ascontiguousarray(dealt[:, j]))
        g.combine_key_shares(d_in, ones, d_in, n, L)
        sigma.append(d_in.view(0, (L, N)))
    # the batch under the joint key, and its decryption under sum sk_i (fuse_shares over the five sk)
    vals = rng.uniform(-0.3, 0.3, size=(B, N // 2))
    scale = g.sf_big(0)
    d_pt, d_ct = g.empty((B, L, N)), g.empty((B, 2, L, N))
    g.encode(g.to_device(vals), d_pt, B, L, scale)
    g.encrypt(d_pk, d_pt, g.to_device(np.stack([sample_ternary(rng, N) for _ in range(B)])),
              g.to_device(np.stack([sample_gauss(rng, N) for _ in range(B)])),
              g.to_device(np.stack([sample_gauss(rng, N) for _ in range(B)])), d_ct, B, L)
    d_sum = g.empty((1, L, N))
    g.fuse_shares(g.to_device(np.stack([s.to_host()[:L] for s in sks])[:, None]), d_sum, n, 1, L)
    d_m = g.empty((B, L, N))
    g.decrypt(d_ct, d_sum, d_m, B, L)
    m0 = d_m.to_host()
    d_vals = g.empty((B, N // 2), dtype=np.float64)
    g.decode(d_m, d_vals, B, L, scale)
    err0 = np.abs(d_vals.to_host() - vals).max()
    assert err0 < 2.0 ** -20, (name, err0)
    zeros = g.to_device(np.zeros((B, N), dtype=np.int64))

    def round_of(T, errors):
        lam = g.lagrange_at_zero(T)
        d_shares = g.empty((len(T), B, L, N))
        for a_, j in enumerate(T):
            d_key = g.empty((L, N))
            g.combine_key_shares(sigma[j - 1], lam[a_:a_ + 1], d_key, 1, L)  # lambda_j sigma_j, u64[L][N]
            g.partial_decrypt(d_ct, d_key, errors[a_], d_shares.view(a_ * B * L * N, (B, L, N)), B, L, L, j == min(T))
        d_out = g.empty((B, L, N))
        g.fuse_shares(d_shares, d_out, len(T), B, L)
        return d_out.to_host()

    for T in ((1, 2, 3), (1, 3, 5), (2, 4, 5), (1, 2, 3, 4, 5)):
        assert np.array_equal(round_of(T, [zeros] * len(T)), m0), (name, T)
    assert not np.array_equal(round_of((1, 2), [zeros] * 2), m0), name
    # smudging: fused - m0 is sum e mod q; decode is linear, so its decode is the decoded error (the method of
    # tests/test_threshold_decrypt.py: the difference of two decodes near 0.3 cannot resolve it at this scale)
    T, sigma_e = (1, 3, 5), 2.0 ** 20
    key = rng.bytes(32)
    errors = []
    for a_ in range(len(T)):
        d_e = g.empty((B, N), np.int64)
        for b in range(B):
            g.sample_gauss_wide(d_e.view(b * N, (N,)), N, sigma_e, key, a_ * B + b)
        errors.append(d_e)
    fused = round_of(T, errors)
    diff = np.empty_like(fused)
    for i in range(L):
        q = g.moduli[i]
        diff[:, i] = (fused[:, i] + (q - m0[:, i])) % q
    e_sum = np.sum([e.to_host() for e in errors], axis=0, dtype=np.int64)
    for i in range(L):
        assert np.array_equal(diff[:, i], np.mod(e_sum, np.int64(int(g.moduli[i]))).astype(np.uint64)), (name, i)
    g.decode(g.to_device(diff), d_vals, B, L, scale)
    noise = d_vals.to_host()
    sd = noise_sd(sigma_e, len(T), N, scale)
    ratio = noise.std() / sd
    err = np.abs((g_dec0(g, m0, scale, B, L) - vals) + noise).max()
    print(f"{name}: sd 2^{np.log2(sd):.2f}, measured / rule {ratio:.4f}, largest / sd {np.abs(noise).max() / sd:.2f}, "
          f"error 2^{np.log2(err):.2f}, zero-smudging error 2^{np.log2(err0):.2f}")
    assert 0.9 < ratio < 1.1, (name, ratio)
    assert err < err0 + 6 * sd, (name, err, err0, sd)


def g_dec0(g, m0, scale, B, L):
    d_vals = g.empty((B, g.N // 2), dtype=np.float64)
    g.decode(g.to_device(m0), d_vals, B, L, scale)
    return d_vals.to_host()


# ---- GPU: through the binaries ------------------------------------------------------------------------------------------

KS_HDR = "<4sIIIIIIIdII4I"  # hostlib.hpp BlobHeader + keyshare.hpp trailer: n_parties, threshold, from_party, to_party
KIND_KEYSHARE = 7


def read_keyshare(path):
    raw = open(path, "rb").read()
    h = struct.unpack(KS_HDR, raw[:64])
    return h, np.frombuffer(raw[64:], dtype=np.uint64)


@pytest.mark.gpu
def test_t_of_n_round_through_the_binaries(tmp_path):
    """N = 2^14, MKWS, 3 parties, t = 2.  Key chain keyGen / keyGen --join x 2; shareKey x 3; combineKeyShares x 3; the
    aggregate of tests/test_threshold_decrypt.py's round; parties 1 and 3 alone, then 2 and 3 alone, open it.  A plain-key
    partialDecrypt round logs and fuses as before: its log lines, file sizes and decoded mean are checked, NOT byte identity
    with earlier builds (the smudging key is drawn from the OS and no test uses a seeded build).  Every misuse exits 1 and writes nothing."""
    from tests.test_seeded_ciphertexts import read_mkws
    tmp, ext, N, n, t = tmp_path, "mkws", 1 << 14, 3, 2
    cc = _small_cc(tmp)
    rng = np.random.default_rng(909)
    vals = [[("dense", rng.uniform(-0.3, 0.3, 8192 + 300)), ("bias", rng.uniform(-0.3, 0.3, 4))] for _ in range(3)]
    mean = [np.mean([np.asarray(vals[c][li][1]) for c in range(3)], axis=0) for li in range(2)]
    _ok(run("keyGen", cc, tmp / "pk1", tmp / "sk1"))
    for p in (2, 3):
        _ok(run("keyGen", cc, tmp / f"pk{p}", tmp / f"sk{p}", "--join", tmp / f"pk{p - 1}"))
    _ok(run("keyGen", cc, tmp / "pkx", tmp / "skx"))
    joint = tmp / "pk3"
    for c, key in ((0, joint), (1, joint), (2, tmp / "pkx")):
        _ok(run("encryptModelWeights", cc, key, _weights(tmp, f"w{c}.json", vals[c]), tmp / f"enc{c}.{ext}"))
    _ok(run("REkeyGen", cc, tmp / "skx", joint, tmp / "rkx"))
    agg = tmp / f"agg.{ext}"
    _ok(run("serverRound", cc, agg, "-", tmp / f"enc0.{ext}", "-", tmp / f"enc1.{ext}", tmp / "rkx", tmp / f"enc2.{ext}"))
    # once per key epoch: every party deals, every party combines what it received
    for i in (1, 2, 3):
        r = _ok(run("shareKey", cc, tmp / f"sk{i}", n, t, i, tmp / f"ks{i}"))
        assert f"[shareKey] {n} key share(s) of party {i}, threshold {t}\n" in r.stdout, r.stdout
        for j in (1, 2, 3):
            h, data = read_keyshare(tmp / f"ks{i}.{j}")
            assert h[2] == KIND_KEYSHARE and h[3] == N and h[5] == 1 and h[6:11] == (0, 0, 0.0, 0, 0) and h[11:] == (n, t, i, j)
            assert data.size == h[4] * N
    L = read_keyshare(tmp / "ks1.1")[0][4]
    for j in (1, 2, 3):
        r = _ok(run("combineKeyShares", cc, tmp / f"sigma{j}", *(tmp / f"ks{i}.{j}" for i in (2, 3, 1))))
        assert f"[combine] {n} key share(s) for party {j} loaded\n" in r.stdout, r.stdout
        h, data = read_keyshare(tmp / f"sigma{j}")
        assert h[2] == KIND_KEYSHARE and h[4] == L and h[11:] == (n, t, 0, j)
        parts = [read_keyshare(tmp / f"ks{i}.{j}")[1].reshape(L, N) for i in (1, 2, 3)]
        moduli = [int(q) for q in json.load(open(cc))["mkckks_cc"]["moduli"]]
        assert np.array_equal(data.reshape(L, N), wsum_ref(np.stack(parts), np.ones((3, L), dtype=np.uint64), moduli))
    # a share file of the same dealer differs between runs (fresh key), and between receivers
    _ok(run("shareKey", cc, tmp / "sk1", n, t, 1, tmp / "again"))
    assert not _same_bytes(tmp / "again.2", tmp / "ks1.2") and not _same_bytes(tmp / "ks1.1", tmp / "ks1.2")

    def fused_error(tag, T):
        for j in T:
            extra = ["--lead"] if j == min(T) else []
            r = _ok(run("partialDecrypt", cc, tmp / f"sigma{j}", agg, tmp / f"{tag}{j}.{ext}", *extra, "--parties", ",".join(map(str, T))))
            assert f"[pdecrypt] Key share of party {j} loaded ({t}-of-{n}, {len(T)} parties this round)\n" in r.stdout, r.stdout
            assert f"{'lead ' if extra else ''}share(s), smudged at sigma 2^20\n" in r.stdout and "Private key" not in r.stdout
        _ok(run("fuseDecryptions", cc, *(tmp / f"{tag}{j}.{ext}" for j in T), tmp / f"{tag}.json"))
        out = json.load(open(tmp / f"{tag}.json"))["weights_summary"]
        return max(np.abs(np.array(out[li]["values"]) - mean[li]).max() for li in range(2))

    for tag, T in (("a", (1, 3)), ("b", (2, 3)), ("c", (3, 1, 2))):
        err = fused_error(tag, T)
        print(f"parties {T}: error 2^{np.log2(err):.2f}")
        assert err < BOUND["p14"], (T, err)
    # shares made with different --parties sets fuse to noise: fuseDecryptions cannot tell
    _ok(run("fuseDecryptions", cc, tmp / f"a1.{ext}", tmp / f"b3.{ext}", tmp / "mixed.json"))
    mixed = json.load(open(tmp / "mixed.json"))["weights_summary"]
    assert np.abs(np.array(mixed[0]["values"]) - mean[0]).max() > 1
    # unchanged: the n-of-n round with the plain keys -- today's log lines, one share blob per ciphertext, the mean
    n_blobs = len(read_mkws(agg)[1])
    for p in (1, 2, 3):
        extra = ["--lead"] if p == 1 else []
        r = _ok(run("partialDecrypt", cc, tmp / f"sk{p}", agg, tmp / f"plain{p}.{ext}", *extra))
        assert r.stdout == ("[pdecrypt] CryptoContext loaded\n[pdecrypt] Private key loaded\n[pdecrypt] Encrypted weights loaded\n"
                            f"[pdecrypt] {n_blobs} {'lead ' if p == 1 else ''}share(s), smudged at sigma 2^20\n"
                            f"[pdecrypt] Partial decryption completed successfully. Output: {tmp / f'plain{p}.{ext}'}\n"), r.stdout
        assert os.path.getsize(tmp / f"plain{p}.{ext}") == os.path.getsize(tmp / f"a1.{ext}")
    _ok(run("fuseDecryptions", cc, *(tmp / f"plain{p}.{ext}" for p in (1, 2, 3)), tmp / "plain.json"))
    plain = json.load(open(tmp / "plain.json"))["weights_summary"]
    for li in range(2):
        assert np.abs(np.array(plain[li]["values"]) - mean[li]).max() < BOUND["p14"], li
    # misuse: exit 1, its message, nothing written
    out = tmp / f"bad.{ext}"
    cases = [
        ((tmp / "sigma1", agg, out), "a key share needs --parties"),
        ((tmp / "sigma1", agg, out, "--lead"), "a key share needs --parties"),
        ((tmp / "sk1", agg, out, "--parties", "1,3"), "--parties needs a combined key share"),
        ((tmp / "sigma1", agg, out, "--parties", "1"), "fewer parties than the threshold"),
        ((tmp / "sigma1", agg, out, "--parties", "2,3"), "does not name the key share's own party"),
        ((tmp / "sigma1", agg, out, "--parties", "1,4"), "above the share's n_parties"),
        ((tmp / "sigma1", agg, out, "--parties", "1,1"), "--parties needs distinct party indices"),
        ((tmp / "sigma1", agg, out, "--parties", "1,x"), "--parties needs distinct party indices"),
        ((tmp / "sigma1", agg, out, "--parties", "0,1"), "--parties needs distinct party indices"),
        ((tmp / "ks2.1", agg, out, "--parties", "1,3"), "one dealer's, not a combined share"),
    ]
    for args, msg in cases:
        r = run("partialDecrypt", cc, *args)
        assert r.returncode == 1 and "[pdecrypt] ERROR: " in r.stderr and msg in r.stderr and "Usage:" in r.stderr, (args, r.stdout + r.stderr)
        assert not os.path.exists(out), args
    cut = tmp / "cut"
    cut.write_bytes(open(tmp / "sigma1", "rb").read()[:-8])
    r = run("partialDecrypt", cc, cut, agg, out, "--parties", "1,3")
    assert r.returncode == 1 and "key-share blob has the wrong size" in r.stderr and not os.path.exists(out)
    sig = tmp / "sig"
    cases = [
        ((tmp / "ks1.1", tmp / "ks2.1"), "need the shares of all 3 dealers, got 2"),
        ((tmp / "ks1.1", tmp / "ks2.1", tmp / "ks2.1"), "two shares of dealer 2"),
        ((tmp / "ks1.1", tmp / "ks2.1", tmp / "ks3.2"), "shares differ in n_parties, threshold or to_party"),
        ((tmp / "ks1.1", tmp / "ks2.1", tmp / "sigma1"), "already a combined share"),
        ((tmp / "ks1.1", tmp / "ks2.1", tmp / "ks3.1", tmp / "again.1"), "two shares of dealer 1"),
        ((tmp / "ks1.1", tmp / "ks2.1", tmp / "sk3"), "not a mkckks key-share blob"),
        ((tmp / "ks1.1", tmp / "ks2.1", cut), "key-share blob has the wrong size"),
        ((tmp / "ks1.1", tmp / "ks2.1", tmp / "nofile"), "Could not open key-share file"),
    ]
    for files, msg in cases:
        r = run("combineKeyShares", cc, sig, *files)
        assert r.returncode == 1 and "[combine] ERROR: " in r.stderr and msg in r.stderr, (files, r.stdout + r.stderr)
        assert not os.path.exists(sig), files
    for args in ((3, 4, 1), (3, 0, 1), (65, 2, 1), (3, 2, 0), (3, 2, 4)):
        r = run("shareKey", cc, tmp / "sk1", *args, tmp / "nope")
        assert r.returncode == 1 and "[shareKey] ERROR: need 1 <= threshold <= n_parties <= 64" in r.stderr, (args, r.stderr)
    r = run("shareKey", cc, tmp / "nokey", 3, 2, 1, tmp / "nope")
    assert r.returncode == 1 and "[shareKey] ERROR: Failed to load private key" in r.stderr
    assert not [f for f in os.listdir(tmp) if f.startswith("nope")]
