"""Collective evaluation keys of a joint key (include/mkckks.h: "collective evaluation keys"; DESIGN.md section of the
same name).

    Galois key for g:  share_p = galois_keygen(s_p, pk_joint, ...)                    key = sum_p share_p
    relinearisation:   K1 = sum_p rekeygen(s_p, pk_joint, ...)
                       share_p[j][c][i] = K1[j][c][i] * sk_p[i] + NTT_i(e_c[j]) mod q_i   key = sum_p share_p

Every device result is compared word for word with Python integer arithmetic (the share formula, the sums) or with the
oracle's rekeygen (the Galois shares).

Key error.  A fused key decrypts under S = sum sk_p to the gadget term plus an error; the noise rule (mkckks.h) predicts
its standard deviation: with n parties, ring size N, sigma = 3.19 and ternary secrets (variance 2/3),
    Galois key:  var = n * (N n sigma^2 2/3  +  sigma^2  +  N sigma^2 2n/3)          (e_pk u_p + e0_p + e1_p S, n parties)
    relin key:   var = N (2n/3) var(n1) + n sigma^2 + N n sigma^2 2n/3,  var(n1) = n sigma^2 (1 + 4 n N / 3)
KEY_SIGMAS = 8 standard deviations bound the maximum over the beta * D * N coefficients of a key: a coefficient is a sum
of N products, close to normal, and 8 sd leaves 1e-15 per sample against at most 2^21 samples per key here.

Decoded values.  `measure_collective(name, seed)` runs the chain on the CPU oracle: 3 parties, joint key, collective
Galois keys for all log2(N/2) steps, collective relinearisation key, two vectors in [-0.3, 0.3] under the joint key,
rescale, product, full-span slot sum, decryption with sum sk_p.  COLLECTIVE_BOUND is 4 x the largest error over seeds
0 .. 5 (`python -m tests.test_collective_keys` prints them), the margin test_product.py uses.  Nothing in a bound comes
from a GPU result.  Measured ranges over seeds 0 .. 5 (slot-wise product, <a, b>, |a|^2), with the single-owner figures
of test_product.PRODUCT_BOUND beside them:
    tiny  collective 2^-31.70 .. 2^-31.37, 2^-32.64 .. 2^-28.87, 2^-33.19 .. 2^-28.12
          single     2^-32.41 .. 2^-31.15, 2^-33.03 .. 2^-28.89, 2^-32.83 .. 2^-28.84
    ref   collective 2^-26.95 .. 2^-26.34, 2^-27.42 .. 2^-23.16, 2^-24.85 .. 2^-21.73
          single     2^-27.90 .. 2^-27.35, 2^-25.73 .. 2^-23.68, 2^-26.66 .. 2^-22.55
At tiny the collective key costs nothing visible (the product's own terms dominate); at ref it costs about one bit in the
slot-wise product and less than one in the sums."""
import numpy as np
import pytest

from oracle.oracle import FastCpuContext, sample_gauss, sample_ternary
from tests.test_gpu_parity import CONFIGS, make_rk_rand
from tests.test_product import oracle_relinearize, product_errors, product_scale, py_tensor
from tests.test_rotation import gal, oracle_slot_sum, rand_evks, sigma_coeff
from tests.test_threshold_decrypt import key_chain

gpu = pytest.mark.gpu

N_PARTIES = 3
SIGMA = 3.19
KEY_SIGMAS = 8.0
# 4 x the largest of measure_collective(name, seed) for seed 0 .. 5: {name: (slot-wise product, <a, b>, |a|^2)}
COLLECTIVE_BOUND = {"tiny": (4 * 2.0 ** -31.37, 4 * 2.0 ** -28.87, 4 * 2.0 ** -28.12),
                    "ref": (4 * 2.0 ** -26.34, 4 * 2.0 ** -23.16, 4 * 2.0 ** -21.73)}
POISON = 0xA5A5A5A5A5A5A5A5
E31 = (1 << 31) - 1


# ---- the definitions in Python integers --------------------------------------------------------------------------------

def py_sum(moduli, shares):
    """shares u64[n][...][D][N] -> u64[...][D][N]: sum over the first axis mod q_i on all D limbs, exact."""
    acc = np.zeros(shares.shape[1:], dtype=object)
    for p in range(shares.shape[0]):
        acc += shares[p].astype(object)
    out = np.empty(shares.shape[1:], dtype=np.uint64)
    for i in range(shares.shape[-2]):
        out[..., i, :] = np.array(acc[..., i, :] % int(moduli[i]), dtype=np.uint64)
    return out


def lift(e, q):
    """signed integers -> residues in [0, q), exact"""
    return np.mod(np.asarray(e, dtype=np.int64), np.int64(q)).astype(np.uint64)


def py_relin_share(o, key1, sk, e0, e1):
    """share[j][c][i] = key1[j][c][i] * sk[i] + NTT_i(e_c[j]) mod q_i on all D limbs."""
    out = np.empty_like(key1)
    for i in range(o.D):
        q = int(o.moduli[i])
        s = sk[i].astype(object)
        for j in range(o.beta):
            for c, e in ((0, e0), (1, e1)):
                ee = o.ntt_fwd(i, lift(e[j], q)).astype(object)
                out[j, c, i] = np.array((key1[j, c, i].astype(object) * s + ee) % q, dtype=np.uint64)
    return out


def key_error(o, key, S_eval, src_eval):
    """Largest |coefficient| of key[j][0] + key[j][1] S - (P mod q_i) src on digit j's own limbs, over all digits and all D
    limbs: what a key for `src` under the secret S carries beside its gadget term."""
    P = 1
    for m in o.moduli[o.L:]:
        P *= int(m)
    worst = 0
    for j in range(o.beta):
        for i in range(o.D):
            q = int(o.moduli[i])
            own = j * o.alpha <= i < min(o.L, (j + 1) * o.alpha)
            x = key[j, 0, i].astype(object) + key[j, 1, i].astype(object) * S_eval[i].astype(object)
            if own:
                x = x - (P % q) * src_eval[i].astype(object)
            c = o.ntt_inv(i, np.array(x % q, dtype=np.uint64)).astype(object)
            c = np.where(c > q // 2, c - q, c)
            worst = max(worst, int(np.abs(c).max()))
    return worst


def galois_key_sd(n, N):
    return np.sqrt(n * (N * n * SIGMA ** 2 * 2 / 3 + SIGMA ** 2 + N * SIGMA ** 2 * 2 * n / 3))


def relin_key_sd(n, N):
    var_n1 = n * SIGMA ** 2 * (1 + 4 * n * N / 3)
    return np.sqrt(N * (2 * n / 3) * var_n1 + n * SIGMA ** 2 + N * n * SIGMA ** 2 * 2 * n / 3)


# ---- the chain: its randomness, and the keys on the CPU oracle -------------------------------------------------------

def collective_case(o, seed, n=N_PARTIES):
    rng = np.random.default_rng(seed)
    N, L = o.N, o.L
    keys = key_chain(o, rng, n)
    pk = keys[-1][1]
    S_eval = py_sum(o.moduli, np.stack([k[2] for k in keys]))
    S_coef = np.sum([k[0].astype(np.int64) for k in keys], axis=0)
    m = (N // 2).bit_length() - 1
    va, vb = rng.uniform(-0.3, 0.3, size=N // 2), rng.uniform(-0.3, 0.3, size=N // 2)
    enc = lambda v: o.encrypt(pk, o.encode(v, o.sf_big(0), L), sample_ternary(rng, N), sample_gauss(rng, N), sample_gauss(rng, N))
    return dict(keys=keys, pk=pk, sk=S_eval, S_coef=S_coef, m=m, va=va, vb=vb, cta=enc(va), ctb=enc(vb), n=n,
                rot_rand=[[make_rk_rand(o, rng) for _ in range(n)] for _ in range(m)],
                r1_rand=[make_rk_rand(o, rng) for _ in range(n)],
                r2_rand=[make_rk_rand(o, rng)[1:] for _ in range(n)])


def eval_of(o, coef):
    """signed coefficient vector -> u64[D][N] EVALUATION"""
    return np.stack([o.ntt_fwd(i, lift(coef, int(o.moduli[i]))) for i in range(o.D)])


def oracle_collective_keys(o, case):
    """(Galois keys u64[m][beta][2][D][N], K1, relinearisation key), each asserted to decrypt under S to its gadget term
    plus an error below KEY_SIGMAS predicted standard deviations."""
    n, N = case["n"], o.N
    s = [k[0] for k in case["keys"]]
    sk = [k[2] for k in case["keys"]]
    evks = []
    for k in range(case["m"]):
        g = gal(N, 1 << k)
        evks.append(py_sum(o.moduli, np.stack([o.rekeygen(sigma_coeff(s[p], g), case["pk"], *case["rot_rand"][k][p])
                                               for p in range(n)])))
    evks = np.stack(evks)
    for k in (0, case["m"] - 1):
        err = key_error(o, evks[k], case["sk"], eval_of(o, sigma_coeff(case["S_coef"], gal(N, 1 << k))))
        assert err <= KEY_SIGMAS * galois_key_sd(n, N), (k, err, galois_key_sd(n, N))
    K1 = py_sum(o.moduli, np.stack([o.rekeygen(s[p], case["pk"], *case["r1_rand"][p]) for p in range(n)]))
    rlk = py_sum(o.moduli, np.stack([py_relin_share(o, K1, sk[p], *case["r2_rand"][p]) for p in range(n)]))
    S2 = np.stack([np.array(case["sk"][i].astype(object) ** 2 % int(o.moduli[i]), dtype=np.uint64) for i in range(o.D)])
    err = key_error(o, rlk, case["sk"], S2)
    assert err <= KEY_SIGMAS * relin_key_sd(n, N), (err, relin_key_sd(n, N))
    case["key_errors"] = (err, relin_key_sd(n, N))
    return evks, K1, rlk


def measure_collective(name, seed):
    """(error of a * b slot-wise, of <a, b>, of |a|^2): max over all slots of |decoded - expected|, every step on the CPU
    oracle composition, keys made collectively by 3 parties, decryption with sum sk_p."""
    c = CONFIGS[name]
    o = FastCpuContext(c[0], c[1], c[2], c[3], dnum=c[4])
    case = collective_case(o, seed)
    evks, _, rlk = oracle_collective_keys(o, case)
    ra, rb = o.rescale(case["cta"]), o.rescale(case["ctb"])
    mod = o.moduli[:o.L - 1]
    ab = oracle_relinearize(o, py_tensor(mod, ra[None], rb[None]), rlk)
    aa = oracle_relinearize(o, py_tensor(mod, ra[None], ra[None]), rlk)
    return product_errors(o, case, ab, oracle_slot_sum(o, ab, evks, o.N // 2), oracle_slot_sum(o, aa, evks, o.N // 2))


def test_collective_chain_on_the_cpu_oracle():
    """tiny, seed 0: the keys' errors are inside the noise rule (asserted in oracle_collective_keys) and the decoded
    values inside COLLECTIVE_BOUND."""
    errs = measure_collective("tiny", 0)
    for err, bound in zip(errs, COLLECTIVE_BOUND["tiny"]):
        assert err <= bound, (errs, COLLECTIVE_BOUND["tiny"])


def test_a_lone_share_is_no_key():
    """A single party's round-2 share decrypts to noise of the size of the modulus, not to the gadget term."""
    c = CONFIGS["tiny"]
    o = FastCpuContext(c[0], c[1], c[2], c[3], dnum=c[4])
    case = collective_case(o, 1)
    s, sk = [k[0] for k in case["keys"]], [k[2] for k in case["keys"]]
    K1 = py_sum(o.moduli, np.stack([o.rekeygen(s[p], case["pk"], *case["r1_rand"][p]) for p in range(case["n"])]))
    lone = py_relin_share(o, K1, sk[0], *case["r2_rand"][0])
    S2 = np.stack([np.array(case["sk"][i].astype(object) ** 2 % int(o.moduli[i]), dtype=np.uint64) for i in range(o.D)])
    assert key_error(o, lone, case["sk"], S2) > 2 ** 30


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctxs():
    from ppqsflhe_amd import Context
    cache = {}

    def get(name):
        if name not in cache:
            a = CONFIGS[name]
            cache[name] = (Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0),
                           FastCpuContext(a[0], a[1], a[2], a[3], dnum=a[4]))
        return cache[name]

    yield get
    for g, _ in cache.values():
        g.close()


def dev_evk_sum(g, shares, in_place=False):
    """shares u64[n][n_keys][beta][2][D][N] -> the device sum, output poisoned first and its guard words checked."""
    n, n_keys = shares.shape[:2]
    words = int(np.prod(shares.shape[1:]))
    d_in = g.to_device(shares)
    if in_place:
        g.evk_sum(d_in, d_in, n, n_keys)
        back = d_in.to_host()
        assert np.array_equal(back[1:], shares[1:])
        return back[0]
    d_big = g.to_device(np.full(words + 4 * g.N, POISON, dtype=np.uint64))
    d_out = d_big.view(2 * g.N, shares.shape[1:])
    g.evk_sum(d_in, d_out, n, n_keys)
    big = d_big.to_host()
    assert np.all(big[:2 * g.N] == POISON) and np.all(big[2 * g.N + words:] == POISON)
    assert np.array_equal(d_in.to_host(), shares)
    return d_out.to_host()


@gpu
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_evk_sum_is_the_integer_sum(ctxs, n):
    g, o = ctxs("tiny")
    rng = np.random.default_rng(2000 + n)
    shares = rand_evks(rng, o, n * 2).reshape(n, 2, o.beta, 2, o.D, o.N)
    for i in range(o.D):
        shares[..., i, 0] = np.uint64(int(o.moduli[i]) - 1)
        shares[..., i, 1] = 0
    want = py_sum(o.moduli, shares)
    assert np.array_equal(dev_evk_sum(g, shares), want), n
    assert np.array_equal(dev_evk_sum(g, shares, in_place=True), want), n
    d_out = g.to_device(want)
    g.evk_sum(g.to_device(shares), d_out, n, 0)  # no keys: nothing written
    assert np.array_equal(d_out.to_host(), want)


@gpu
def test_evk_sum_of_64_parties_at_q_minus_1(ctxs):
    """64 * (2^61 - 1) does not fit 64 bits: the lazy sum must fold.  Every residue of every party is q - 1."""
    g, o = ctxs("tiny")
    shares = np.empty((64, 1, o.beta, 2, o.D, o.N), dtype=np.uint64)
    for i in range(o.D):
        shares[..., i, :] = np.uint64(int(o.moduli[i]) - 1)
    want = np.empty(shares.shape[1:], dtype=np.uint64)
    for i in range(o.D):
        q = int(o.moduli[i])
        want[..., i, :] = np.uint64(64 * (q - 1) % q)
    assert np.array_equal(dev_evk_sum(g, shares), want)
    assert np.array_equal(dev_evk_sum(g, shares, in_place=True), want)


_share = {}


def share_case(o, name):
    """A random round-1 key and secret with residues 0 and q - 1 in every limb (P limbs included), errors with
    +-(2^31 - 1), and the share in Python integers; computed once per configuration and shared (read-only)."""
    if name not in _share:
        rng = np.random.default_rng(2100 + o.N.bit_length() + o.D)
        key1 = rand_evks(rng, o, 1)[0]
        sk = rand_evks(rng, o, 1)[0, 0, 0].copy()
        for i in range(o.D):
            qm1 = np.uint64(int(o.moduli[i]) - 1)
            key1[..., i, 0], key1[..., i, 1], key1[..., i, 2], key1[..., i, 3] = qm1, 0, qm1, 0
            sk[i, 0], sk[i, 1], sk[i, 2], sk[i, 3] = qm1, qm1, 0, 0
        _, e0, e1 = make_rk_rand(o, rng)
        e0[:, 0], e0[:, 1], e1[:, 0], e1[:, 2] = E31, -E31, -E31, E31
        e0[-1, -1], e1[-1, -1] = E31, -E31
        want = py_relin_share(o, key1, sk, e0, e1)
        for arr in (key1, sk, e0, e1, want):
            arr.setflags(write=False)
        _share[name] = (key1, sk, e0, e1, want)
    return _share[name]


def check_relin_share(g, case, tag):
    key1, sk, e0, e1, want = case
    N = g.N
    words = key1.size
    d_key1, d_sk, d_e0, d_e1 = g.to_device(key1), g.to_device(sk), g.to_device(e0), g.to_device(e1)
    d_big = g.to_device(np.full(words + 4 * N, POISON, dtype=np.uint64))
    d_out = d_big.view(2 * N, key1.shape)
    g.relin_share(d_key1, d_sk, d_e0, d_e1, d_out)
    big = d_big.to_host()
    assert np.all(big[:2 * N] == POISON) and np.all(big[2 * N + words:] == POISON), tag
    assert np.array_equal(d_out.to_host(), want), (tag, "out of place")
    assert np.array_equal(d_key1.to_host(), key1) and np.array_equal(d_sk.to_host(), sk), tag
    assert np.array_equal(d_e0.to_host(), e0) and np.array_equal(d_e1.to_host(), e1), tag
    g.relin_share(d_key1, d_sk, d_e0, d_e1, d_key1)  # d_share == d_key1
    assert np.array_equal(d_key1.to_host(), want), (tag, "in place")
    assert np.array_equal(d_sk.to_host(), sk) and np.array_equal(d_e0.to_host(), e0) and np.array_equal(d_e1.to_host(), e1), tag


@gpu
@pytest.mark.parametrize("name", ["tiny", "c1", "ref", "c5s", "c3", "n11", "n17"])
def test_relin_share_is_the_integer_formula(ctxs, name):
    g, o = ctxs(name)
    check_relin_share(g, share_case(o, name), name)


@gpu
@pytest.mark.parametrize("name", ["c3", "ref"])
@pytest.mark.parametrize("env", [{"MKCKKS_GENERIC_NTT": "1"}, {"MKCKKS_NO_FP64": "1"}, {"MKCKKS_NO_PM": "1"}, {"MKCKKS_CHUNK": "1"},
                                 {"MKCKKS_RELSHARE_FUSED": "0"}])
def test_relin_share_under_the_library_switches(ctxs, monkeypatch, env, name):
    """Switches are read once, when a context is created: a fresh context under each gives the same bits (the first three
    take the composition, as does MKCKKS_RELSHARE_FUSED=0)."""
    from ppqsflhe_amd import Context
    _, o = ctxs(name)
    case = share_case(o, name)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    c = CONFIGS[name]
    g = Context(c[0], c[1], c[2], c[3], dnum=c[4], device=0)
    try:
        check_relin_share(g, case, (name, env))
    finally:
        g.close()


def device_galois_shares(g, case, k):
    """The n parties' shares for step 2^k, u64[n][1][beta][2][D][N] on the device."""
    n, per_key = case["n"], g.beta * 2 * g.D * g.N
    d_pk = g.to_device(case["pk"])
    d_shares = g.empty((n, 1, g.beta, 2, g.D, g.N))
    for p in range(n):
        u, e0, e1 = case["rot_rand"][k][p]
        g.galois_keygen(g.to_device(case["keys"][p][0]), d_pk, g.to_device(u), g.to_device(e0), g.to_device(e1),
                        g.galois_element(1 << k), d_shares.view(p * per_key, (g.beta, 2, g.D, g.N)))
    return d_shares


@gpu
@pytest.mark.parametrize("name", ["tiny", "ref"])
def test_collective_chain_on_the_device(ctxs, name):
    """Shares from galois_keygen(s_p, pk_joint) and rekeygen(s_p, pk_joint) summed on the device equal the oracle's
    rekeygen summed in integers; relin_share x 3 summed equals the integer formula; then rescale, products and slot sums
    on the device with the collective keys, decryption with sum sk_p on the oracle, held to COLLECTIVE_BOUND."""
    g, o = ctxs(name)
    N, L, D, n = g.N, g.L, g.D, N_PARTIES
    case = collective_case(o, 5)
    evks, K1, rlk = oracle_collective_keys(o, case)
    m, per_key, kshape = case["m"], g.beta * 2 * D * N, (g.beta, 2, D, N)
    d_evks = g.empty((m,) + kshape)
    for k in range(m):
        g.evk_sum(device_galois_shares(g, case, k), d_evks.view(k * per_key, (1,) + kshape), n, 1)
    assert np.array_equal(d_evks.to_host(), evks), name
    d_pk = g.to_device(case["pk"])
    d_r1 = g.empty((n, 1) + kshape)
    for p in range(n):
        g.rekeygen(g.to_device(case["keys"][p][0]), d_pk, *[g.to_device(x) for x in case["r1_rand"][p]],
                   d_r1.view(p * per_key, kshape))
    d_K1 = g.empty(kshape)
    g.evk_sum(d_r1, d_K1, n, 1)
    assert np.array_equal(d_K1.to_host(), K1), name
    d_r2 = g.empty((n, 1) + kshape)
    for p in range(n):
        e0, e1 = case["r2_rand"][p]
        g.relin_share(d_K1, g.to_device(case["keys"][p][2]), g.to_device(e0), g.to_device(e1), d_r2.view(p * per_key, kshape))
    d_rlk = d_r2.view(0, kshape)
    g.evk_sum(d_r2, d_rlk, n, 1)  # onto the first share
    assert np.array_equal(d_rlk.to_host(), rlk), name

    d_a, d_b = g.empty((1, 2, L - 1, N)), g.empty((1, 2, L - 1, N))
    g.rescale(g.to_device(case["cta"][None]), d_a, 1, L)
    g.rescale(g.to_device(case["ctb"][None]), d_b, 1, L)
    d_ab, d_aa = g.empty((1, 2, L - 1, N)), g.empty((1, 2, L - 1, N))
    g.mult_relin(d_a, d_b, d_rlk, d_ab, 1, L - 1)
    g.mult_relin(d_a, d_a, d_rlk, d_aa, 1, L - 1)
    d_sab, d_saa = g.empty((1, 2, L - 1, N)), g.empty((1, 2, L - 1, N))
    g.slot_sum(d_ab, d_evks, d_sab, 1, L - 1, N // 2)
    g.slot_sum(d_aa, d_evks, d_saa, 1, L - 1, N // 2)
    errs = product_errors(o, case, d_ab.to_host()[0], d_sab.to_host()[0], d_saa.to_host()[0])
    print(f"{name}: product error 2^{np.log2(errs[0]):.2f}, <a, b> error 2^{np.log2(errs[1]):.2f}, "
          f"|a|^2 error 2^{np.log2(errs[2]):.2f}; relin key error {case['key_errors'][0]} (sd {case['key_errors'][1]:.3g})")
    for err, bound in zip(errs, COLLECTIVE_BOUND[name]):
        assert err <= bound, (name, errs, COLLECTIVE_BOUND[name])


if __name__ == "__main__":
    for cfg in ("tiny", "ref"):
        errs = [measure_collective(cfg, seed) for seed in range(6)]
        for seed, e in enumerate(errs):
            print(f"{cfg} seed {seed}: product 2^{np.log2(e[0]):.2f}, <a, b> 2^{np.log2(e[1]):.2f}, |a|^2 2^{np.log2(e[2]):.2f}")
        for k, what in enumerate(("product", "<a, b>", "|a|^2")):
            col = [e[k] for e in errs]
            print(f"{cfg}: {what} 2^{np.log2(min(col)):.2f} .. 2^{np.log2(max(col)):.2f}")
