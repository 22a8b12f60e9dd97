"""Ciphertext products on the device (include/mkckks.h: "ciphertext products").

    tensor:  (a0, a1) x (b0, b1) = (a0 b0, a0 b1 + a1 b0, a1 b1) pointwise mod q_i, summed over the terms
    relinearisation key = rekeygen with NTT(s_old) replaced by NTT(s)^2
    Relinearize(d0, d1, d2) = (d0, d1) + KeySwitch(d2, rlk);   mult_relin = Relinearize(tensor)

The oracle has no product, so every expectation is built from what it has: the tensor product is Python integer arithmetic
per limb, relinearisation is o.eval_add((d0, d1), o.reencrypt((0, d2), rlk)), and the key is o.rekeygen of the zero secret
(rekeygen is affine in its source key) plus (P mod q_i) sk_eval[i]^2 on each digit's own limbs.  Device results are
compared word for word.

Decoded values: `measure_products(name, seed)` runs the chain fresh ciphertexts -> rescale -> product -> full-span slot
sum on the CPU oracle composition and returns the largest errors of the slot-wise product, of <a, b> and of |a|^2.
PRODUCT_BOUND is 4 x the largest error seen over seeds 0 .. 5 (run `python -m tests.test_product` to print them; the
figures are in DESIGN.md "ciphertext products"): the margin test_rotation.py uses for the seed-to-seed spread of a maximum
over N/2 slots.  Nothing in a bound comes from a GPU result."""
import numpy as np
import pytest

from oracle.oracle import FastCpuContext, sample_gauss, sample_ternary
from tests.test_gpu_parity import CONFIGS, make_keys, make_rk_rand, rand_ct
from tests.test_rotation import gal, oracle_slot_sum, rand_evks, sigma_coeff

gpu = pytest.mark.gpu

# 4 x the largest of measure_products(name, seed) for seed 0 .. 5: {name: (slot-wise product, <a, b>, |a|^2)}
# measured: tiny 2^-32.41 .. 2^-31.15, 2^-33.03 .. 2^-28.89, 2^-32.83 .. 2^-28.84;
#           ref  2^-27.90 .. 2^-27.35, 2^-25.73 .. 2^-23.68, 2^-26.66 .. 2^-22.55
PRODUCT_BOUND = {"tiny": (4 * 2.0 ** -31.15, 4 * 2.0 ** -28.89, 4 * 2.0 ** -28.84),
                 "ref": (4 * 2.0 ** -27.35, 4 * 2.0 ** -23.68, 4 * 2.0 ** -22.55)}
POISON = 0xA5A5A5A5A5A5A5A5


# ---- the definitions in Python integers --------------------------------------------------------------------------------

def py_tensor(moduli, a, b):
    """a, b u64[T][2][nl][N] -> u64[3][nl][N]: sum over T of (a0 b0, a0 b1 + a1 b0, a1 b1) mod q_i, exact."""
    T, _, nl, N = a.shape
    out = np.empty((3, nl, N), dtype=np.uint64)
    for i in range(nl):
        q = int(moduli[i])
        d = [np.zeros(N, dtype=object) for _ in range(3)]
        for t in range(T):
            a0, a1 = a[t, 0, i].astype(object), a[t, 1, i].astype(object)
            b0, b1 = b[t, 0, i].astype(object), b[t, 1, i].astype(object)
            d[0] += a0 * b0
            d[1] += a0 * b1 + a1 * b0
            d[2] += a1 * b1
        for k in range(3):
            out[k, i] = np.array(d[k] % q, dtype=np.uint64)
    return out


def oracle_relinearize(o, d, rlk):
    """(d0, d1) + KeySwitch(d2, rlk) through the oracle's re-encryption of (0, d2)."""
    zero_d2 = np.stack([np.zeros_like(d[2]), d[2]])
    return o.eval_add(np.ascontiguousarray(d[:2]), o.reencrypt(zero_d2, rlk))


def oracle_relin_key(o, sk_eval, pk, u, e0, e1):
    """rekeygen(0, pk, u, e0, e1) + (P mod q_i) sk_eval[i]^2 on the own limbs of each digit, component 0."""
    evk = o.rekeygen(np.zeros(o.N, dtype=np.int8), pk, u, e0, e1)
    P = 1
    for m in o.moduli[o.L:]:
        P *= int(m)
    for j in range(o.beta):
        for i in range(j * o.alpha, min(o.L, (j + 1) * o.alpha)):
            q = int(o.moduli[i])
            s = sk_eval[i].astype(object)
            evk[j, 0, i] = np.array((evk[j, 0, i].astype(object) + (P % q) * s * s) % q, dtype=np.uint64)
    return evk


def with_edges(ct, moduli):
    """Residues 0 and q - 1 in every limb: index 0 all q - 1 (the edge of the lazy d1 sum), 1 all zero, 2 and 3 mixed."""
    ct = ct.copy()
    nl = ct.shape[-2]
    for i in range(nl):
        qm1 = np.uint64(int(moduli[i]) - 1)
        ct[..., i, 0] = qm1
        ct[..., i, 1] = 0
        ct[..., 0, i, 2] = qm1
        ct[..., 1, i, 2] = 0
        ct[..., 0, i, 3] = 0
        ct[..., 1, i, 3] = qm1
    return ct


# ---- decoded values on the CPU oracle: where PRODUCT_BOUND comes from ----------------------------------------------------

def product_case(o, seed):
    """A key pair, the relinearisation key's randomness, Galois-key randomness for the full-span slot sum, two value
    vectors in [-0.3, 0.3] and their fresh ciphertexts."""
    rng = np.random.default_rng(seed)
    N, L = o.N, o.L
    s, a, e = make_keys(o, rng)
    pk, sk = o.keygen(s, a, e)
    va, vb = rng.uniform(-0.3, 0.3, size=N // 2), rng.uniform(-0.3, 0.3, size=N // 2)
    enc = lambda v: o.encrypt(pk, o.encode(v, o.sf_big(0), L), sample_ternary(rng, N), sample_gauss(rng, N), sample_gauss(rng, N))
    cta, ctb = enc(va), enc(vb)
    m = (N // 2).bit_length() - 1
    return dict(s=s, pk=pk, sk=sk, va=va, vb=vb, cta=cta, ctb=ctb, rlk_rand=make_rk_rand(o, rng),
                rot_rand=[make_rk_rand(o, rng) for _ in range(m)], m=m)


def product_scale(o):
    """Scale of a product of two rescaled fresh ciphertexts: (sf_big(0) / q_{L-1})^2 on L - 1 limbs."""
    return (o.sf_big(0) / float(o.moduli[o.L - 1])) ** 2


def product_errors(o, case, prod_ab, sum_ab, sum_aa):
    sk, va, vb, S2 = case["sk"], case["va"], case["vb"], product_scale(o)
    return (np.abs(o.decrypt_decode(prod_ab, sk, S2) - va * vb).max(),
            np.abs(o.decrypt_decode(sum_ab, sk, S2) - np.dot(va, vb)).max(),
            np.abs(o.decrypt_decode(sum_aa, sk, S2) - np.dot(va, va)).max())


def measure_products(name, seed):
    """(error of a * b slot-wise, of <a, b>, of |a|^2): max over all slots of |decoded - expected| with every step on the
    CPU oracle composition."""
    c = CONFIGS[name]
    o = FastCpuContext(c[0], c[1], c[2], c[3], dnum=c[4])
    case = product_case(o, seed)
    ra, rb = o.rescale(case["cta"]), o.rescale(case["ctb"])
    rlk = oracle_relin_key(o, case["sk"], case["pk"], *case["rlk_rand"])
    evks = [o.rekeygen(sigma_coeff(case["s"], gal(o.N, 1 << k)), case["pk"], *case["rot_rand"][k]) for k in range(case["m"])]
    mod = o.moduli[:o.L - 1]
    ab = oracle_relinearize(o, py_tensor(mod, ra[None], rb[None]), rlk)
    aa = oracle_relinearize(o, py_tensor(mod, ra[None], ra[None]), rlk)
    return product_errors(o, case, ab, oracle_slot_sum(o, ab, evks, o.N // 2), oracle_slot_sum(o, aa, evks, o.N // 2))


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


@gpu
@pytest.mark.parametrize("name", ["tiny", "ref", "c3"])
def test_relin_keygen_is_the_construction_and_the_factored_keygens_keep_their_bits(ctxs, name):
    g, o = ctxs(name)
    N, D = g.N, g.D
    rng = np.random.default_rng(900 + N.bit_length())
    s, a, e = make_keys(o, rng)
    pk, sk = o.keygen(s, a, e)
    s2 = sample_ternary(rng, N)
    u, e0, e1 = make_rk_rand(o, rng)
    d_s, d_pk = g.to_device(s), g.to_device(pk)
    d_u, d_e0, d_e1 = g.to_device(u), g.to_device(e0), g.to_device(e1)
    d_evk = g.empty((g.beta, 2, D, N))
    g.relin_keygen(d_s, d_pk, d_u, d_e0, d_e1, d_evk)
    assert np.array_equal(d_evk.to_host(), oracle_relin_key(o, sk, pk, u, e0, e1)), name
    # the shared tail serves rekeygen and galois_keygen as before
    g.rekeygen(g.to_device(s2), d_pk, d_u, d_e0, d_e1, d_evk)
    assert np.array_equal(d_evk.to_host(), o.rekeygen(s2, pk, u, e0, e1)), name
    gel = gal(N, 3)
    g.galois_keygen(d_s, d_pk, d_u, d_e0, d_e1, gel, d_evk)
    assert np.array_equal(d_evk.to_host(), o.rekeygen(sigma_coeff(s, gel), pk, u, e0, e1)), name
    assert np.array_equal(d_s.to_host(), s) and np.array_equal(d_pk.to_host(), pk)


def dev_tensor(g, a, b, nl, square=False):
    """a, b u64[T][B][2][nl][N] -> (out3 u64[B][3][nl][N], the guard words around it are checked here)."""
    T, B = a.shape[:2]
    N = g.N
    words = B * 3 * nl * N
    d_big = g.to_device(np.full(words + 4 * N, POISON, dtype=np.uint64))
    d_out = d_big.view(2 * N, (B, 3, nl, N))
    d_a = g.to_device(a)
    d_b = d_a if square else g.to_device(b)
    g.tensor_sum(d_a, d_b, d_out, T, B, nl)
    big = d_big.to_host()
    assert np.all(big[:2 * N] == POISON) and np.all(big[2 * N + words:] == POISON)
    assert np.array_equal(d_a.to_host(), a)
    return d_out.to_host()


TENSOR_CASES = [("n11", 3, 2, 1), ("c1", 2, 2, 1), ("ref", 3, 2, 1), ("c3", 12, 1, 1), ("n17", 2, 1, 1)]


@gpu
@pytest.mark.parametrize("name,nl,B,T", TENSOR_CASES)
def test_tensor_sum_is_the_integer_definition(ctxs, name, nl, B, T):
    g, _ = ctxs(name)
    rng = np.random.default_rng(1000 + 7 * nl + g.N.bit_length())
    a = with_edges(np.stack([rand_ct(rng, g, nl, B) for _ in range(T)]), g.moduli)
    b = with_edges(np.stack([rand_ct(rng, g, nl, B) for _ in range(T)]), g.moduli)
    got = dev_tensor(g, a, b, nl)
    for i in range(B):
        assert np.array_equal(got[i], py_tensor(g.moduli, a[:, i], b[:, i])), (name, i)
    sq = dev_tensor(g, a, a, nl, square=True)
    assert np.array_equal(sq, dev_tensor(g, a, a.copy(), nl)), name  # the square path against the general path on copies
    assert np.array_equal(sq[0], py_tensor(g.moduli, a[:, 0], a[:, 0])), name


@gpu
@pytest.mark.parametrize("T", [1, 2, 5, 33])
def test_tensor_sum_on_every_level_and_term_count_of_the_small_ring(ctxs, T):
    """tiny has an integer-class q_0 and fp64-class limbs; every nl from 1 to L, 2 ciphertexts.  33 terms pass the fold
    of every class's lazy sums twice (16 terms pseudo-Mersenne, 2 terms fp64) with index 0 at q - 1 in all operands."""
    g, _ = ctxs("tiny")
    B = 2
    rng = np.random.default_rng(1100 + T)
    for nl in range(1, g.L + 1) if T <= 5 else (1, 2):
        a = with_edges(np.stack([rand_ct(rng, g, nl, B) for _ in range(T)]), g.moduli)
        b = with_edges(np.stack([rand_ct(rng, g, nl, B) for _ in range(T)]), g.moduli)
        got = dev_tensor(g, a, b, nl)
        for i in range(B):
            assert np.array_equal(got[i], py_tensor(g.moduli, a[:, i], b[:, i])), (T, nl, i)
        sq = dev_tensor(g, a, a, nl, square=True)
        assert np.array_equal(sq[1], py_tensor(g.moduli, a[:, 1], a[:, 1])), (T, nl)
    d_out = g.to_device(got)
    g.tensor_sum(g.to_device(a), g.to_device(b), d_out, T, 0, nl)  # empty: nothing written
    assert np.array_equal(d_out.to_host(), got)


RELIN_CASES = [("tiny", nl, 2) for nl in range(1, 6)] + [("ref", 3, 2), ("c3", 12, 2), ("c3", 11, 2)]
_relin = {}


def relin_case(o, name, nl, B):
    """Uniform random operands with the edge residues, a random key, the tensor product and the oracle's relinearisation
    of it, for (a, b) and for the square of a; computed once and shared (read-only)."""
    key = (name, nl, B)
    if key not in _relin:
        rng = np.random.default_rng(1200 + 31 * nl + B + o.N.bit_length())
        a, b = with_edges(rand_ct(rng, o, nl, B), o.moduli), with_edges(rand_ct(rng, o, nl, B), o.moduli)
        rlk = rand_evks(rng, o, 1)[0]
        d3 = np.stack([py_tensor(o.moduli, a[None, i], b[None, i]) for i in range(B)])
        want = np.stack([oracle_relinearize(o, d3[i], rlk) for i in range(B)])
        want_sq = oracle_relinearize(o, py_tensor(o.moduli, a[None, 0], a[None, 0]), rlk)
        for arr in (a, b, rlk, d3, want, want_sq):
            arr.setflags(write=False)
        _relin[key] = (a, b, rlk, d3, want, want_sq)
    return _relin[key]


def check_products(g, case, nl, tag):
    """relinearize_batch of the tensor product, mult_relin_batch out of place, onto a, onto b, and the square."""
    a, b, rlk, d3, want, want_sq = case
    B = a.shape[0]
    d_rlk, d_a, d_b = g.to_device(rlk), g.to_device(a), g.to_device(b)
    d_in3, d_out = g.to_device(d3), g.empty(a.shape)
    g.relinearize(d_in3, d_rlk, d_out, B, nl)
    assert np.array_equal(d_out.to_host(), want), (tag, "relinearize")
    assert np.array_equal(d_in3.to_host(), d3)
    d_out = g.empty(a.shape)
    g.mult_relin(d_a, d_b, d_rlk, d_out, B, nl)
    assert np.array_equal(d_out.to_host(), want), (tag, "mult_relin")
    assert np.array_equal(d_a.to_host(), a) and np.array_equal(d_b.to_host(), b)
    d_x = g.to_device(a)
    g.mult_relin(d_x, d_b, d_rlk, d_x, B, nl)  # d_out == d_a
    assert np.array_equal(d_x.to_host(), want), (tag, "out is a")
    d_x = g.to_device(b)
    g.mult_relin(d_a, d_x, d_rlk, d_x, B, nl)  # d_out == d_b
    assert np.array_equal(d_x.to_host(), want), (tag, "out is b")
    d_out = g.empty(a.shape)
    g.mult_relin(d_a, d_a, d_rlk, d_out, B, nl)  # d_a == d_b
    assert np.array_equal(d_out.to_host()[0], want_sq), (tag, "square")


@gpu
@pytest.mark.parametrize("name,nl,B", RELIN_CASES)
def test_relinearize_and_mult_relin_are_the_oracle_composition(ctxs, name, nl, B):
    g, o = ctxs(name)
    check_products(g, relin_case(o, name, nl, B), nl, (name, nl))


@gpu
@pytest.mark.parametrize("name,nl", [("c3", 12), ("ref", 3)])
@pytest.mark.parametrize("env", [{"MKCKKS_GENERIC_NTT": "1"}, {"MKCKKS_NO_FP64": "1"}, {"MKCKKS_NO_PM": "1"}, {"MKCKKS_CHUNK": "1"}])
def test_products_under_the_library_switches(ctxs, monkeypatch, env, name, nl):
    """Switches are read once, when a context is created: a fresh context under each gives the same bits -- the tensor
    kernel takes its arithmetic class from the limb table the switches shape."""
    from ppqsflhe_amd import Context
    _, o = ctxs(name)
    case = relin_case(o, name, nl, 2)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    c = CONFIGS[name]
    g = Context(c[0], c[1], c[2], c[3], dnum=c[4], device=0)
    try:
        check_products(g, case, nl, (name, env))
        a, b, _, d3, _, _ = case
        assert np.array_equal(dev_tensor(g, a[None], b[None], nl), d3), (name, env)
    finally:
        g.close()


@gpu
def test_products_across_workspace_chunks(ctxs, monkeypatch):
    """More ciphertexts than a chunk: MKCKKS_CHUNK = 2, 5 ciphertexts, in a fresh context."""
    from ppqsflhe_amd import Context
    _, o = ctxs("tiny")
    monkeypatch.setenv("MKCKKS_CHUNK", "2")
    c = CONFIGS["tiny"]
    g = Context(c[0], c[1], c[2], c[3], dnum=c[4], device=0)
    try:
        check_products(g, relin_case(o, "tiny", 4, 5), 4, "chunks")
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("name", ["tiny", "ref"])
def test_decoded_values_of_products_and_inner_products(ctxs, name):
    """Real encode / encrypt under a generated key; relinearisation and Galois keys, rescale, products and slot sums on
    the device; decryption and decoding on the oracle."""
    g, o = ctxs(name)
    N, L, D = g.N, g.L, g.D
    case = product_case(o, 5)
    d_s, d_pk = g.to_device(case["s"]), g.to_device(case["pk"])
    keygen_args = lambda rnd: [g.to_device(x) for x in rnd]
    d_rlk = g.empty((g.beta, 2, D, N))
    g.relin_keygen(d_s, d_pk, *keygen_args(case["rlk_rand"]), d_rlk)
    assert np.array_equal(d_rlk.to_host(), oracle_relin_key(o, case["sk"], case["pk"], *case["rlk_rand"]))
    m, per_key = case["m"], g.beta * 2 * D * N
    d_evks = g.empty((m, g.beta, 2, D, N))
    for k in range(m):
        g.galois_keygen(d_s, d_pk, *keygen_args(case["rot_rand"][k]), g.galois_element(1 << k),
                        d_evks.view(k * per_key, (g.beta, 2, D, N)))
    d_a, d_b = g.empty((1, 2, L - 1, N)), g.empty((1, 2, L - 1, N))
    g.rescale(g.to_device(case["cta"][None]), d_a, 1, L)
    g.rescale(g.to_device(case["ctb"][None]), d_b, 1, L)
    assert np.array_equal(d_a.to_host()[0], o.rescale(case["cta"]))
    d_ab, d_aa = g.empty((1, 2, L - 1, N)), g.empty((1, 2, L - 1, N))
    g.mult_relin(d_a, d_b, d_rlk, d_ab, 1, L - 1)
    g.mult_relin(d_a, d_a, d_rlk, d_aa, 1, L - 1)
    d_sab, d_saa = g.empty((1, 2, L - 1, N)), g.empty((1, 2, L - 1, N))
    g.slot_sum(d_ab, d_evks, d_sab, 1, L - 1, N // 2)
    g.slot_sum(d_aa, d_evks, d_saa, 1, L - 1, N // 2)
    errs = product_errors(o, case, d_ab.to_host()[0], d_sab.to_host()[0], d_saa.to_host()[0])
    print(f"{name}: product error 2^{np.log2(errs[0]):.2f}, <a, b> error 2^{np.log2(errs[1]):.2f}, "
          f"|a|^2 error 2^{np.log2(errs[2]):.2f}")
    for err, bound in zip(errs, PRODUCT_BOUND[name]):
        assert err <= bound, (name, errs, PRODUCT_BOUND[name])


if __name__ == "__main__":
    for cfg in ("tiny", "ref"):
        errs = [measure_products(cfg, seed) for seed in range(6)]
        for seed, e in enumerate(errs):
            print(f"{cfg} seed {seed}: product 2^{np.log2(e[0]):.2f}, <a, b> 2^{np.log2(e[1]):.2f}, |a|^2 2^{np.log2(e[2]):.2f}")
        for k, what in enumerate(("product", "<a, b>", "|a|^2")):
            col = [e[k] for e in errs]
            print(f"{cfg}: {what} 2^{np.log2(min(col)):.2f} .. 2^{np.log2(max(col)):.2f}")
