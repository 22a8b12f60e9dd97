"""Slot rotations and slot sums on the device (include/mkckks.h: "slot rotations and slot sums").

    sigma_g(a)(X) = a(X^g);   EVALUATION: sigma_g(X)[i] = X[src(i)], 2 brev(src(i)) + 1 = (2 brev(i) + 1) g mod 2N
    Galois key for g = rekeygen(sigma_g(s), pk);   Rotate(ct, g) = ReEncrypt((sigma_g(c0), sigma_g(c1)), evk_g)
    SlotSum(ct, 2^m): ct <- ct + Rotate(ct, 5^(2^k)), k = 0 .. m - 1

Every device result is compared word for word: the automorphism with the definition on coefficients (numpy: coefficient k
to position k g mod 2N, negated past N) between the oracle's transforms, the keys with the oracle's rekeygen on the permuted
secret, rotations and slot sums with the oracle's reencrypt / eval_add on ciphertexts gathered with `src_index` below.

Decoded values: a rotation must not cost more than 4 x the decoded error of the unrotated ciphertext in the same test (the
CPU check of the construction saw at most 1.93 x in 18 cases; the margin covers the seed-to-seed spread of a maximum over
N/2 slots).  Full-span slot sums and inner products are held to SUM_BOUND = 4 x the largest error `measure_sums` gives on
the CPU oracle over seeds 0 .. 5 at the same parameters (run `python -m tests.test_rotation` to print them; the figures
are in DESIGN.md "rotations and slot sums"); nothing in the bound comes from a GPU result."""
import numpy as np
import pytest

from oracle.oracle import FastCpuContext, sample_gauss, sample_ternary
from tests.test_gpu_parity import CONFIGS, make_keys, make_rk_rand, rand_ct, rand_polys
from tests.test_slot_weights import py_product

gpu = pytest.mark.gpu

# 4 x the largest of measure_sums(name, seed) for seed 0 .. 5: {name: (slot sum, inner product)}
# measured: tiny 2^-44.78 .. 2^-41.13 and 2^-38.56 .. 2^-35.66; ref 2^-36.94 .. 2^-34.50 and 2^-35.59 .. 2^-30.55
SUM_BOUND = {"tiny": (4 * 2.0 ** -41.13, 4 * 2.0 ** -35.66), "ref": (4 * 2.0 ** -34.50, 4 * 2.0 ** -30.55)}


# ---- the definitions in numpy ---------------------------------------------------------------------------------------

def brev(x, bits):
    x = np.asarray(x, dtype=np.int64)
    out = np.zeros_like(x)
    for b in range(bits):
        out |= ((x >> b) & 1) << (bits - 1 - b)
    return out


def src_index(N, g):
    """sigma_g in EVALUATION format is out = in[src_index(N, g)]."""
    bits = N.bit_length() - 1
    k = brev(np.arange(N), bits)
    ks = (((2 * k + 1) * g) % (2 * N) - 1) // 2
    return brev(ks, bits)


def sigma_coeff(a, g, q=None):
    """sigma_g on a coefficient vector: coefficient k goes to position k g mod 2N; past N the sign flips (mod q: q - a)."""
    a = np.asarray(a)
    N = a.shape[-1]
    t = (np.arange(N, dtype=np.int64) * g) % (2 * N)
    neg = t >= N
    flipped = -a if q is None else np.where(a == 0, a, (np.uint64(q) - a).astype(a.dtype))
    out = np.empty_like(a)
    out[t % N] = np.where(neg, flipped, a)
    return out


def gal(N, r):
    return pow(5, r, 2 * N)


def oracle_rotate(o, ct, evk, g):
    return o.reencrypt(np.ascontiguousarray(ct[:, :, src_index(o.N, g)]), evk)


def oracle_slot_sum(o, ct, evks, span):
    k = 0
    while (1 << k) < span:
        ct = o.eval_add(ct, oracle_rotate(o, ct, evks[k], gal(o.N, 1 << k)))
        k += 1
    return ct


def rand_evks(rng, o, n):
    return rand_polys(rng, o, list(range(o.D)) * (2 * o.beta), n).reshape(n, o.beta, 2, o.D, o.N)


# ---- decoded values on the CPU oracle: where SUM_BOUND comes from -----------------------------------------------------

def keyed_case(o, seed, steps):
    """A key pair, Galois keys for the rotation steps in `steps`, values, per-slot factors and a fresh ciphertext."""
    rng = np.random.default_rng(seed)
    N, L = o.N, o.L
    s, a, e = make_keys(o, rng)
    pk, sk = o.keygen(s, a, e)
    vals = rng.uniform(-0.3, 0.3, size=N // 2)
    w = rng.uniform(0.0, 1.0, size=N // 2)
    ct = o.encrypt(pk, o.encode(vals, o.sf_big(0), L), sample_ternary(rng, N), sample_gauss(rng, N), sample_gauss(rng, N))
    rk = {r: make_rk_rand(o, rng) for r in steps}
    return dict(s=s, pk=pk, sk=sk, vals=vals, w=w, ct=ct, rk=rk, rng=rng)


def oracle_galois_key(o, case, r):
    return o.rekeygen(sigma_coeff(case["s"], gal(o.N, r)), case["pk"], *case["rk"][r])


def weighted(o, case):
    """Rescale(ct * encode(w, sf(1))): L - 1 limbs at scale sf_big(0) * sf(1) / q_{L-1}."""
    L = o.L
    pt = o.encode(case["w"], o.sf(1), L)
    return o.rescale(py_product(o, case["ct"], pt)), o.sf_big(0) * o.sf(1) / float(o.moduli[L - 1])


def measure_sums(name, seed):
    """(error of the full-span slot sum of a fresh ciphertext, error of the inner product with per-slot factors): max over
    all slots of |decoded - expected| on the CPU oracle."""
    a = CONFIGS[name]
    o = FastCpuContext(a[0], a[1], a[2], a[3], dnum=a[4])
    N = o.N
    m = (N // 2).bit_length() - 1
    case = keyed_case(o, seed, [1 << k for k in range(m)])
    evks = [oracle_galois_key(o, case, 1 << k) for k in range(m)]
    total = oracle_slot_sum(o, case["ct"], evks, N // 2)
    e_sum = np.abs(o.decrypt_decode(total, case["sk"], o.sf_big(0)) - case["vals"].sum()).max()
    wct, wscale = weighted(o, case)
    ip = oracle_slot_sum(o, wct, evks, N // 2)
    e_ip = np.abs(o.decrypt_decode(ip, case["sk"], wscale) - np.dot(case["vals"], case["w"])).max()
    return e_sum, e_ip


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


def dev_automorphism(g, x, gel):
    """x u64[P][nl][N] -> (sigma_g(x), the input buffer)."""
    P, nl = x.shape[:2]
    d_in, d_out = g.to_device(x), g.empty(x.shape)
    g.automorphism(d_in, d_out, P, nl, gel)
    return d_out.to_host(), d_in


@gpu
@pytest.mark.parametrize("name,P", [("tiny", 2), ("n11", 2), ("c1", 2), ("ref", 2), ("c3", 1), ("n17", 1)])
def test_automorphism_is_the_definition_bit_for_bit(ctxs, name, P):
    """Per limb ntt_fwd(sigma_g(ntt_inv(x))) with sigma_g on coefficients; limbs 0 and 1 are one integer-class and one
    fp64-class limb where the ring has both.  g = 1 is the identity; sigma_g then sigma_{g^-1} is the identity; the input
    is not modified; the gather form `src_index` the other tests use is the same permutation."""
    g, o = ctxs(name)
    N, nl = g.N, 2
    rng = np.random.default_rng(500 + N.bit_length())
    x = rand_polys(rng, g, list(range(nl)), P)
    coef = [[o.ntt_inv(l, x[p, l]) for l in range(nl)] for p in range(P)]
    for gel in (5, pow(5, -1, 2 * N), gal(N, N // 4 - 7), 2 * N - 1):
        got, d_in = dev_automorphism(g, x, gel)
        assert np.array_equal(d_in.to_host(), x)
        for p in range(P):
            for l in range(nl):
                want = o.ntt_fwd(l, sigma_coeff(coef[p][l], gel, int(g.moduli[l])))
                assert np.array_equal(got[p, l], want), (name, gel, p, l)
        assert np.array_equal(got, x[:, :, src_index(N, gel)]), (name, gel)
        back, _ = dev_automorphism(g, got, pow(gel, -1, 2 * N))
        assert np.array_equal(back, x), (name, gel)
    assert np.array_equal(dev_automorphism(g, x, 1)[0], x)


@gpu
def test_automorphism_batches_levels_and_neighbours(ctxs):
    """Every level of a ring with 1024-word tiles and of the one-tile ring, more rows than one polynomial, and the words
    around the output stay as they were."""
    POISON = 0xA5A5A5A5A5A5A5A5
    for name in ("tiny", "c1"):
        g, _ = ctxs(name)
        N = g.N
        rng = np.random.default_rng(77)
        for nl in range(1, g.L + 1):
            P, gel = 3, gal(N, nl)
            x = rand_polys(rng, g, list(range(nl)), P)
            words = P * nl * N
            d_big = g.to_device(np.full(words + 4 * N, POISON, dtype=np.uint64))
            d_out = d_big.view(2 * N, (P, nl, N))
            g.automorphism(g.to_device(x), d_out, P, nl, gel)
            assert np.array_equal(d_out.to_host(), x[:, :, src_index(N, gel)]), (name, nl)
            big = d_big.to_host()
            assert np.all(big[:2 * N] == POISON) and np.all(big[2 * N + words:] == POISON)
            g.automorphism(g.to_device(x), d_out, 0, nl, gel)  # empty: nothing written
            assert np.array_equal(d_out.to_host(), x[:, :, src_index(N, gel)])


@gpu
@pytest.mark.parametrize("name", ["tiny", "ref", "c3"])
def test_automorphism_secret_and_galois_keygen_match_the_oracle(ctxs, name):
    g, o = ctxs(name)
    N, D = g.N, g.D
    rng = np.random.default_rng(600 + N.bit_length())
    s, a, e = make_keys(o, rng)
    pk, _ = o.keygen(s, a, e)
    u, e0, e1 = make_rk_rand(o, rng)
    d_s, d_pk = g.to_device(s), g.to_device(pk)
    d_u, d_e0, d_e1 = g.to_device(u), g.to_device(e0), g.to_device(e1)
    for gel in (gal(N, 1), gal(N, -3), 2 * N - 1):
        d_sg = g.empty((N,), np.int8)
        g.automorphism_secret(d_s, d_sg, gel)
        sg = sigma_coeff(s, gel)
        assert np.array_equal(d_sg.to_host(), sg), (name, gel)
        d_evk = g.empty((g.beta, 2, D, N))
        g.galois_keygen(d_s, d_pk, d_u, d_e0, d_e1, gel, d_evk)
        assert np.array_equal(d_evk.to_host(), o.rekeygen(sg, pk, u, e0, e1)), (name, gel)
    assert np.array_equal(d_s.to_host(), s)


ROTATE_CASES = [("c1", 2, 2), ("ref", 4, 2), ("ref", 3, 2), ("ref", 2, 2), ("c5s", 20, 2), ("c5s", 15, 2), ("c3", 12, 1),
                ("c3", 2, 1), ("n17", 4, 1), ("tiny", 5, 2), ("n11", 4, 2)]
_rot = {}


def rotate_case(o, name, nl, B):
    """Uniform random residues, a random key, and the oracle's result; computed once and shared (read-only)."""
    key = (name, nl, B)
    if key not in _rot:
        rng = np.random.default_rng(700 + 31 * nl + B + o.N.bit_length())
        ct, evk = rand_ct(rng, o, nl, B), rand_evks(rng, o, 1)[0]
        gel = gal(o.N, 3 if nl % 2 else -(o.N // 4 - 1))
        want = np.stack([oracle_rotate(o, ct[b], evk, gel) for b in range(B)])
        for arr in (ct, evk, want):
            arr.setflags(write=False)
        _rot[key] = (ct, evk, gel, want)
    return _rot[key]


def dev_rotate(g, ct, evk, gel, nl):
    B = ct.shape[0]
    d_ct, d_out = g.to_device(ct), g.empty(ct.shape)
    g.rotate(d_ct, g.to_device(evk), d_out, B, nl, gel)
    return d_out.to_host(), d_ct


def dev_composition(g, ct, evk, gel, nl):
    """automorphism x 2 + reencrypt, through the public calls."""
    B = ct.shape[0]
    c0, c1 = np.ascontiguousarray(ct[:, 0]), np.ascontiguousarray(ct[:, 1])
    p0, p1 = dev_automorphism(g, c0, gel)[0], dev_automorphism(g, c1, gel)[0]
    d_perm, d_out = g.to_device(np.stack([p0, p1], axis=1)), g.empty(ct.shape)
    g.reencrypt(d_perm, g.to_device(evk), d_out, B, nl)
    return d_out.to_host()


@gpu
@pytest.mark.parametrize("name,nl,B", ROTATE_CASES)
def test_rotate_is_the_reencryption_of_the_permuted_ciphertext(ctxs, name, nl, B):
    g, o = ctxs(name)
    ct, evk, gel, want = rotate_case(o, name, nl, B)
    got, d_ct = dev_rotate(g, ct, evk, gel, nl)
    assert np.array_equal(got, want), (name, nl)
    assert np.array_equal(d_ct.to_host(), ct)
    assert np.array_equal(dev_composition(g, ct, evk, gel, nl), want), (name, nl)


@gpu
@pytest.mark.parametrize("name,nl", [("c3", 12), ("ref", 3)])
@pytest.mark.parametrize("env", [{"MKCKKS_GENERIC_NTT": "1"}, {"MKCKKS_NO_FP64": "1"}, {"MKCKKS_NO_PM": "1"}, {"MKCKKS_CHUNK": "1"}])
def test_rotate_under_the_library_switches(ctxs, monkeypatch, env, name, nl):
    """Switches are read once, when a context is created: a fresh context under each gives the oracle's bits from
    rotate_batch and from the device composition."""
    from ppqsflhe_amd import Context
    _, o = ctxs(name)
    B = 1 if name == "c3" else 2
    ct, evk, gel, want = rotate_case(o, name, nl, B)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    a = CONFIGS[name]
    g = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)
    try:
        assert np.array_equal(dev_rotate(g, ct, evk, gel, nl)[0], want), (name, env)
        assert np.array_equal(dev_composition(g, ct, evk, gel, nl), want), (name, env)
    finally:
        g.close()


@gpu
def test_rotate_across_workspace_chunks(ctxs):
    """More ciphertexts than one workspace chunk (MKCKKS_CHUNK = 16) on the small ring; an empty batch writes nothing."""
    g, o = ctxs("tiny")
    rng = np.random.default_rng(88)
    B, nl = 19, 3
    ct, evk, gel = rand_ct(rng, g, nl, B), rand_evks(rng, o, 1)[0], gal(g.N, 9)
    got, _ = dev_rotate(g, ct, evk, gel, nl)
    for b in range(B):
        assert np.array_equal(got[b], oracle_rotate(o, ct[b], evk, gel)), b
    d_out = g.to_device(got)
    g.rotate(g.to_device(ct), g.to_device(evk), d_out, 0, nl, gel)
    assert np.array_equal(d_out.to_host(), got)


@gpu
@pytest.mark.parametrize("name,spans", [("tiny", (1, 2, 8, 512)), ("c1", (1, 2, 8, 2048)), ("ref", (8192,))])
def test_slot_sum_is_the_loop_of_rotations_and_additions(ctxs, name, spans):
    g, o = ctxs(name)
    N, nl, B = g.N, g.L - 1, 2 if name != "ref" else 1
    assert spans[-1] == N // 2
    rng = np.random.default_rng(800 + N.bit_length())
    m = (N // 2).bit_length() - 1
    ct, evks = rand_ct(rng, g, nl, B), rand_evks(rng, o, m)
    d_ct, d_evks = g.to_device(ct), g.to_device(evks)
    for span in spans:
        d_out = g.empty(ct.shape)
        g.slot_sum(d_ct, d_evks, d_out, B, nl, span)
        got = d_out.to_host()
        if span == 1:
            assert np.array_equal(got, ct)
        for b in range(B):
            assert np.array_equal(got[b], oracle_slot_sum(o, ct[b], evks, span)), (name, span, b)
    assert np.array_equal(d_ct.to_host(), ct)


@gpu
def test_slot_sum_across_workspace_chunks(ctxs, monkeypatch):
    from ppqsflhe_amd import Context
    _, o = ctxs("tiny")
    monkeypatch.setenv("MKCKKS_CHUNK", "2")
    a = CONFIGS["tiny"]
    g = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)
    try:
        rng = np.random.default_rng(89)
        B, nl, span = 3, 4, 4
        ct, evks = rand_ct(rng, g, nl, B), rand_evks(rng, o, 2)
        d_out = g.empty(ct.shape)
        g.slot_sum(g.to_device(ct), g.to_device(evks), d_out, B, nl, span)
        got = d_out.to_host()
        for b in range(B):
            assert np.array_equal(got[b], oracle_slot_sum(o, ct[b], evks, span)), b
    finally:
        g.close()


def dev_galois_key(g, case, d, r, d_evk=None):
    rk = case["rk"][r]
    if d_evk is None:
        d_evk = g.empty((g.beta, 2, g.D, g.N))
    g.galois_keygen(d["s"], d["pk"], g.to_device(rk[0]), g.to_device(rk[1]), g.to_device(rk[2]), g.galois_element(r), d_evk)
    return d_evk


@gpu
@pytest.mark.parametrize("name", ["tiny", "ref"])
def test_decoded_values_of_rotations_and_slot_sums(ctxs, name):
    """Real encode / encrypt under a generated key; Galois keys, rotations, the plaintext product and slot sums on the
    device; decryption and decoding on the oracle."""
    g, o = ctxs(name)
    N, L = g.N, g.L
    m = (N // 2).bit_length() - 1
    rots = (1, -3, N // 4 - 1)
    case = keyed_case(o, 5, sorted(set(rots) | {1 << k for k in range(m)}))
    vals, w, ct, sk = case["vals"], case["w"], case["ct"], case["sk"]
    d = dict(s=g.to_device(case["s"]), pk=g.to_device(case["pk"]))
    d_ct = g.to_device(ct[None])
    base = np.abs(o.decrypt_decode(ct, sk, o.sf_big(0)) - vals).max()
    for r in rots:
        assert g.galois_element(r) == gal(N, r)
        d_evk = dev_galois_key(g, case, d, r)
        assert np.array_equal(d_evk.to_host(), oracle_galois_key(o, case, r)), r
        d_out = g.empty((1, 2, L, N))
        g.rotate(d_ct, d_evk, d_out, 1, L, g.galois_element(r))
        err = np.abs(o.decrypt_decode(d_out.to_host()[0], sk, o.sf_big(0)) - np.roll(vals, -r)).max()
        print(f"{name} rotate {r}: error 2^{np.log2(err):.2f}, unrotated 2^{np.log2(base):.2f}, ratio {err / base:.2f}")
        assert err <= 4 * base, (name, r, err, base)
    d_evks = g.empty((m, g.beta, 2, g.D, N))
    per_key = g.beta * 2 * g.D * N
    for k in range(m):
        dev_galois_key(g, case, d, 1 << k, d_evks.view(k * per_key, (g.beta, 2, g.D, N)))
    d_sum = g.empty((1, 2, L, N))
    g.slot_sum(d_ct, d_evks, d_sum, 1, L, N // 2)
    e_sum = np.abs(o.decrypt_decode(d_sum.to_host()[0], sk, o.sf_big(0)) - vals.sum()).max()
    d_w, d_ip = g.empty((1, 2, L - 1, N)), g.empty((1, 2, L - 1, N))
    g.mult_plain_rescale(d_ct, g.to_device(o.encode(w, o.sf(1), L)[None]), d_w, 1, 1, L)
    wct, wscale = weighted(o, case)
    assert np.array_equal(d_w.to_host()[0], wct)
    g.slot_sum(d_w, d_evks, d_ip, 1, L - 1, N // 2)
    e_ip = np.abs(o.decrypt_decode(d_ip.to_host()[0], sk, wscale) - np.dot(vals, w)).max()
    print(f"{name}: slot sum error 2^{np.log2(e_sum):.2f}, inner product error 2^{np.log2(e_ip):.2f}")
    assert e_sum <= SUM_BOUND[name][0], (name, e_sum)
    assert e_ip <= SUM_BOUND[name][1], (name, e_ip)


if __name__ == "__main__":
    for cfg in ("tiny", "ref"):
        errs = [measure_sums(cfg, seed) for seed in range(6)]
        for seed, (es, ei) in enumerate(errs):
            print(f"{cfg} seed {seed}: slot sum 2^{np.log2(es):.2f}, inner product 2^{np.log2(ei):.2f}")
        print(f"{cfg}: max slot sum 2^{np.log2(max(e[0] for e in errs)):.2f}, max inner product "
              f"2^{np.log2(max(e[1] for e in errs)):.2f}")
