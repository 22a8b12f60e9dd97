"""Per-slot aggregation weights on the GPU: EvalMult(ct, plaintext) fused into the rescale (include/mkckks.h).

mkckks_mult_plain_rescale_batch is DEFINED as the pointwise product of the canonical residues mod q_i on both components
followed by DropLastElementAndScale, so the expected residues are a product formed with Python integers and the oracle's
rescale: bit-exact on every path (the fused row kernels of every ring size, the composition on rings without them and
under the library switches).  The precision test runs real encode / encrypt / eval_sum inputs through the call and
compares the decoded result with the plaintext w * sum(x) and with OpenFHE's order (rescale, then EvalMult).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.oracle import OracleContext, sample_gauss, sample_ternary  # noqa: E402
from tests.test_gpu_parity import CONFIGS, make_keys, rand_ct, rand_polys  # noqa: E402


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


def py_product(g, ct, pt):
    """ct u64[2][nl][N] * pt u64[nl][N] mod q_i with Python integers."""
    out = np.empty_like(ct)
    for i in range(ct.shape[1]):
        q = int(g.moduli[i])
        m = pt[i].astype(object)
        for k in range(2):
            out[k, i] = np.array((ct[k, i].astype(object) * m) % q, dtype=np.uint64)
    return out


def expected(g, o, ct, pt, n_pt):
    """[b] -> Rescale(ct[b] * pt[b % n_pt]) by the definition."""
    return [o.rescale(py_product(g, ct[b], pt[b % n_pt])) for b in range(ct.shape[0])]


def run_fused(g, ct, pt, n_pt, nl):
    B = ct.shape[0]
    d_in, d_pt = g.to_device(ct), g.to_device(pt[:n_pt])
    d_out = g.empty((B, 2, nl - 1, g.N))
    g.mult_plain_rescale(d_in, d_pt, d_out, B, n_pt, nl)
    return d_out.to_host(), d_in


CASES = [("c1", 2, 2),    # 64 x 64 ring, one remaining integer limb, fp64-class dropped limb
         ("ref", 4, 3),   # multi-limb level (64 x 256 ring)
         ("ref", 3, 2),   # reduced levels
         ("ref", 2, 1),
         ("c5s", 20, 1),  # 19 remaining limbs, several of each class
         ("c3", 12, 1),   # 256 x 256 ring
         ("n17", 4, 1),   # 512-point rows
         ("tiny", 5, 2),  # composition path
         ("n11", 4, 1)]   # composition path


@pytest.mark.parametrize("name,nl,B", CASES)
def test_mult_plain_rescale_is_the_definition_bit_for_bit(ctxs, name, nl, B):
    """One plaintext per ciphertext (n_pt = n_ct) and one plaintext for all (n_pt = 1); every ciphertext index."""
    g, o = ctxs(name)
    rng = np.random.default_rng(90 + nl)
    ct = rand_ct(rng, g, nl, B)
    pt = rand_polys(rng, g, list(range(nl)), B)
    prod = {}  # (b, plaintext index) -> expected output, shared by the two forms
    for n_pt in (B, 1):
        got, d_in = run_fused(g, ct, pt, n_pt, nl)
        assert np.array_equal(d_in.to_host(), ct)  # the input is not modified
        for b in range(B):
            key = (b, b % n_pt)
            if key not in prod:
                prod[key] = o.rescale(py_product(g, ct[b], pt[key[1]]))
            assert np.array_equal(got[b], prod[key]), (name, nl, n_pt, b)


@pytest.fixture(scope="module")
def ref_case(ctxs):
    """ref, nl = 4, B = 2: inputs and the definition's outputs for both forms, computed once."""
    g, o = ctxs("ref")
    rng = np.random.default_rng(97)
    nl, B = 4, 2
    ct = rand_ct(rng, g, nl, B)
    pt = rand_polys(rng, g, list(range(nl)), B)
    return nl, B, ct, pt, {n_pt: expected(g, o, ct, pt, n_pt) for n_pt in (B, 1)}


@pytest.mark.parametrize("env", [{"MKCKKS_NO_PM": "1"}, {"MKCKKS_NO_FP64": "1"}, {"MKCKKS_GENERIC_NTT": "1"},
                                 {"MKCKKS_PLAIN_FUSED": "0"}])
def test_library_switches_stay_bit_exact(ref_case, monkeypatch, env):
    """Shoup instead of pseudo-Mersenne arithmetic, integer arithmetic on every limb, the LDS-stage transforms (no fused
    rescale: the composition) and the composition forced on a ring that has the fused kernels.  Switches are read once,
    when a context is created."""
    from ppqsflhe_amd import Context
    nl, B, ct, pt, want = ref_case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a = CONFIGS["ref"]
    g2 = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)
    try:
        for n_pt in (B, 1):
            got, _ = run_fused(g2, ct, pt, n_pt, nl)
            for b in range(B):
                assert np.array_equal(got[b], want[n_pt][b]), (env, n_pt, b)
    finally:
        g2.close()


def test_extreme_residues(ctxs):
    """Every ciphertext and plaintext residue is q_i - 1: the largest product in every limb and arithmetic class."""
    g, o = ctxs("ref")
    nl, B = 4, 1
    ct = np.empty((B, 2, nl, g.N), dtype=np.uint64)
    pt = np.empty((B, nl, g.N), dtype=np.uint64)
    for i in range(nl):
        ct[:, :, i, :] = np.uint64(int(g.moduli[i]) - 1)
        pt[:, i, :] = np.uint64(int(g.moduli[i]) - 1)
    got, _ = run_fused(g, ct, pt, 1, nl)
    assert np.array_equal(got[0], expected(g, o, ct, pt, 1)[0])
    d = g.to_device(ct)
    g.mult_plain(d, g.to_device(pt), B, 1, nl)
    assert np.array_equal(d.to_host()[0], py_product(g, ct[0], pt[0]))  # (q-1)^2 = 1 mod q
    assert np.all(d.to_host() == 1)


@pytest.mark.parametrize("name,nl", [("ref", 4), ("n17", 3), ("tiny", 4)])
def test_identities(ctxs, name, nl):
    """A plaintext of all-one residues gives exactly rescale(in); a plaintext of all-zero residues the rescale of zero."""
    g, o = ctxs(name)
    rng = np.random.default_rng(98)
    B = 2
    ct = rand_ct(rng, g, nl, B)
    d_in = g.to_device(ct)
    d_want = g.empty((B, 2, nl - 1, g.N))
    g.rescale(d_in, d_want, B, nl)
    got, _ = run_fused(g, ct, np.ones((1, nl, g.N), dtype=np.uint64), 1, nl)
    assert np.array_equal(got, d_want.to_host())
    got, _ = run_fused(g, ct, np.zeros((B, nl, g.N), dtype=np.uint64), B, nl)
    zero = o.rescale(np.zeros((2, nl, g.N), dtype=np.uint64))
    for b in range(B):
        assert np.array_equal(got[b], zero)


@pytest.mark.parametrize("name,nl,B", [("ref", 4, 3), ("c1", 2, 2), ("tiny", 5, 2)])
def test_device_consistency(ctxs, name, nl, B):
    """mult_plain on a copy followed by rescale equals mult_plain_rescale; mult_plain equals the Python product; the fused
    call leaves d_in as it was."""
    g, o = ctxs(name)
    rng = np.random.default_rng(99)
    ct = rand_ct(rng, g, nl, B)
    pt = rand_polys(rng, g, list(range(nl)), B)
    for n_pt in (B, 1):
        fused, d_in = run_fused(g, ct, pt, n_pt, nl)
        assert np.array_equal(d_in.to_host(), ct)
        d_copy, d_pt = g.to_device(ct), g.to_device(pt[:n_pt])
        g.mult_plain(d_copy, d_pt, B, n_pt, nl)
        prod = d_copy.to_host()
        for b in range(B):
            assert np.array_equal(prod[b], py_product(g, ct[b], pt[b % n_pt])), (n_pt, b)
        d_out = g.empty((B, 2, nl - 1, g.N))
        g.rescale(d_copy, d_out, B, nl)
        assert np.array_equal(d_out.to_host(), fused)


def test_arguments_are_checked_and_empty_batches_are_noops(ctxs):
    from ppqsflhe_amd import MkckksError
    g, _ = ctxs("tiny")
    nl, B = g.L, 3
    d_ct, d_pt, d_out = g.empty((B, 2, nl, g.N)), g.empty((B, nl, g.N)), g.empty((B, 2, nl - 1, g.N))

    def refused(call):
        with pytest.raises(MkckksError) as ei:
            call()
        assert ei.value.code == -1

    refused(lambda: g.mult_plain(d_ct, d_pt, B, 2, nl))                      # n_pt neither 1 nor n_ct
    refused(lambda: g.mult_plain_rescale(d_ct, d_pt, d_out, B, 2, nl))
    refused(lambda: g.mult_plain_rescale(d_ct, d_pt, d_out, B, B, 1))        # nothing left after the rescale
    refused(lambda: g.mult_plain_rescale(d_ct, d_pt, d_out, B, B, nl + 1))
    refused(lambda: g.mult_plain(d_ct, d_pt, B, B, nl + 1))
    refused(lambda: g.mult_plain_rescale(d_ct, d_pt, d_ct, B, B, nl))        # output over the input
    refused(lambda: g.mult_plain_rescale(d_ct, d_pt, d_ct.ptr + 8 * g.N, B, B, nl))
    g.mult_plain(d_ct, d_pt, 0, 0, nl)
    g.mult_plain_rescale(d_ct, d_pt, d_out, 0, 1, nl)
    g.sync()


# ---- precision: the reference's parameters, real inputs ----------------------------------------------------------------

def test_per_slot_weights_precision_against_the_openfhe_order(ctxs):
    """Three clients under one key, values in [-1, 1], per-slot factors in [0, 1] (0, 1, 0.5 and 1/3 among them).  New order
    (multiply by the plaintext at sf(1), ONE rescale) against OpenFHE's (rescale, then multiply by an (nl-1)-limb
    plaintext), both on the device and decoded with the same scale.  Required: err_new < 2^-25 (the project's bar for
    decoded doubles at these parameters) and err_new < err_other.

    Measured on an MI355X (profiles/slot_weights_ab.txt): err_new 2^-32.28, err_other 2^-26.31; the CPU oracle gives
    2^-31.97 (multiply first) against 2^-26.13 (rescale first) at these parameters."""
    g, o = ctxs("ref")
    rng = np.random.default_rng(43)
    N, L, slots, C = g.N, g.L, g.N // 2, 3
    x = rng.uniform(-1.0, 1.0, size=(C, slots))
    w = rng.uniform(0.0, 1.0, size=slots)
    w[:4] = [0.0, 1.0, 0.5, 1.0 / 3.0]
    want = w * x.sum(axis=0)
    s, a, e = make_keys(o, rng)
    pk, sk = o.keygen(s, a, e)
    d_pk, d_sk = g.to_device(pk), g.to_device(sk)
    d_pts = g.empty((C, L, N))
    g.encode(g.to_device(x), d_pts, C, L, o.sf_big(0))
    v = np.stack([sample_ternary(rng, N) for _ in range(C)])
    e0 = np.stack([sample_gauss(rng, N) for _ in range(C)])
    e1 = np.stack([sample_gauss(rng, N) for _ in range(C)])
    d_cts = g.empty((C, 2, L, N))
    g.encrypt(d_pk, d_pts, g.to_device(v), g.to_device(e0), g.to_device(e1), d_cts, C, L)
    d_sum = g.empty((1, 2, L, N))
    g.eval_sum(d_cts, d_sum, C, 1, L)
    d_w = g.empty((1, L, N))
    g.encode(g.to_device(w[None]), d_w, 1, L, o.sf(1))
    scale = o.sf_big(0) / float(o.moduli[L - 1]) * o.sf(1)
    d_m, d_vals = g.empty((1, L - 1, N)), g.empty((1, slots), dtype=np.float64)

    def decoded(d_ct):
        g.decrypt(d_ct, d_sk, d_m, 1, L - 1)
        g.decode(d_m, d_vals, 1, L - 1, scale)
        return d_vals.to_host()[0]

    d_new = g.empty((1, 2, L - 1, N))
    g.mult_plain_rescale(d_sum, d_w, d_new, 1, 1, L)
    err_new = np.abs(decoded(d_new) - want).max()
    # the other order: rescale, then the product with a plaintext of L - 1 limbs
    d_other = g.empty((1, 2, L - 1, N))
    g.rescale(d_sum, d_other, 1, L)
    d_w1 = g.empty((1, L - 1, N))
    g.encode(g.to_device(w[None]), d_w1, 1, L - 1, o.sf(1))
    g.mult_plain(d_other, d_w1, 1, 1, L - 1)
    err_other = np.abs(decoded(d_other) - want).max()
    print(f"per-slot weights, ref context, 3 clients: err_new 2^{np.log2(err_new):.2f}, err_other 2^{np.log2(err_other):.2f}")
    assert err_new < 2.0 ** -25, (err_new, err_other)
    assert err_new < err_other, (err_new, err_other)
