"""Polynomial evaluation on the device (include/mkckks.h: "polynomial evaluation"; DESIGN.md "polynomial evaluation").

    powers:      z^k = rescale(mult_relin(z^i, prefix(z^j, nl_i))), i = ceil(k / 2), j = k - i
    poly_tensor: (d0, d1, d2) = sum_{j>=1} [Q_j (x) g_j + M_{j,0} (g_j, 0)] + (Q_0, 0) + (M_{0,0}, 0, 0), Q_j = sum_{i>=1} M_{j,i} b_i
    poly_eval:   powers of x up to y = x^B, powers of y, poly_weights, poly_tensor, relinearize, rescale, rescale

The oracle has no product, so expectations are built as tests/test_product.py builds them: tensor products and constant
products are Python integer arithmetic per limb (py_tensor, py_poly_tensor), relinearisation is oracle_relinearize, the
rescale is the oracle's; plan, scales and weights are the Python restatements of tests/test_poly_surface.py.  Device
results are compared word for word.

Decoded values: `measure_poly(name, degree, seed)` runs encrypt -> rescale -> that CPU chain -> decrypt -> decode and returns
max |decoded - numpy polyval| over the slots, inputs uniform in [-1, 1], coefficients the Taylor coefficients of tanh
(TANH: fixed numbers below; degree 3 on "tiny", 7 and 15 on "c5s").  POLY_BOUND is 4 x the largest error over the seeds
(run `python -m tests.test_poly` to print them): the margin test_product.py and test_rotation.py use for the seed-to-seed
spread of a slot maximum.  Nothing in a bound comes from a GPU result.
Measured on the CPU chain, seeds 0 .. 5:
    tiny d = 3:   2^-30.32 .. 2^-29.25
    c5s  d = 7:   2^-37.81 .. 2^-37.56
    c5s  d = 15:  2^-38.00 .. 2^-37.37"""
import numpy as np
import pytest

from oracle.oracle import FastCpuContext, sample_gauss, sample_ternary
from tests.test_gpu_parity import CONFIGS, make_keys, make_rk_rand, rand_ct
from tests.test_poly_surface import py_constants, py_ladder, py_plan, py_weights
from tests.test_product import POISON, oracle_relin_key, oracle_relinearize, py_tensor, with_edges
from tests.test_rotation import rand_evks

gpu = pytest.mark.gpu

TANH = [0.0, 1.0, 0.0, -1.0 / 3, 0.0, 2.0 / 15, 0.0, -17.0 / 315, 0.0, 62.0 / 2835, 0.0, -1382.0 / 155925, 0.0,
        21844.0 / 6081075, 0.0, -929569.0 / 638512875]
# 4 x the largest of measure_poly(name, degree, seed) over seeds 0 .. 5
POLY_BOUND = {("tiny", 3): 4 * 2.0 ** -29.25, ("c5s", 7): 4 * 2.0 ** -37.56, ("c5s", 15): 4 * 2.0 ** -37.37}


# ---- the definitions in Python integers --------------------------------------------------------------------------------

def py_poly_tensor(moduli, babies, giants, M, nl_T):
    """babies[i - 1] = x^i u64[2][nl_i][N], giants[j - 1] = y^j, M[j][i] Python integers -> u64[3][nl_T][N], exact."""
    N = babies[0].shape[-1]
    out = np.empty((3, nl_T, N), dtype=np.uint64)
    G, B = len(M), len(M[0])
    for t in range(nl_T):
        q = int(moduli[t])
        b = [(x[0, t].astype(object), x[1, t].astype(object)) for x in babies]
        d = [np.zeros(N, dtype=object) for _ in range(3)]
        for j in range(G):
            Q0 = sum((M[j][i] % q) * b[i - 1][0] for i in range(1, B))
            Q1 = sum((M[j][i] % q) * b[i - 1][1] for i in range(1, B))
            if j == 0:
                d[0] = d[0] + Q0 + M[0][0]
                d[1] = d[1] + Q1
                continue
            g0, g1 = giants[j - 1][0, t].astype(object), giants[j - 1][1, t].astype(object)
            d[0] = d[0] + Q0 * g0 + M[j][0] * g0
            d[1] = d[1] + Q0 * g1 + Q1 * g0 + M[j][0] * g1
            d[2] = d[2] + Q1 * g1
        for k in range(3):
            out[k, t] = np.array(d[k] % q, dtype=np.uint64)
    return out


def cpu_ladder(o, z, rlk, n_pow):
    """[z^1 .. z^n_pow] on the CPU: py_tensor on the level cut, oracle_relinearize, the oracle's rescale."""
    pw = {1: z}
    for k in range(2, n_pow + 1):
        i = (k + 1) // 2
        j = k - i
        nli = pw[i].shape[1]
        a, b = pw[i], np.ascontiguousarray(pw[j][:, :nli])
        pw[k] = o.rescale(oracle_relinearize(o, py_tensor(o.moduli[:nli], a[None], b[None]), rlk))
    return [pw[k] for k in range(1, n_pow + 1)]


def cpu_poly_eval(o, ct, rlk, coef, scale):
    """The whole algorithm on the CPU for one ciphertext u64[2][nl][N]; returns (u64[2][nl_out][N], S_out)."""
    nl = ct.shape[1]
    p = py_plan(len(coef) - 1, nl)
    w, s_out = py_weights(o.moduli, o.L, o.sf, coef, nl, scale)
    xs = cpu_ladder(o, ct, rlk, p["B"])
    ys = cpu_ladder(o, xs[-1], rlk, p["G"] - 1)
    d3 = py_poly_tensor(o.moduli, xs[:-1], ys, py_constants(w), p["nl_T"])
    return o.rescale(o.rescale(oracle_relinearize(o, d3, rlk))), s_out


# ---- decoded values on the CPU chain: where POLY_BOUND comes from -----------------------------------------------------------

def poly_case(o, seed):
    rng = np.random.default_rng(seed)
    N, L = o.N, o.L
    s, a, e = make_keys(o, rng)
    pk, sk = o.keygen(s, a, e)
    v = rng.uniform(-1.0, 1.0, size=N // 2)
    ct = o.encrypt(pk, o.encode(v, o.sf_big(0), L), sample_ternary(rng, N), sample_gauss(rng, N), sample_gauss(rng, N))
    return dict(s=s, pk=pk, sk=sk, v=v, ct=ct, rlk_rand=make_rk_rand(o, rng),
                scale=o.sf_big(0) / float(int(o.moduli[L - 1])))  # of the rescaled fresh ciphertext, on L - 1 limbs


def poly_error(o, case, coef, out, s_out):
    want = np.polyval(list(coef)[::-1], case["v"])
    return np.abs(o.decrypt_decode(out, case["sk"], s_out) - want).max()


def measure_poly(name, degree, seed):
    c = CONFIGS[name]
    o = FastCpuContext(c[0], c[1], c[2], c[3], dnum=c[4])
    case = poly_case(o, seed)
    rlk = oracle_relin_key(o, case["sk"], case["pk"], *case["rlk_rand"])
    coef = TANH[:degree + 1]
    out, s_out = cpu_poly_eval(o, o.rescale(case["ct"]), rlk, coef, case["scale"])
    return poly_error(o, case, coef, out, s_out)


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


def pack(arrs):
    return np.concatenate([a.reshape(-1) for a in arrs])


def tensor_weights(rng, moduli, nl_T, B, G, p_bits, table):
    """G x B weights below a quarter of the level's modulus: random magnitudes over the whole range, negative values,
    zeros, a half (rint rounds to even), values of about 2^(3p) where the modulus holds them (else just under the cap) in
    the constant term and the constant column, and one below 0.5 (M = 0).
    A 2 x 2 table has a single baby column, which must stay live (a zero there would make every Q_j vanish), so the kinds
    are spread over two tables that keep M_{0,1} and M_{1,1} non-zero: table 0 holds the negative 2^(3p) constant term and
    the 0.3, table 1 the exact zero, the half and the positive 2^(3p) column entry."""
    cap = sum(int(m).bit_length() - 1 for m in moduli[:nl_T]) - 2  # log2 of the bound, rounded down
    big = 2.0 ** min(3 * p_bits, cap)
    w = rng.uniform(0.5, 1.0, size=(G, B)) * 2.0 ** rng.integers(1, cap, size=(G, B)) * rng.choice([-1.0, 1.0], size=(G, B))
    if (B, G) == (2, 2):
        if table == 0:
            w[0, 0], w[1, 0], w[1, 1] = -big * 0.75, 0.3, -abs(w[1, 1])
        else:
            w[0, 0], w[1, 0], w[0, 1] = 0.0, big * 0.625, -12345.5  # a tie: rounds to the even -12346
        return w
    assert table == 0
    w[0, 0] = -big * 0.75  # the constant term
    w[G - 1, 0] = big * 0.625  # a constant-column entry
    w[0, 1] = 0.0
    w[1, 1] = -12345.5  # a tie: rounds to the even -12346
    w[G - 1, B - 1] = 0.3
    w[1, 2] = 2.0 ** 53 + 2.0  # an integer a double holds exactly, above the rint range
    w[0, 2] = 0.0
    return w


_tensor = {}


def tensor_case(g, name, nl_T, B, G, n_ct, extra, table=0):
    """Operands with the edge residues at nl_T + extra[..] limbs, the weights and the integer definition; computed once and
    shared (read-only)."""
    key = (name, nl_T, B, G, n_ct, extra, table)
    if key not in _tensor:
        rng = np.random.default_rng(1500 + 97 * nl_T + 7 * B + G + g.N.bit_length() + 1000 * table)
        baby_nl = [nl_T + extra[(i - 1) % len(extra)] for i in range(1, B)]
        giant_nl = [nl_T + extra[j % len(extra)] for j in range(1, G)]
        babies = [with_edges(rand_ct(rng, g, nl, n_ct), g.moduli) for nl in baby_nl]
        giants = [with_edges(rand_ct(rng, g, nl, n_ct), g.moduli) for nl in giant_nl]
        w = tensor_weights(rng, g.moduli, nl_T, B, G, CONFIGS[name][2], table)
        M = py_constants(w)
        # the inner sums are live in the first row and in a giant's row: no case reduces to constants times giants
        assert any(M[0][i] for i in range(1, B)) and any(M[j][i] for j in range(1, G) for i in range(1, B)), M
        want = np.stack([py_poly_tensor(g.moduli, [x[b] for x in babies], [y[b] for y in giants], M, nl_T) for b in range(n_ct)])
        assert want[:, 2].any()  # d2 = sum Q_j1 g_j1 is not identically zero
        for arr in babies + giants + [w, want]:
            arr.setflags(write=False)
        _tensor[key] = (babies, baby_nl, giants, giant_nl, w, want)
    return _tensor[key]


def dev_poly_tensor(g, case, n_ct, nl_T):
    """poly_tensor into a buffer pre-filled with POISON; the words around the output are checked unchanged."""
    babies, baby_nl, giants, giant_nl, w, _ = case
    N = g.N
    words = n_ct * 3 * nl_T * N
    d_big = g.to_device(np.full(words + 4 * N, POISON, dtype=np.uint64))
    d_out = d_big.view(2 * N, (n_ct, 3, nl_T, N))
    hb, hg = pack(babies), pack(giants)
    d_b, d_g = g.to_device(hb), g.to_device(hg)
    g.poly_tensor(d_b, baby_nl, d_g, giant_nl, w, d_out, n_ct, nl_T)
    big = d_big.to_host()
    assert np.all(big[:2 * N] == POISON) and np.all(big[2 * N + words:] == POISON)
    assert np.array_equal(d_b.to_host(), hb) and np.array_equal(d_g.to_host(), hg)
    return d_out.to_host()


# (name, nl_T, B, G, ciphertexts, limbs of the operands above nl_T, weight table).  B = G = 2 has one baby and one giant: the
# two c3 rows together put the operands at 8, 9, 10 and 11 limbs above the 7 of the outer sum
TENSOR_CASES = [("n11", 3, 2, 2, 1, (0,), 0), ("n11", 3, 2, 2, 1, (0,), 1),
                ("tiny", 1, 4, 3, 2, (1, 2), 0), ("tiny", 2, 4, 3, 2, (1, 2), 0), ("tiny", 3, 4, 3, 2, (1, 2), 0),
                ("ref", 3, 8, 8, 1, (0,), 0), ("c3", 7, 2, 2, 1, (1, 2), 0), ("c3", 7, 2, 2, 1, (3, 4), 1)]


@gpu
@pytest.mark.parametrize("name,nl_T,B,G,n_ct,extra,table", TENSOR_CASES)
def test_poly_tensor_is_the_integer_definition(ctxs, name, nl_T, B, G, n_ct, extra, table):
    g, _ = ctxs(name)
    case = tensor_case(g, name, nl_T, B, G, n_ct, extra, table)
    assert np.array_equal(dev_poly_tensor(g, case, n_ct, nl_T), case[-1]), (name, nl_T, B, G, table)


@gpu
@pytest.mark.parametrize("name,nl_T,B,G,extra,table", [("ref", 3, 4, 4, (0,), 0), ("c3", 7, 2, 2, (1, 2), 0), ("c3", 7, 2, 2, (3, 4), 1)])
@pytest.mark.parametrize("env", [{"MKCKKS_POLY_FUSED": "0"}, {"MKCKKS_POLY_FUSED": "1"}, {"MKCKKS_NO_FP64": "1"},
                                 {"MKCKKS_NO_PM": "1"}, {"MKCKKS_CHUNK": "1"}, {"MKCKKS_POLY_FUSED": "0", "MKCKKS_NO_FP64": "1"}])
def test_poly_tensor_under_the_library_switches(ctxs, monkeypatch, env, name, nl_T, B, G, extra, table):
    """Switches are read once, when a context is created: a fresh context under each gives the bits of the definition,
    the composition (MKCKKS_POLY_FUSED=0) included."""
    from ppqsflhe_amd import Context
    g0, _ = ctxs(name)
    case = tensor_case(g0, name, nl_T, B, G, 1, extra, table)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    c = CONFIGS[name]
    g = Context(c[0], c[1], c[2], c[3], dnum=c[4], device=0)
    try:
        assert np.array_equal(dev_poly_tensor(g, case, 1, nl_T), case[-1]), (name, env)
    finally:
        g.close()


def dev_ladder_by_hand(g, z, d_rlk, n_ct, nl, n_pow):
    """The loop the header states: packed prefix copy + mult_relin + rescale, every step a call of its own."""
    pw = {1: z}
    for k in range(2, n_pow + 1):
        i = (k + 1) // 2
        j = k - i
        nli = pw[i].shape[2]
        d_a = g.to_device(pw[i])
        d_b = d_a if i == j else g.to_device(np.ascontiguousarray(pw[j][:, :, :nli]))
        d_p, d_r = g.empty((n_ct, 2, nli, g.N)), g.empty((n_ct, 2, nli - 1, g.N))
        g.mult_relin(d_a, d_b, d_rlk, d_p, n_ct, nli)
        g.rescale(d_p, d_r, n_ct, nli)
        pw[k] = d_r.to_host()
    return [pw[k] for k in range(1, n_pow + 1)]


def split_powers(flat, nls, n_ct, N):
    out, off = [], 0
    for nl in nls:
        words = n_ct * 2 * nl * N
        out.append(flat[off:off + words].reshape(n_ct, 2, nl, N))
        off += words
    assert off == flat.size
    return out


@gpu
@pytest.mark.parametrize("name,nl,n_pow", [("tiny", 4, 3), ("c5s", 12, 8)])
def test_powers_are_the_loop_of_products_and_rescales(ctxs, name, nl, n_pow):
    g, o = ctxs(name)
    N, n_ct = g.N, 2
    rng = np.random.default_rng(1600 + nl)
    z = rand_ct(rng, g, nl, n_ct)
    rlk = rand_evks(rng, o, 1)[0]
    d_z, d_rlk = g.to_device(z), g.to_device(rlk)
    scale = g.sf(g.L - nl)
    want_nl, want_s = py_ladder(g.moduli, nl, n_pow, scale)
    assert want_nl == [nl - (k - 1).bit_length() for k in range(1, n_pow + 1)]
    words = n_ct * 2 * N * sum(want_nl)
    d_big = g.to_device(np.full(words + 4 * N, POISON, dtype=np.uint64))
    d_out = d_big.view(2 * N, (words,))
    nls, scales = g.powers(d_z, d_rlk, d_out, n_ct, nl, n_pow, scale)
    assert nls == want_nl
    assert scales == want_s  # the same three double operations in the same order: equal to the last bit
    big = d_big.to_host()
    assert np.all(big[:2 * N] == POISON) and np.all(big[2 * N + words:] == POISON)
    assert np.array_equal(d_z.to_host(), z)
    got = split_powers(d_out.to_host(), nls, n_ct, N)
    want = dev_ladder_by_hand(g, z, d_rlk, n_ct, nl, n_pow)
    for k in range(n_pow):
        assert np.array_equal(got[k], want[k]), (name, k + 1)


def dev_eval_by_hand(g, ct, d_rlk, coef, n_ct, nl, scale):
    """powers on x (n_pow = B), powers on y (n_pow = G - 1), poly_weights, poly_tensor, relinearize, rescale twice."""
    N = g.N
    p = g.poly_plan(len(coef) - 1, nl)
    B, G, nl_T = p["B"], p["G"], p["nl_T"]
    nlx, _ = py_ladder(g.moduli, nl, B, scale)
    d_x = g.empty((n_ct * 2 * N * sum(nlx),))
    nls, sx = g.powers(g.to_device(ct), d_rlk, d_x, n_ct, nl, B, scale)
    assert nls == nlx == p["baby_nl"] + [nlx[-1]]
    off_y = n_ct * 2 * N * sum(nlx[:-1])
    d_y = d_x.view(off_y, (n_ct, 2, nlx[-1], N))
    nly, _ = py_ladder(g.moduli, nlx[-1], G - 1, sx[-1])
    d_g = g.empty((n_ct * 2 * N * sum(nly),))
    nls, _ = g.powers(d_y, d_rlk, d_g, n_ct, nlx[-1], G - 1, sx[-1])
    assert nls == nly == p["giant_nl"]
    w, s_out = g.poly_weights(coef, nl, scale)
    d_3 = g.empty((n_ct, 3, nl_T, N))
    g.poly_tensor(d_x, p["baby_nl"], d_g, p["giant_nl"], w, d_3, n_ct, nl_T)
    d_r = g.empty((n_ct, 2, nl_T, N))
    g.relinearize(d_3, d_rlk, d_r, n_ct, nl_T)
    d_1, d_0 = g.empty((n_ct, 2, nl_T - 1, N)), g.empty((n_ct, 2, nl_T - 2, N))
    g.rescale(d_r, d_1, n_ct, nl_T)
    g.rescale(d_1, d_0, n_ct, nl_T - 1)
    return d_0.to_host(), s_out


def check_eval(g, o, name, degree, nl, n_ct, against_cpu=False):
    N = g.N
    rng = np.random.default_rng(1700 + 13 * degree + nl)
    ct = rand_ct(rng, g, nl, n_ct)
    rlk = rand_evks(rng, o, 1)[0]
    coef = rng.uniform(-1, 1, size=degree + 1)
    coef[1] = 0.0
    scale = g.sf(g.L - nl)
    p = g.poly_plan(degree, nl)
    d_ct, d_rlk = g.to_device(ct), g.to_device(rlk)
    words = n_ct * 2 * p["nl_out"] * N
    d_big = g.to_device(np.full(words + 4 * N, POISON, dtype=np.uint64))
    d_out = d_big.view(2 * N, (n_ct, 2, p["nl_out"], N))
    s_out = g.poly_eval(d_ct, d_rlk, coef, d_out, n_ct, nl, scale)
    big = d_big.to_host()
    assert np.all(big[:2 * N] == POISON) and np.all(big[2 * N + words:] == POISON)
    assert np.array_equal(d_ct.to_host(), ct)
    want, want_s = dev_eval_by_hand(g, ct, d_rlk, coef, n_ct, nl, scale)
    assert s_out == want_s == g.sf(g.L - p["nl_out"])
    got = d_out.to_host()
    assert np.array_equal(got, want), (name, degree)
    if against_cpu:
        cpu, cpu_s = cpu_poly_eval(o, ct[0], rlk, coef, scale)
        assert cpu_s == s_out and np.array_equal(got[0], cpu), (name, degree, "CPU chain")


@gpu
@pytest.mark.parametrize("name,degree,nl", [("tiny", 3, 4)] + [("c5s", d, 12) for d in (2, 7, 15, 31, 63)])
def test_poly_eval_is_its_composition(ctxs, name, degree, nl):
    g, o = ctxs(name)
    check_eval(g, o, name, degree, nl, 2, against_cpu=name == "tiny")


@gpu
def test_poly_eval_across_workspace_chunks(ctxs, monkeypatch):
    """MKCKKS_CHUNK = 1, 3 ciphertexts, in a fresh context: every chunk reuses the engine's buffers."""
    from ppqsflhe_amd import Context
    _, o = ctxs("c5s")
    monkeypatch.setenv("MKCKKS_CHUNK", "1")
    c = CONFIGS["c5s"]
    g = Context(c[0], c[1], c[2], c[3], dnum=c[4], device=0)
    try:
        check_eval(g, o, "c5s", 15, 12, 3)
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("name,degree", [("tiny", 3), ("c5s", 7), ("c5s", 15)])
def test_decoded_values_of_an_encrypted_polynomial(ctxs, name, degree):
    """Real encode / encrypt under a generated key; the relinearisation key, the rescale and the evaluation on the device;
    decryption and decoding on the oracle."""
    g, o = ctxs(name)
    N, L, D = g.N, g.L, g.D
    case = poly_case(o, 5)
    d_rlk = g.empty((g.beta, 2, D, N))
    g.relin_keygen(g.to_device(case["s"]), g.to_device(case["pk"]), *[g.to_device(x) for x in case["rlk_rand"]], d_rlk)
    d_x = g.empty((1, 2, L - 1, N))
    g.rescale(g.to_device(case["ct"][None]), d_x, 1, L)
    coef = TANH[:degree + 1]
    p = g.poly_plan(degree, L - 1)
    d_out = g.empty((1, 2, p["nl_out"], N))
    s_out = g.poly_eval(d_x, d_rlk, coef, d_out, 1, L - 1, case["scale"])
    err = poly_error(o, case, coef, d_out.to_host()[0], s_out)
    print(f"{name} degree {degree}: error 2^{np.log2(err):.2f}, bound 2^{np.log2(POLY_BOUND[(name, degree)]):.2f}")
    assert err <= POLY_BOUND[(name, degree)], (name, degree, err)


@gpu
def test_poly_refusals_on_a_device_context(ctxs):
    from ppqsflhe_amd.binding import MkckksError
    g, _ = ctxs("tiny")
    N, nl = g.N, 4
    p = g.poly_plan(3, nl)
    nl_T = p["nl_T"]
    scale = g.sf(g.L - nl)
    w, _ = g.poly_weights([0.5, 1.0, 0.0, -1.0 / 3], nl, scale)
    d_b, d_g = g.empty((1, 2, p["baby_nl"][0], N)), g.empty((1, 2, p["giant_nl"][0], N))
    d_out = g.empty((2, 3, nl_T, N))
    d_rlk = g.empty((g.beta, 2, g.D, N))

    def refused(call, text):
        with pytest.raises(MkckksError) as e:
            call()
        assert e.value.code == -1 and text in str(e.value), (text, str(e.value))

    tensor = lambda b, gi, o, ww=w: g.poly_tensor(b, p["baby_nl"], gi, p["giant_nl"], ww, o, 1, nl_T)
    refused(lambda: tensor(d_b, d_g, d_b), "overlaps")                                  # d_out3 is an input
    refused(lambda: tensor(d_b, d_out.view(N, (1, 2, p["giant_nl"][0], N)), d_out), "overlaps")  # a giant inside d_out3
    refused(lambda: tensor(d_b, d_g, d_out.view(1, (1, 3, nl_T, N))), "16-byte aligned")  # an odd word offset
    refused(lambda: tensor(d_b.view(1, (1,)), d_g, d_out), "16-byte aligned")
    half_q = 0.5
    for m in g.moduli[:nl_T]:
        half_q *= float(int(m))
    big = w.copy()
    big[0, 0] = half_q * 1.001
    refused(lambda: tensor(d_b, d_g, d_out, big), "does not fit")                       # |w| beyond the modulus bound
    big[0, 0] = np.inf
    refused(lambda: tensor(d_b, d_g, d_out, big), "not finite")
    refused(lambda: g.poly_tensor(d_b, [nl_T - 1], d_g, p["giant_nl"], w, d_out, 1, nl_T), "limb count")
    d_ct, d_res = g.empty((1, 2, nl, N)), g.empty((1, 2, p["nl_out"], N))
    refused(lambda: g.poly_eval(d_ct, d_rlk, [1.0, 0.5, 0.25, 0.125], d_res, 1, 3, g.sf(g.L - 3)), "needs 4 limbs")  # nl_out < 1
    refused(lambda: g.poly_eval(d_ct, d_rlk, [1.0, 0.5, 0.25, 0.125], d_ct, 1, nl, scale), "overlaps")
    refused(lambda: g.poly_eval(d_ct, d_rlk, [1.0, 0.5, 0.25, 0.125], d_res.view(1, (1,)), 1, nl, scale), "16-byte aligned")
    refused(lambda: g.powers(d_ct, d_rlk, d_ct, 1, nl, 3, scale), "overlaps")
    refused(lambda: g.powers(d_ct, d_rlk, d_out, 1, nl, 9, scale), "power ladder")     # 4 - ceil(log2 9) < 1
    g.poly_eval(d_ct, d_rlk, [1.0, 0.5, 0.25, 0.125], d_res, 0, nl, scale)             # zero count: a no-op


if __name__ == "__main__":
    for cfg, degree, seeds in (("tiny", 3, range(6)), ("c5s", 7, range(6)), ("c5s", 15, range(6))):
        errs = [measure_poly(cfg, degree, seed) for seed in seeds]
        for seed, e in zip(seeds, errs):
            print(f"{cfg} degree {degree} seed {seed}: 2^{np.log2(e):.2f}")
        print(f"{cfg} degree {degree}: 2^{np.log2(min(errs)):.2f} .. 2^{np.log2(max(errs)):.2f}")
