"""Chebyshev series on the device (include/mkckks.h: "Chebyshev series"; DESIGN.md "Chebyshev series").

    cheb_tensor: (d0, d1, d2) = (2 a0 b0 - M t0, 2 (a0 b1 + a1 b0) - M t1, 2 a1 b1), M = rint(w); t absent: (1, 0)
    cheb_ladder: T_k = rescale(relinearize(cheb_tensor(T_i, T_j, T_{i-j}; S_i S_j / S_{i-j}))), i = ceil(k / 2), j = k - i
    affine:      out = M_a in + (M_c, 0)
    cheb_eval:   affine + rescale (unless [-1, 1]), the ladder on u to T_B, the ladder on T_B, cheb_weights, poly_tensor,
                 relinearize, rescale, rescale

The oracle has no product, so expectations are built as tests/test_poly.py builds them: the ladder step and the affine map
are Python integer arithmetic per limb (py_cheb_tensor, py_affine), the outer sum is py_poly_tensor, relinearisation is
oracle_relinearize, the rescale is the oracle's; plan, scales and weights are the Python restatements of
tests/test_poly_surface.py and tests/test_cheb_surface.py.  Device results are compared word for word.

Decoded values: `measure_cheb(name, key, seed)` runs encrypt -> rescale -> that CPU chain -> decrypt -> decode and returns
max |decoded - chebval| over the slots, inputs uniform in [a, b], the expectation being the FITTED series' value (the fit
error is not in the bound).  Coefficients: numpy.polynomial.chebyshev.chebinterpolate of tanh on [-1, 1] (degrees 3 and
15) and of 1 / sqrt(t) on [0.25, 4] (degree 31), fixed numbers below.  CHEB_BOUND is 4 x the largest error over seeds
0 .. 5 (run `python -m tests.test_cheb` to print them): the margin test_poly.py and test_product.py use for the
seed-to-seed spread of a slot maximum.  Nothing in a bound comes from a GPU result.
Measured on the CPU chain, seeds 0 .. 5:
    tiny tanh d = 3 on [-1, 1]:       2^-30.36 .. 2^-29.73
    c5s  tanh d = 15 on [-1, 1]:      2^-37.80 .. 2^-37.20
    c5s  invsqrt d = 31 on [0.25, 4]: 2^-36.32 .. 2^-35.82"""
import numpy as np
import pytest
from numpy.polynomial import chebyshev as npcheb

from oracle.oracle import FastCpuContext, sample_gauss, sample_ternary
from tests.test_cheb_surface import py_cheb_weights
from tests.test_gpu_parity import CONFIGS, make_keys, make_rk_rand, rand_ct
from tests.test_poly import py_poly_tensor, split_powers
from tests.test_poly_surface import py_constants, py_ladder, py_plan
from tests.test_product import POISON, oracle_relin_key, oracle_relinearize, with_edges
from tests.test_rotation import rand_evks

gpu = pytest.mark.gpu

TANH3 = [0.0, 0.8120256702143022, 0.0, -0.05875964592213401]
TANH15 = [0.0, 0.811675685131559, 1.3877787807814457e-17, -0.05424581032626491, -1.3877787807814457e-17,
          0.004516821992838205, 0.0, -0.0003824471706602717, 1.3877787807814457e-17, 3.2443949467581e-05,
          1.3877787807814457e-17, -2.7529621762691775e-06, 0.0, 2.3374445835876514e-07, 0.0, -2.150440383667004e-08]
INVSQRT31 = [0.8916515899871222, -0.5647588258978908, 0.25897894358762014, -0.1307598555001495, 0.06906275955198984,
             -0.03744656126389159, 0.020656716910329387, -0.011534655850624707, 0.006499717277255859, -0.003688426009551035,
             0.0021048730250639927, -0.0012067055375182614, 0.0006944369251111054, -0.0004009256545001172,
             0.00023210970776785939, -0.0001346978199891491, 7.83312977724604e-05, -4.5636294144023315e-05,
             2.6631549518540965e-05, -1.5563895403747363e-05, 9.10776491386961e-06, -5.336066296560138e-06,
             3.129652783144532e-06, -1.837326992173982e-06, 1.0795179993111637e-06, -6.346280523039649e-07,
             3.730865042461673e-07, -2.1900349811421194e-07, 1.2782327291072093e-07, -7.326460288448189e-08,
             3.965062297939248e-08, -1.7352159598083006e-08]
# key -> (configuration, coefficients, a, b)
DECODED = {"tanh3": ("tiny", TANH3, -1.0, 1.0), "tanh15": ("c5s", TANH15, -1.0, 1.0), "invsqrt31": ("c5s", INVSQRT31, 0.25, 4.0)}
# 4 x the largest of measure_cheb(name, key, seed) over seeds 0 .. 5
CHEB_BOUND = {"tanh3": 4 * 2.0 ** -29.73, "tanh15": 4 * 2.0 ** -37.20, "invsqrt31": 4 * 2.0 ** -35.82}


# ---- the definitions in Python integers --------------------------------------------------------------------------------

def py_int(w):
    """rint of a double as a Python integer (round half to even; a double at or above 2^53 is an integer)."""
    return int(round(float(w)))


def py_cheb_tensor(moduli, a, b, t, M, nl):
    """a, b, t u64[2][nl_x][N] (t None: the constant 1), M a Python integer -> u64[3][nl][N], exact."""
    N = a.shape[-1]
    out = np.empty((3, nl, N), dtype=np.uint64)
    for l in range(nl):
        q = int(moduli[l])
        a0, a1, b0, b1 = (x[l].astype(object) for x in (a[0], a[1], b[0], b[1]))
        t0, t1 = (t[0, l].astype(object), t[1, l].astype(object)) if t is not None else (1, 0)
        d = (2 * a0 * b0 - M * t0, 2 * (a0 * b1 + a1 * b0) - M * t1, 2 * a1 * b1)
        for k in range(3):
            out[k, l] = np.array(d[k] % q, dtype=np.uint64)
    return out


def py_affine(moduli, ct, Ma, Mc):
    """ct u64[2][nl][N] -> Ma ct + (Mc, 0), exact."""
    out = np.empty_like(ct)
    for l in range(ct.shape[1]):
        q = int(moduli[l])
        out[0, l] = np.array((Ma * ct[0, l].astype(object) + Mc) % q, dtype=np.uint64)
        out[1, l] = np.array((Ma * ct[1, l].astype(object)) % q, dtype=np.uint64)
    return out


def ladder_weight(sc, i, j):
    """S_i S_j / S_{i-j}: the product first, then the quotient; S_0 = 1 (sc is 1-based: sc[k - 1] belongs to T_k)."""
    prod = sc[i - 1] * sc[j - 1]
    return prod / sc[0] if i != j else prod


def cpu_cheb_ladder(o, u, rlk, n, scale):
    """[T_1 .. T_n] of u u64[2][nl][N] on the CPU: py_cheb_tensor, oracle_relinearize, the oracle's rescale."""
    _, sc = py_ladder(o.moduli, u.shape[1], n, scale)
    T = {1: u}
    for k in range(2, n + 1):
        i = (k + 1) // 2
        j = k - i
        nli = T[i].shape[1]
        d3 = py_cheb_tensor(o.moduli, T[i], T[j], T[1] if i != j else None, py_int(ladder_weight(sc, i, j)), nli)
        T[k] = o.rescale(oracle_relinearize(o, d3, rlk))
    return [T[k] for k in range(1, n + 1)], sc


def map_weights(moduli, L, sf, nl, a, b, scale):
    """(w_mul, w_add, nl_u, S_u) of the map of [a, b] onto [-1, 1]; None weights for (-1, 1)."""
    if (a, b) == (-1.0, 1.0):
        return None, None, nl, scale
    alpha, beta = 2.0 / (b - a), -(a + b) / (b - a)
    s_u = sf(L - (nl - 1))
    sigma1 = s_u * float(int(moduli[nl - 1]))
    return alpha * (sigma1 / scale), beta * sigma1, nl - 1, s_u


def cpu_cheb_eval(o, ct, rlk, coef, a, b, scale):
    """The whole algorithm on the CPU for one ciphertext u64[2][nl][N]; returns (u64[2][nl_out][N], S_out)."""
    nl = ct.shape[1]
    w_mul, w_add, nl_u, s_u = map_weights(o.moduli, o.L, o.sf, nl, a, b, scale)
    u = ct if w_mul is None else o.rescale(py_affine(o.moduli, ct, py_int(w_mul), py_int(w_add)))
    p = py_plan(len(coef) - 1, nl_u)
    w, s_out = py_cheb_weights(o.moduli, o.L, o.sf, coef, nl_u, s_u)
    xs, sx = cpu_cheb_ladder(o, u, rlk, p["B"], s_u)
    ys, _ = cpu_cheb_ladder(o, xs[-1], rlk, p["G"] - 1, sx[-1])
    d3 = py_poly_tensor(o.moduli, xs[:-1], ys, py_constants(w), p["nl_T"])
    return o.rescale(o.rescale(oracle_relinearize(o, d3, rlk))), s_out


# ---- decoded values on the CPU chain: where CHEB_BOUND comes from -----------------------------------------------------------

def cheb_case(o, seed, a, b):
    rng = np.random.default_rng(seed)
    N, L = o.N, o.L
    s, pa, e = make_keys(o, rng)
    pk, sk = o.keygen(s, pa, e)
    v = rng.uniform(a, b, size=N // 2)
    ct = o.encrypt(pk, o.encode(v, o.sf_big(0), L), sample_ternary(rng, N), sample_gauss(rng, N), sample_gauss(rng, N))
    return dict(s=s, pk=pk, sk=sk, v=v, ct=ct, rlk_rand=make_rk_rand(o, rng),
                scale=o.sf_big(0) / float(int(o.moduli[L - 1])))  # of the rescaled fresh ciphertext, on L - 1 limbs


def cheb_error(o, case, coef, a, b, out, s_out):
    u = (2.0 * case["v"] - (a + b)) / (b - a)
    return np.abs(o.decrypt_decode(out, case["sk"], s_out) - npcheb.chebval(u, coef)).max()


def measure_cheb(key, seed):
    name, coef, a, b = DECODED[key]
    c = CONFIGS[name]
    o = FastCpuContext(c[0], c[1], c[2], c[3], dnum=c[4])
    case = cheb_case(o, seed, a, b)
    rlk = oracle_relin_key(o, case["sk"], case["pk"], *case["rlk_rand"])
    out, s_out = cpu_cheb_eval(o, o.rescale(case["ct"]), rlk, coef, a, b, case["scale"])
    return cheb_error(o, case, coef, a, b, out, s_out)


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


INSTANCES = [(True, False), (False, False), (True, True), (False, True)]  # (square, ciphertext term)


def step_weights(moduli, nl, p_bits):
    """One negative, one of about 2^(2p) (capped a quarter below the level's modulus; far above 2^53 on every level), a tie
    (rint rounds to the even 12346) and one below 0.5 (M = 0)."""
    cap = sum(int(m).bit_length() - 1 for m in moduli[:nl]) - 2
    return [-0.7 * 2.0 ** min(p_bits, cap), 0.625 * 2.0 ** min(2 * p_bits, cap), 12345.5, 0.3]


_step = {}


def step_case(g, name, nl, n_ct, combos):
    """Operands with the edge residues at nl + 0, 1, 2 limbs (as far as the configuration has them) and the integer
    definition for each (instance, weight) of `combos`; computed once and shared (read-only)."""
    key = (name, nl, n_ct, combos)
    if key not in _step:
        rng = np.random.default_rng(2300 + 97 * nl + g.N.bit_length())
        nl_t, nl_a, nl_b = nl, min(g.L, nl + 1), min(g.L, nl + 2)
        a, b, t = (with_edges(rand_ct(rng, g, x, n_ct), g.moduli) for x in (nl_a, nl_b, nl_t))
        weights = step_weights(g.moduli, nl, CONFIGS[name][2])
        assert py_int(weights[1]) > 2 ** 53 and py_int(weights[2]) == 12346 and py_int(weights[3]) == 0
        want = {}
        for inst, wi in combos:
            square, term = INSTANCES[inst]
            bb = a if square else b
            want[(inst, wi)] = np.stack([py_cheb_tensor(g.moduli, a[c], bb[c], t[c] if term else None, py_int(weights[wi]), nl)
                                         for c in range(n_ct)])
            want[(inst, wi)].setflags(write=False)
        for arr in (a, b, t):
            arr.setflags(write=False)
        _step[key] = (a, nl_a, b, nl_b, t, nl_t, weights, want)
    return _step[key]


def dev_cheb_tensor(g, case, inst, wi, n_ct, nl, bufs=None):
    """cheb_tensor into a buffer pre-filled with POISON; the words around the output and the inputs are checked unchanged."""
    a, nl_a, b, nl_b, t, nl_t, weights, _ = case
    square, term = INSTANCES[inst]
    N = g.N
    words = n_ct * 3 * nl * N
    d_big = g.to_device(np.full(words + 4 * N, POISON, dtype=np.uint64))
    d_out = d_big.view(2 * N, (n_ct, 3, nl, N))
    d_a, d_b, d_t = bufs if bufs else (g.to_device(a), g.to_device(b), g.to_device(t))
    g.cheb_tensor(d_a, nl_a, d_a if square else d_b, nl_a if square else nl_b, d_t if term else None, nl_t, weights[wi], d_out,
                  n_ct, nl)
    big = d_big.to_host()
    assert np.all(big[:2 * N] == POISON) and np.all(big[2 * N + words:] == POISON)
    assert np.array_equal(d_a.to_host(), a) and np.array_equal(d_b.to_host(), b) and np.array_equal(d_t.to_host(), t)
    return d_out.to_host()


ALL = tuple((inst, wi) for inst in range(4) for wi in range(4))
# N = 2^16: a selection, so that the Python integers of the expectation stay a few seconds: every instance, the large weight
# on a constant instance (M far above 2^53) and with a term, the tie and M = 0 in the general instance with a term
C3 = ((0, 1), (1, 0), (2, 2), (3, 0), (3, 1), (3, 2), (3, 3))
# (name, nl, ciphertexts, (instance, weight) pairs)
STEP_CASES = [("n11", 3, 2, ALL), ("tiny", 1, 2, ALL), ("tiny", 2, 2, ALL), ("tiny", 3, 2, ALL), ("ref", 3, 1, ALL),
              ("c3", 7, 1, C3)]


def check_steps(g, name, nl, n_ct, combos):
    case = step_case(g, name, nl, n_ct, combos)
    bufs = tuple(g.to_device(x) for x in (case[0], case[2], case[4]))
    for inst, wi in combos:
        got = dev_cheb_tensor(g, case, inst, wi, n_ct, nl, bufs)
        assert np.array_equal(got, case[-1][(inst, wi)]), (name, nl, INSTANCES[inst], case[6][wi])


@gpu
@pytest.mark.parametrize("name,nl,n_ct,combos", STEP_CASES)
def test_cheb_tensor_is_the_integer_definition(ctxs, name, nl, n_ct, combos):
    g, _ = ctxs(name)
    check_steps(g, name, nl, n_ct, combos)


@gpu
@pytest.mark.parametrize("name,nl,n_ct,combos", [c for c in STEP_CASES if c[0] in ("tiny", "c3")])
@pytest.mark.parametrize("env", [{"MKCKKS_CHEB_FUSED": "0"}, {"MKCKKS_CHEB_FUSED": "1"}, {"MKCKKS_NO_FP64": "1"},
                                 {"MKCKKS_NO_PM": "1"}, {"MKCKKS_CHUNK": "1"}, {"MKCKKS_CHEB_FUSED": "0", "MKCKKS_NO_FP64": "1"}])
def test_cheb_tensor_under_the_library_switches(ctxs, monkeypatch, env, name, nl, n_ct, combos):
    """Switches are read once, when a context is created: a fresh context under each gives the bits of the definition,
    the composition (MKCKKS_CHEB_FUSED=0) included."""
    from ppqsflhe_amd import Context
    g0, _ = ctxs(name)
    step_case(g0, name, nl, n_ct, combos)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    c = CONFIGS[name]
    g = Context(c[0], c[1], c[2], c[3], dnum=c[4], device=0)
    try:
        check_steps(g, name, nl, n_ct, combos)
    finally:
        g.close()


def dev_ladder_by_hand(g, u, d_rlk, n_ct, nl, n, scale):
    """The loop the header states: cheb_tensor + relinearize + rescale, every step a call of its own."""
    N = g.N
    _, sc = py_ladder(g.moduli, nl, n, scale)
    T = {1: g.to_device(u)}
    nls = {1: nl}
    for k in range(2, n + 1):
        i = (k + 1) // 2
        j = k - i
        nli = nls[i]
        d_3, d_r, d_k = g.empty((n_ct, 3, nli, N)), g.empty((n_ct, 2, nli, N)), g.empty((n_ct, 2, nli - 1, N))
        g.cheb_tensor(T[i], nli, T[j], nls[j], T[1] if i != j else None, nl, ladder_weight(sc, i, j), d_3, n_ct, nli)
        g.relinearize(d_3, d_rlk, d_r, n_ct, nli)
        g.rescale(d_r, d_k, n_ct, nli)
        T[k], nls[k] = d_k, nli - 1
    return [T[k] for k in range(1, n + 1)], [nls[k] for k in range(1, n + 1)], sc


@gpu
@pytest.mark.parametrize("name,nl,n", [("tiny", 4, 3), ("c5s", 12, 8)])
def test_the_ladder_is_the_loop_of_steps_relinearisations_and_rescales(ctxs, name, nl, n):
    g, o = ctxs(name)
    N, n_ct = g.N, 2
    rng = np.random.default_rng(2400 + nl)
    u = rand_ct(rng, g, nl, n_ct)
    rlk = rand_evks(rng, o, 1)[0]
    d_u, d_rlk = g.to_device(u), g.to_device(rlk)
    scale = g.sf(g.L - nl)
    want_nl, want_s = py_ladder(g.moduli, nl, n, scale)
    words = n_ct * 2 * N * sum(want_nl)
    d_big = g.to_device(np.full(words + 4 * N, POISON, dtype=np.uint64))
    d_out = d_big.view(2 * N, (words,))
    nls, scales = g.cheb_ladder(d_u, d_rlk, d_out, n_ct, nl, n, scale)
    assert nls == want_nl and scales == want_s
    big = d_big.to_host()
    assert np.all(big[:2 * N] == POISON) and np.all(big[2 * N + words:] == POISON)
    assert np.array_equal(d_u.to_host(), u)
    got = split_powers(d_out.to_host(), nls, n_ct, N)
    want, hand_nl, _ = dev_ladder_by_hand(g, u, d_rlk, n_ct, nl, n, scale)
    assert hand_nl == want_nl
    for k in range(n):
        assert np.array_equal(got[k], want[k].to_host()), (name, k + 1)
    if name == "tiny":
        cpu, cpu_s = cpu_cheb_ladder(o, u[0], rlk, n, scale)
        assert cpu_s == scales
        for k in range(n):
            assert np.array_equal(got[k][0], cpu[k]), (name, k + 1, "CPU chain")


@gpu
@pytest.mark.parametrize("name,nl", [("tiny", 4), ("tiny", 1), ("n11", 3)])
def test_affine_is_the_integer_definition_in_place_and_out_of_place(ctxs, name, nl):
    g, _ = ctxs(name)
    N, n_ct = g.N, 2
    rng = np.random.default_rng(2500 + nl + g.N.bit_length())
    ct = with_edges(rand_ct(rng, g, nl, n_ct), g.moduli)
    cap = sum(int(m).bit_length() - 1 for m in g.moduli[:nl]) - 2
    p = CONFIGS[name][2]
    for w_mul, w_add in ((0.7 * 2.0 ** 30, -0.625 * 2.0 ** min(2 * p, cap)), (-12345.5, 0.3), (1.0, 0.75 * 2.0 ** min(p, cap)),
                         (0.0, -3.0)):
        want = np.stack([py_affine(g.moduli, ct[c], py_int(w_mul), py_int(w_add)) for c in range(n_ct)])
        words = ct.size
        d_in = g.to_device(ct)
        d_big = g.to_device(np.full(words + 4 * N, POISON, dtype=np.uint64))
        d_out = d_big.view(2 * N, ct.shape)
        g.affine(d_in, d_out, n_ct, nl, w_mul, w_add)
        big = d_big.to_host()
        assert np.all(big[:2 * N] == POISON) and np.all(big[2 * N + words:] == POISON)
        assert np.array_equal(d_in.to_host(), ct)
        assert np.array_equal(d_out.to_host(), want), (name, nl, w_mul, w_add)
        g.affine(d_in, d_in, n_ct, nl, w_mul, w_add)
        assert np.array_equal(d_in.to_host(), want), (name, nl, w_mul, w_add, "in place")


def dev_eval_by_hand(g, ct, d_rlk, coef, a, b, n_ct, nl, scale):
    """affine + rescale (unless (-1, 1)), cheb_ladder on u (n = B) and on y = T_B (n = G - 1), cheb_weights, poly_tensor,
    relinearize, rescale twice."""
    N = g.N
    w_mul, w_add, nl_u, s_u = map_weights(g.moduli, g.L, g.sf, nl, a, b, scale)
    d_u = g.to_device(ct)
    if w_mul is not None:
        d_m, d_u = g.empty((n_ct, 2, nl, N)), g.empty((n_ct, 2, nl_u, N))
        g.affine(g.to_device(ct), d_m, n_ct, nl, w_mul, w_add)
        g.rescale(d_m, d_u, n_ct, nl)
    p = g.poly_plan(len(coef) - 1, nl_u)
    B, G, nl_T = p["B"], p["G"], p["nl_T"]
    nlx, _ = py_ladder(g.moduli, nl_u, B, s_u)
    d_x = g.empty((n_ct * 2 * N * sum(nlx),))
    nls, sx = g.cheb_ladder(d_u, d_rlk, d_x, n_ct, nl_u, B, s_u)
    assert nls == nlx == p["baby_nl"] + [nlx[-1]]
    d_y = d_x.view(n_ct * 2 * N * sum(nlx[:-1]), (n_ct, 2, nlx[-1], N))
    nly, _ = py_ladder(g.moduli, nlx[-1], G - 1, sx[-1])
    d_g = g.empty((n_ct * 2 * N * sum(nly),))
    nls, _ = g.cheb_ladder(d_y, d_rlk, d_g, n_ct, nlx[-1], G - 1, sx[-1])
    assert nls == nly == p["giant_nl"]
    w, s_out = g.cheb_weights(coef, nl_u, s_u)
    d_3 = g.empty((n_ct, 3, nl_T, N))
    g.poly_tensor(d_x, p["baby_nl"], d_g, p["giant_nl"], w, d_3, n_ct, nl_T)
    d_r = g.empty((n_ct, 2, nl_T, N))
    g.relinearize(d_3, d_rlk, d_r, n_ct, nl_T)
    d_1, d_0 = g.empty((n_ct, 2, nl_T - 1, N)), g.empty((n_ct, 2, nl_T - 2, N))
    g.rescale(d_r, d_1, n_ct, nl_T)
    g.rescale(d_1, d_0, n_ct, nl_T - 1)
    return d_0.to_host(), s_out, p["nl_out"]


def check_eval(g, o, name, degree, a, b, nl, n_ct, against_cpu=False):
    N = g.N
    rng = np.random.default_rng(2600 + 13 * degree + nl)
    ct = rand_ct(rng, g, nl, n_ct)
    rlk = rand_evks(rng, o, 1)[0]
    coef = rng.uniform(-1, 1, size=degree + 1)
    coef[1] = 0.0
    scale = g.sf(g.L - nl)
    d_ct, d_rlk = g.to_device(ct), g.to_device(rlk)
    want, want_s, nl_out = dev_eval_by_hand(g, ct, d_rlk, coef, a, b, n_ct, nl, scale)
    words = n_ct * 2 * nl_out * N
    d_big = g.to_device(np.full(words + 4 * N, POISON, dtype=np.uint64))
    d_out = d_big.view(2 * N, (n_ct, 2, nl_out, N))
    s_out = g.cheb_eval(d_ct, d_rlk, coef, a, b, d_out, n_ct, nl, scale)
    big = d_big.to_host()
    assert np.all(big[:2 * N] == POISON) and np.all(big[2 * N + words:] == POISON)
    assert np.array_equal(d_ct.to_host(), ct)
    assert s_out == want_s == g.sf(g.L - nl_out)
    got = d_out.to_host()
    assert np.array_equal(got, want), (name, degree, a, b)
    if against_cpu:
        cpu, cpu_s = cpu_cheb_eval(o, ct[0], rlk, coef, a, b, scale)
        assert cpu_s == s_out and np.array_equal(got[0], cpu), (name, degree, "CPU chain")


@gpu
@pytest.mark.parametrize("a,b", [(-1.0, 1.0), (0.25, 4.0)])
@pytest.mark.parametrize("name,degree,nl", [("tiny", 3, 4)] + [("c5s", d, 12) for d in (2, 7, 15, 31, 63)])
def test_cheb_eval_is_its_composition(ctxs, name, degree, nl, a, b):
    g, o = ctxs(name)
    if name == "tiny":
        nl = 4 if (a, b) == (-1.0, 1.0) else 5  # the map spends a level: the same 4 limbs of u
    check_eval(g, o, name, degree, a, b, nl, 2, against_cpu=name == "tiny")


@gpu
def test_cheb_eval_across_workspace_chunks(ctxs, monkeypatch):
    """MKCKKS_CHUNK = 1, 3 ciphertexts, in a fresh context: every chunk reuses the engine's buffers."""
    from ppqsflhe_amd import Context
    _, o = ctxs("c5s")
    monkeypatch.setenv("MKCKKS_CHUNK", "1")
    c = CONFIGS["c5s"]
    g = Context(c[0], c[1], c[2], c[3], dnum=c[4], device=0)
    try:
        check_eval(g, o, "c5s", 15, 0.25, 4.0, 12, 3)
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("prefill", [58, 60, 62, 63, 64])  # the 7 lookups of the call: emptied at the last, ..., at the first
def test_cheb_eval_while_the_table_cache_is_emptied(ctxs, prefill):
    """The engine keeps at most 64 constant tables and frees them all when a 65th arrives.  A cheb_eval on a mapped
    interval looks up the map's table, one per ladder step and the outer sum's; with `prefill` tables already cached (affine
    maps with distinct weights, in a fresh context) the cache is emptied at a different lookup of the call each time,
    between the first and the last.  The result is that of the composition, computed in another context beforehand."""
    from ppqsflhe_amd import Context
    g0, o = ctxs("c5s")
    N, nl, n_ct, degree, a, b = g0.N, 12, 2, 15, 0.25, 4.0
    rng = np.random.default_rng(2700)
    ct = rand_ct(rng, g0, nl, n_ct)
    rlk = rand_evks(rng, o, 1)[0]
    coef = rng.uniform(-1, 1, size=degree + 1)
    scale = g0.sf(g0.L - nl)
    want, want_s, nl_out = dev_eval_by_hand(g0, ct, g0.to_device(rlk), coef, a, b, n_ct, nl, scale)
    c = CONFIGS["c5s"]
    g = Context(c[0], c[1], c[2], c[3], dnum=c[4], device=0)
    try:
        d_small = g.empty((1, 2, 1, N))
        for k in range(prefill):
            g.affine(d_small, d_small, 1, 1, float(k + 2), float(k))  # a table per distinct pair of weights
        d_out = g.empty((n_ct, 2, nl_out, N))
        for _ in range(2):  # the second call finds some of its tables cached and some not
            s_out = g.cheb_eval(g.to_device(ct), g.to_device(rlk), coef, a, b, d_out, n_ct, nl, scale)
            assert s_out == want_s and np.array_equal(d_out.to_host(), want), prefill
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("key", ["tanh3", "tanh15", "invsqrt31"])
def test_decoded_values_of_an_encrypted_series(ctxs, key):
    """Real encode / encrypt under a generated key; the relinearisation key, the rescale and the evaluation on the device;
    decryption and decoding on the oracle; compared with the fitted series' own value."""
    name, coef, a, b = DECODED[key]
    g, o = ctxs(name)
    N, L, D = g.N, g.L, g.D
    case = cheb_case(o, 5, a, b)
    d_rlk = g.empty((g.beta, 2, D, N))
    g.relin_keygen(g.to_device(case["s"]), g.to_device(case["pk"]), *[g.to_device(x) for x in case["rlk_rand"]], d_rlk)
    d_x = g.empty((1, 2, L - 1, N))
    g.rescale(g.to_device(case["ct"][None]), d_x, 1, L)
    nl_u = L - 1 if (a, b) == (-1.0, 1.0) else L - 2
    p = g.poly_plan(len(coef) - 1, nl_u)
    d_out = g.empty((1, 2, p["nl_out"], N))
    s_out = g.cheb_eval(d_x, d_rlk, coef, a, b, d_out, 1, L - 1, case["scale"])
    err = cheb_error(o, case, coef, a, b, d_out.to_host()[0], s_out)
    print(f"{key}: error 2^{np.log2(err):.2f}, bound 2^{np.log2(CHEB_BOUND[key]):.2f}")
    assert err <= CHEB_BOUND[key], (key, err)


@gpu
def test_cheb_refusals_on_a_device_context(ctxs):
    from ppqsflhe_amd.binding import MkckksError
    g, _ = ctxs("tiny")
    N, nl = g.N, 3
    d_a, d_b, d_t = g.empty((1, 2, 4, N)), g.empty((1, 2, 5, N)), g.empty((1, 2, 3, N))
    d_out = g.empty((2, 3, nl, N))
    d_rlk = g.empty((g.beta, 2, g.D, N))

    def refused(call, text):
        with pytest.raises(MkckksError) as e:
            call()
        assert e.value.code == -1 and text in str(e.value), (text, str(e.value))

    step = lambda a=d_a, b=d_b, t=d_t, o=d_out, w=7.0, la=4, lb=5, lt=3: g.cheb_tensor(a, la, b, lb, t, lt, w, o, 1, nl)
    refused(lambda: step(o=d_a), "overlaps")                                           # d_out3 is an input
    refused(lambda: step(t=d_out.view(N, (1, 2, 3, N))), "overlaps")                   # the term inside d_out3
    refused(lambda: step(o=d_out.view(1, (1, 3, nl, N))), "16-byte aligned")           # an odd word offset
    refused(lambda: step(a=d_a.view(1, (1,))), "16-byte aligned")
    half_q = 0.5
    for m in g.moduli[:nl]:
        half_q *= float(int(m))
    refused(lambda: step(w=half_q * 1.001), "does not fit")                            # |w| beyond the modulus bound
    refused(lambda: step(w=np.inf), "not finite")
    refused(lambda: step(la=nl - 1), "limb count")                                     # an operand below nl
    refused(lambda: step(t=d_t, lt=nl - 1), "limb count")
    refused(lambda: step(b=d_a, lb=5), "one limb count")                               # a square at two limb counts
    d_ct, d_res = g.empty((1, 2, 4, N)), g.empty((1, 2, 1, N))
    scale, coef = g.sf(g.L - 4), [1.0, 0.5, 0.25, 0.125]
    refused(lambda: g.cheb_eval(d_ct, d_rlk, coef, -1.0, 1.0, d_res, 1, 3, g.sf(g.L - 3)), "needs 4 limbs")  # nl_out < 1
    refused(lambda: g.cheb_eval(d_ct, d_rlk, coef, 0.25, 4.0, d_res, 1, 4, scale), "needs 4 limbs")
    refused(lambda: g.cheb_eval(d_ct, d_rlk, coef, 1.0, 1.0, d_res, 1, 4, scale), "finite a < b")
    refused(lambda: g.cheb_eval(d_ct, d_rlk, coef, -1.0, 1.0, d_ct, 1, 4, scale), "overlaps")
    refused(lambda: g.cheb_eval(d_ct, d_rlk, coef, -1.0, 1.0, d_res.view(1, (1,)), 1, 4, scale), "16-byte aligned")
    refused(lambda: g.cheb_ladder(d_ct, d_rlk, d_ct, 1, 4, 3, scale), "overlaps")
    refused(lambda: g.cheb_ladder(d_ct, d_rlk, d_out, 1, 4, 9, scale), "power ladder")
    refused(lambda: g.cheb_ladder(d_ct, d_rlk, d_out, 1, 2, 2, 2.0 ** 60), "does not fit")  # a step's weight S^2 at 2 limbs
    refused(lambda: g.affine(d_ct, d_ct.view(1, (1,)), 1, 4, 3.0, 5.0), "16-byte aligned")
    refused(lambda: g.affine(d_ct, d_ct.view(2 * N, (1,)), 1, 4, 3.0, 5.0), "overlaps")
    g.cheb_eval(d_ct, d_rlk, coef, -1.0, 1.0, d_res, 0, 4, scale)                       # zero count: a no-op


if __name__ == "__main__":
    for key in DECODED:
        errs = [measure_cheb(key, seed) for seed in range(6)]
        for seed, e in enumerate(errs):
            print(f"{key} seed {seed}: 2^{np.log2(e):.2f}")
        print(f"{key}: 2^{np.log2(min(errs)):.2f} .. 2^{np.log2(max(errs)):.2f}")
