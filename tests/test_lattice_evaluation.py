"""The evaluation entry points up to the linear transforms on every parameter region of tests/test_parameter_lattice.py's
TABLE; polynomial and Chebyshev evaluation, which came after them, run on the same table in tests/test_lattice_poly.py.

The feature tests of the plaintext products, the weighted aggregation, rotations, ciphertext products, collective keys, the
share protocols and the linear transforms run on the seven CONFIGS shapes of tests/test_gpu_parity.py, which all have one
class layout (q_0 pseudo-Mersenne at 60 bits, fp64 scaling limbs, pseudo-Mersenne P limbs, a 20-bit extra limb).  Their
kernels pick the arithmetic per limb from the limb table, so this file runs them once per TABLE entry: Shoup-class q_0 and
scaling limbs beside an fp64 limb, an fp64 q_0, fp64-class P limbs, 18- and 30-bit limbs, digit sizes 1, 5 and 8, K = 8,
L = 32, and the rings 2^8, 2^13, 2^15 (generic transforms) beside 2^16 and 2^17.

One test function per section, parametrised over every name of TABLE (`test_every_section_covers_every_table_entry` checks
that, without a device).  The `ctxs` fixture is test_parameter_lattice's: it asserts the entry's arithmetic classes before
anything else.  Every comparison is np.array_equal against Python-integer or oracle references -- the helpers of the feature
test files, unchanged; there is no tolerance in this file.  Inputs and expected results are built once per (section, entry)
by the `*_case` functions, which need the oracle only, kept read-only in `_CASES` and shared with the runs under the library
switches (a fresh context per switch, as test_key_switch_under_the_arithmetic_switches does it).

Shapes: B = _batch (2 up to N = 2^14, 1 above), nl in {L, L - 1} (L - 1 is a partial last digit wherever alpha does not
divide it; the three rings of 2^16 and 2^17 run nl = L only).  Random inputs carry q_i - 1 in every third or fifth word of
item 0 and one pattern of 0 beside q_i - 1.  The 33-term tensor sum is pointwise, so its operands are 512 distinct columns
repeated along the ring: every device word is compared, and the Python-integer reference stays below a second.

Two input patterns beyond those of the feature tests, because q - 1 is the edge of the integer classes only (a product of
two q - 1 is 1): the 33-term tensor operands carry columns whose products have centred remainders next to +q/2 and -q/2 in
every term (`with_half_moduli`: the longest same-sign runs of the fp64 class's lazy sums; with TENSOR_FP_TERMS raised to 8
test_products[d30] fails on its 50-bit fp64 limbs), and the extreme linear-transform cases run a third pattern with uniform
inner sums under plaintexts at q - 1 ("outer").  The pseudo-Mersenne fold of k_lt_accum has slack the tests cannot take away:
64 products are inside pm_reduce128's documented range, and with the small c of the moduli generate() picks 128 are too.

Wall time on an MI355X: the whole file (238 tests) 37 s; slowest test 2.1 s
(test_extreme_residues_through_the_linear_transform[d30-q-1]), every other one below 1.5 s.
"""
import os
import re
import types

import numpy as np
import pytest

from tests.test_collective_keys import check_relin_share, dev_evk_sum, py_relin_share, py_sum, share_case  # noqa: F401
from tests.test_gpu_parity import make_keys, make_rk_rand, rand_ct, rand_polys
from tests.test_key_sharing import KEY, rand_weights, shamir_ref, wsum_ref
from tests.test_key_switch_shares import exact_switch_share, switch_share
from tests.test_key_switch_shares import wide_inputs as switch_inputs
from tests.test_linear_transform import cadences, dev_lt, extreme_case, random_case, ref_linear_transform
from tests.test_parameter_lattice import FP64, NAMES, PM, TABLE, _batch, _kwargs, ctxs, oracle  # noqa: F401  (ctxs: fixture)
from tests.test_product import check_products, dev_tensor, oracle_relin_key, oracle_relinearize, py_tensor, relin_case, with_edges
from tests.test_rotation import gal, oracle_rotate, oracle_slot_sum, rand_evks, sigma_coeff, src_index
from tests.test_seeded_ciphertexts import uniform_stream
from tests.test_slot_weights import expected, py_product
from tests.test_threshold_decrypt import sum_mod
from tests.test_weighted_aggregation import WEIGHTS, device_wsum, oracle_wsum, scaled_evk

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BIG = ("s56n16", "s21n16", "s24n17")  # N = 2^16 and 2^17: nl = L only
TENSOR_TERMS, TENSOR_COLUMNS = 33, 512
KEY2 = bytes(range(101, 133))
# a fresh context per switch; the class the switch removes (None: the switch changes a path, not a class)
FORKS = [("a45", "MKCKKS_NO_FP64", "1", FP64), ("s54", "MKCKKS_NO_FP64", "1", FP64), ("al8k8", "MKCKKS_NO_FP64", "1", FP64),
         ("f52", "MKCKKS_NO_PM", "1", PM), ("a55", "MKCKKS_NO_PM", "1", PM),
         ("a45", "MKCKKS_RELSHARE_FUSED", "0", None), ("s59", "MKCKKS_RELSHARE_FUSED", "0", None),
         ("a45", "MKCKKS_PLAIN_FUSED", "0", None), ("s59", "MKCKKS_PLAIN_FUSED", "0", None),
         ("a45", "MKCKKS_LT_ORDER", "1", None)]
EXTREME_LT = ["s59", "f40", "a45", "e30", "d30"]
EXTREME_KS = ["s59", "f40", "a45", "al8k8"]


def levels(name):
    L = TABLE[name][1][0]
    return (L,) if name in BIG else (L, L - 1)


def tensor_cadences():
    """The fold cadences of the tensor kernel's lazy sums (fp64, pseudo-Mersenne), read from its constants."""
    src = open(os.path.join(ROOT, "ppqsflhe_amd", "csrc", "tensor_kernels.hpp")).read()
    m = re.search(r"TENSOR_FP_TERMS = (\d+), TENSOR_PM_TERMS = (\d+);", src)
    return tuple(int(x) for x in m.groups())


# ---- inputs ---------------------------------------------------------------------------------------------------------

def edge_polys(rng, o, ids, count):
    """uniform residues; item 0: q - 1 in every third word, 0 right behind it"""
    x = rand_polys(rng, o, ids, count)
    x[0, :, ::3] = (o.moduli[ids] - np.uint64(1))[:, None]
    x[0, :, 1::3] = 0
    return x


def edge_ct(rng, o, nl, B):
    """uniform residues; item 0: c1 with q - 1 in every third word, c0 with q - 1 in every fifth and 0 right behind it"""
    ct = rand_ct(rng, o, nl, B)
    q1 = (o.moduli[:nl] - np.uint64(1))[:, None]
    ct[0, 1, :, ::3] = q1
    ct[0, 0, :, ::5] = q1
    ct[0, 0, :, 1::5] = 0
    return ct


def edge_evks(rng, o, n):
    """[n][beta][2][D][N] uniform; key 0: q - 1 in every fifth word of every limb, P limbs included"""
    evks = rand_evks(rng, o, n)
    evks[0, :, :, :, ::5] = (o.moduli - np.uint64(1))[:, None]
    return evks


def all_q_minus_1(o, ids, lead):
    x = np.empty(tuple(lead) + (len(ids), o.N), dtype=np.uint64)
    for j, l in enumerate(ids):
        x[..., j, :] = np.uint64(int(o.moduli[l]) - 1)
    return x


def with_half_moduli(rng, a, b, moduli):
    """a, b u64[T][1][2][nl][W]: columns 4 .. 35 get the operands whose products have centred remainders next to +q/2 and
    -q/2 in every term -- the longest same-sign runs of the fp64 class's lazy sums (a product of two q - 1 is 1: the edge
    of the integer classes' 128-bit sums, and nothing to a sum of remainders).  The offsets make the partial sums odd.
    Columns 4 .. 19: a0 = a1 = 1 and b0, b1 at q/2 -+ d (d1 of the general instance); columns 20 .. 35: a0 = 1 and a1 at
    q/2 -+ d (2 a0 a1 of the square instance)."""
    a, b = a.copy(), b.copy()
    T, nl = a.shape[0], a.shape[-2]
    for i in range(nl):
        h = (int(moduli[i]) - 1) // 2
        d = rng.integers(0, 1 << 8, size=(3, T, 16), dtype=np.uint64)
        near = np.concatenate([np.uint64(h) - d[:, :, :8], np.uint64(h + 1) + d[:, :, 8:]], axis=2)  # +q/2 x 8, -q/2 x 8
        a[:, 0, :, i, 4:20] = 1
        b[:, 0, 0, i, 4:20], b[:, 0, 1, i, 4:20] = near[0], near[1]
        a[:, 0, 0, i, 20:36], a[:, 0, 1, i, 20:36] = 1, near[2]
    return a, b


_CASES = {}


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _freeze(v)


def cached(build, name):
    """inputs and reference results of one (section, entry): built once from the oracle alone, read-only afterwards"""
    key = (build.__name__, name)
    if key not in _CASES:
        case = build(name)
        _freeze(case)
        _CASES[key] = case
    return _CASES[key]


def same(got, want, *tag):
    assert np.array_equal(got, want), tag


# ---- 1: plain products and sums ---------------------------------------------------------------------------------------

def plain_case(name):
    o = oracle(name)
    rng = np.random.default_rng(1101)
    L, B = o.L, _batch(o)
    case = dict(B=B)
    for nl in levels(name):
        ct, pt = edge_ct(rng, o, nl, B), edge_polys(rng, o, list(range(nl)), B)
        forms = sorted({1, B})
        case["mult", nl] = dict(ct=ct, pt=pt, prod={n: [py_product(o, ct[b], pt[b % n]) for b in range(B)] for n in forms},
                                resc={n: expected(o, o, ct, pt, n) for n in forms})
        ct, acc, evk = edge_ct(rng, o, nl, B), edge_ct(rng, o, nl, B), edge_evks(rng, o, 1)[0]
        case["acc", nl] = dict(ct=ct, acc=acc, evk=evk,
                               want=np.stack([o.eval_add(acc[b], o.reencrypt(ct[b], evk)) for b in range(B)]))
    a, b = edge_ct(rng, o, L, B), edge_ct(rng, o, L, B)
    case["add"] = dict(a=a, b=b, want=np.stack([o.eval_add(a[i], b[i]) for i in range(B)]))
    cts = np.stack([edge_ct(rng, o, L, B) for _ in range(5)])  # 5 clients: past k_sum's fold at 4
    cts[2] = all_q_minus_1(o, list(range(L)), (B, 2))
    want = []
    for i in range(B):
        acc = cts[0, i]
        for c in range(1, 5):
            acc = o.eval_add(acc, cts[c, i])
        want.append(acc)
    case["sum"] = dict(cts=cts, want=np.stack(want))
    return case


def run_plain(g, o, name, tag):
    case = cached(plain_case, name)
    N, L, B = g.N, g.L, case["B"]
    for nl in levels(name):
        c = case["mult", nl]
        for n_pt in sorted({1, B}):
            d_in, d_pt, d_out = g.to_device(c["ct"]), g.to_device(c["pt"][:n_pt]), g.empty((B, 2, nl - 1, N))
            g.mult_plain_rescale(d_in, d_pt, d_out, B, n_pt, nl)
            same(d_in.to_host(), c["ct"], name, tag, "mult_plain_rescale changed its input", nl, n_pt)
            got = d_out.to_host()
            for b in range(B):
                same(got[b], c["resc"][n_pt][b], name, tag, "mult_plain_rescale", nl, n_pt, b)
            g.mult_plain(d_in, d_pt, B, n_pt, nl)
            got = d_in.to_host()
            for b in range(B):
                same(got[b], c["prod"][n_pt][b], name, tag, "mult_plain", nl, n_pt, b)
        c = case["acc", nl]
        d_acc = g.to_device(c["acc"])
        g.reencrypt_accumulate(g.to_device(c["ct"]), g.to_device(c["evk"]), d_acc, B, nl)
        same(d_acc.to_host(), c["want"], name, tag, "reencrypt_accumulate", nl)
    c = case["add"]
    d_out = g.empty((B, 2, L, N))
    g.eval_add(g.to_device(c["a"]), g.to_device(c["b"]), d_out, B, L)
    same(d_out.to_host(), c["want"], name, tag, "eval_add")
    c = case["sum"]
    d_in = g.to_device(c["cts"])
    g.eval_sum(d_in, d_out, 5, B, L)
    same(d_out.to_host(), c["want"], name, tag, "eval_sum")
    same(d_in.to_host(), c["cts"], name, tag, "eval_sum changed its input")


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_plain_products_and_sums(ctxs, name):
    g, o = ctxs(name)
    run_plain(g, o, name, "default")


# ---- 2: weighted aggregation ------------------------------------------------------------------------------------------

W3 = [0.3125, 1.0, 0.123456789]


def weighted_case(name):
    o = oracle(name)
    rng = np.random.default_rng(1202)
    L, B = o.L, _batch(o)
    evks = edge_evks(rng, o, 3)
    case = dict(B=B, evks=evks)
    for nl in levels(name):
        sf_level = L - nl + 1
        cts = np.stack([edge_ct(rng, o, nl, B) for _ in range(3)])
        scaled = np.stack([scaled_evk(o, evks[c], W3[c], sf_level) for c in range(3)])
        case["wsum", nl] = dict(cts=cts, scaled=scaled,
                                want=np.stack([oracle_wsum(o, cts, scaled, W3, sf_level, b) for b in range(B)]))
    terms, weights = np.stack([edge_ct(rng, o, L, B) for _ in range(5)]), WEIGHTS[:5]
    prods = [[o.mult_factors(terms[k, b], o.const_factors(L, 1, weights[k])) for b in range(B)] for k in range(5)]
    want = {}
    for first_is_sum in (False, True):
        out = []
        for b in range(B):
            acc = terms[0, b] if first_is_sum else prods[0][b]
            for k in range(1, 5):
                acc = o.eval_add(acc, prods[k][b])
            out.append(acc)
        want[first_is_sum] = np.stack(out)
    case["terms"] = dict(terms=terms, weights=weights, want=want)
    return case


def run_weighted(g, o, name, tag):
    case = cached(weighted_case, name)
    N, L, B = g.N, g.L, case["B"]
    for nl in levels(name):
        c = case["wsum", nl]
        got, d_scaled = device_wsum(g, c["cts"], case["evks"], W3, L - nl + 1, nl)
        same(d_scaled.to_host(), c["scaled"], name, tag, "scale_evk", nl)
        same(got, c["want"], name, tag, "reencrypt_wsum", nl)
    c = case["terms"]
    for first_is_sum in (False, True):
        d_out = g.empty((B, 2, L, N))
        g.eval_wsum(g.to_device(c["terms"]), d_out, 5, B, L, c["weights"], 1, first_is_sum)
        same(d_out.to_host(), c["want"][first_is_sum], name, tag, "eval_wsum", first_is_sum)


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_weighted_aggregation(ctxs, name):
    g, o = ctxs(name)
    run_weighted(g, o, name, "default")


# ---- 3: rotations -----------------------------------------------------------------------------------------------------

def rotation_case(name):
    o = oracle(name)
    rng = np.random.default_rng(1303)
    N, L, B = o.N, o.L, _batch(o)
    case = dict(B=B, x=edge_polys(rng, o, list(range(L)), B))
    case["gs"] = [5, pow(5, -1, 2 * N), 2 * N - 1, gal(N, N // 4 - 1)]
    s, a, e = make_keys(o, rng)
    pk, _ = o.keygen(s, a, e)
    u, e0, e1 = make_rk_rand(o, rng)
    keys = {}
    for gel in (gal(N, 1), 2 * N - 1):
        sg = sigma_coeff(s, gel)
        keys[gel] = (sg, o.rekeygen(sg, pk, u, e0, e1))
    case["keygen"] = dict(s=s, pk=pk, u=u, e0=e0, e1=e1, keys=keys)
    evks = edge_evks(rng, o, 2)
    case["evks"] = evks
    for nl in levels(name):
        ct = edge_ct(rng, o, nl, B)
        gel = gal(N, 3 if nl % 2 else -(N // 4 - 1))
        case["rotate", nl] = dict(ct=ct, gel=gel, want=np.stack([oracle_rotate(o, ct[b], evks[0], gel) for b in range(B)]))
    nl = levels(name)[-1]
    ct = case["rotate", nl]["ct"]
    case["slot_sum"] = dict(nl=nl, want=np.stack([oracle_slot_sum(o, ct[b], evks, 4) for b in range(B)]))
    return case


def run_rotations(g, o, name, tag):
    case = cached(rotation_case, name)
    N, L, D, B = g.N, g.L, g.D, case["B"]
    x = case["x"]
    d_in, d_out = g.to_device(x), g.empty(x.shape)
    for gel in case["gs"]:
        g.automorphism(d_in, d_out, B, L, gel)
        same(d_out.to_host(), x[:, :, src_index(N, gel)], name, tag, "automorphism", gel)
    same(d_in.to_host(), x, name, tag, "automorphism changed its input")
    c = case["keygen"]
    d_s, d_pk = g.to_device(c["s"]), g.to_device(c["pk"])
    d_u, d_e0, d_e1 = g.to_device(c["u"]), g.to_device(c["e0"]), g.to_device(c["e1"])
    for gel, (sg, evk) in c["keys"].items():
        d_sg, d_evk = g.empty((N,), np.int8), g.empty((g.beta, 2, D, N))
        g.automorphism_secret(d_s, d_sg, gel)
        same(d_sg.to_host(), sg, name, tag, "automorphism_secret", gel)
        g.galois_keygen(d_s, d_pk, d_u, d_e0, d_e1, gel, d_evk)
        same(d_evk.to_host(), evk, name, tag, "galois_keygen", gel)
    d_evks = g.to_device(case["evks"])
    for nl in levels(name):
        c = case["rotate", nl]
        d_ct, d_out = g.to_device(c["ct"]), g.empty(c["ct"].shape)
        g.rotate(d_ct, d_evks, d_out, B, nl, c["gel"])  # the first key of the pair
        same(d_out.to_host(), c["want"], name, tag, "rotate", nl)
        same(d_ct.to_host(), c["ct"], name, tag, "rotate changed its input", nl)
    c = case["slot_sum"]
    ct = case["rotate", c["nl"]]["ct"]
    d_ct, d_out = g.to_device(ct), g.empty(ct.shape)
    g.slot_sum(d_ct, d_evks, d_out, B, c["nl"], 4)
    same(d_out.to_host(), c["want"], name, tag, "slot_sum")
    same(d_ct.to_host(), ct, name, tag, "slot_sum changed its input")


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_rotations(ctxs, name):
    g, o = ctxs(name)
    run_rotations(g, o, name, "default")


# ---- 4: products ------------------------------------------------------------------------------------------------------

def product_case(name):
    o = oracle(name)
    rng = np.random.default_rng(1404)
    N, L, B = o.N, o.L, _batch(o)
    case = dict(B=B)
    a = with_edges(np.stack([rand_ct(rng, o, L, B)]), o.moduli)
    b = with_edges(np.stack([rand_ct(rng, o, L, B)]), o.moduli)
    case["tensor", 1] = dict(a=a, b=b, want=np.stack([py_tensor(o.moduli, a[:, i], b[:, i]) for i in range(B)]),
                             want_sq=np.stack([py_tensor(o.moduli, a[:, i], a[:, i]) for i in range(B)]))
    # 33 terms, one ciphertext: TENSOR_COLUMNS distinct columns (the edge residues among them) repeated along the ring
    W = min(N, TENSOR_COLUMNS)
    narrow = types.SimpleNamespace(N=W, moduli=o.moduli)
    a = with_edges(np.stack([rand_ct(rng, narrow, L, 1) for _ in range(TENSOR_TERMS)]), o.moduli)
    b = with_edges(np.stack([rand_ct(rng, narrow, L, 1) for _ in range(TENSOR_TERMS)]), o.moduli)
    a, b = with_half_moduli(rng, a, b, o.moduli)
    wide = lambda x: np.tile(x, N // W)
    case["tensor", TENSOR_TERMS] = dict(a=wide(a), b=wide(b), want=wide(py_tensor(o.moduli, a[:, 0], b[:, 0]))[None],
                                        want_sq=wide(py_tensor(o.moduli, a[:, 0], a[:, 0]))[None])
    s, a_, e = make_keys(o, rng)
    pk, sk = o.keygen(s, a_, e)
    u, e0, e1 = make_rk_rand(o, rng)
    case["keygen"] = dict(s=s, pk=pk, u=u, e0=e0, e1=e1, want=oracle_relin_key(o, sk, pk, u, e0, e1))
    for nl in levels(name):
        relin_case(o, name, nl, B)  # tests/test_product.py keeps it (read-only) under (name, nl, B)
    return case


def run_products(g, o, name, tag):
    case = cached(product_case, name)
    N, L, D, B = g.N, g.L, g.D, case["B"]
    fp_terms, pm_terms = tensor_cadences()
    assert TENSOR_TERMS > 2 * max(fp_terms, pm_terms)  # both classes fold twice
    for T in (1, TENSOR_TERMS):
        c = case["tensor", T]
        same(dev_tensor(g, c["a"], c["b"], L), c["want"], name, tag, "tensor_sum", T)
        same(dev_tensor(g, c["a"], c["a"], L, square=True), c["want_sq"], name, tag, "tensor_sum, square", T)
    c = case["keygen"]
    d_evk = g.empty((g.beta, 2, D, N))
    g.relin_keygen(g.to_device(c["s"]), g.to_device(c["pk"]), g.to_device(c["u"]), g.to_device(c["e0"]), g.to_device(c["e1"]),
                   d_evk)
    same(d_evk.to_host(), c["want"], name, tag, "relin_keygen")
    for nl in levels(name):
        # relinearize, mult_relin out of place, onto a, onto b, and the square
        check_products(g, relin_case(o, name, nl, B), nl, (name, tag, nl))


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_products(ctxs, name):
    g, o = ctxs(name)
    run_products(g, o, name, "default")


# ---- 5: collective keys -----------------------------------------------------------------------------------------------

def collective_case(name):
    o = oracle(name)
    rng = np.random.default_rng(1505)
    shares = rand_evks(rng, o, 5).reshape(5, 1, o.beta, 2, o.D, o.N)  # 5 parties: past k_sum's fold at 4
    shares[3] = all_q_minus_1(o, list(range(o.D)), (1, o.beta, 2))
    for i in range(o.D):
        shares[:3, ..., i, 0] = np.uint64(int(o.moduli[i]) - 1)
        shares[:3, ..., i, 1] = 0
    share_case(o, name)  # tests/test_collective_keys.py keeps it (read-only) under the name
    return dict(shares=shares, want=py_sum(o.moduli, shares))


def run_collective(g, o, name, tag):
    case = cached(collective_case, name)
    same(dev_evk_sum(g, case["shares"]), case["want"], name, tag, "evk_sum")
    same(dev_evk_sum(g, case["shares"], in_place=True), case["want"], name, tag, "evk_sum in place")
    check_relin_share(g, share_case(o, name), (name, tag))


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_collective_keys(ctxs, name):
    g, o = ctxs(name)
    run_collective(g, o, name, "default")


# ---- 6: shares --------------------------------------------------------------------------------------------------------

SHARE_SID = 40


def share_levels(name):
    L = TABLE[name][1][0]
    return (L,) if name in BIG else (L, L - 1, 1)


def shares_case(name):
    o = oracle(name)
    rng = np.random.default_rng(1606)
    N, L, D, B = o.N, o.L, o.D, _batch(o)
    moduli = [int(q) for q in o.moduli]
    ct, sk, pk, v, e0, e1 = switch_inputs(rng, o, L, B)  # 62-bit errors
    case = dict(B=B, switch=dict(ct=ct, sk=sk, pk=pk, v=v, e0=e0, e1=e1))
    for lead in (0, 1):
        for nl in share_levels(name):
            case["switch", lead, nl] = np.stack([exact_switch_share(o, ct[b], sk, pk, v[b], e0[b], e1[b], nl, lead)
                                                 for b in range(B)])
    shares = np.stack([edge_polys(rng, o, list(range(L)), B) for _ in range(3)])
    shares[1] = all_q_minus_1(o, list(range(L)), (B,))
    case["fuse"] = dict(shares=shares, want=sum_mod(o, list(shares)))
    # the uniform stream: Q limbs of streams SHARE_SID and SHARE_SID + 1 (the Shamir coefficients r_1, r_2 of a 3-of-5
    # sharing, and c1 of two seeded ciphertexts), all D limbs of stream 7
    q_streams = [uniform_stream(KEY, SHARE_SID + k, moduli[:L], N)[0] for k in range(2)]
    case["stream"] = dict(q=q_streams, q2=uniform_stream(KEY2, SHARE_SID + 1, moduli[:L], N)[0],
                          d=uniform_stream(KEY, 7, moduli, N)[0])
    key = edge_polys(rng, o, list(range(D)), 1)[0]
    case["shamir"] = dict(sk=key, want=shamir_ref(key[:L], q_streams, moduli[:L], 5))
    inp, w = edge_polys(rng, o, list(range(L)), 5), rand_weights(rng, o, 5, L)
    inp[1], w[1] = all_q_minus_1(o, list(range(L)), ()), o.moduli[:L] - np.uint64(1)
    case["combine"] = dict(inp=inp, w=w, want=wsum_ref(inp, w, moduli[:L]))
    return case


def run_shares(g, o, name, tag):
    case = cached(shares_case, name)
    N, L, D, B = g.N, g.L, g.D, case["B"]
    c = case["switch"]
    for lead in (0, 1):
        for nl in share_levels(name):
            got = switch_share(g, c["ct"], c["sk"], c["pk"], c["v"], c["e0"], c["e1"], nl, lead)
            same(got, case["switch", lead, nl], name, tag, "switch_share", lead, nl)
    c = case["fuse"]
    d_m = g.empty((B, L, N))
    g.fuse_shares(g.to_device(c["shares"]), d_m, 3, B, L)
    same(d_m.to_host(), c["want"], name, tag, "fuse_shares")
    c = case["stream"]
    d_q, d_d = g.empty((1, L, N)), g.empty((1, D, N))
    g.sample_uniform(d_q, 1, L, False, KEY, SHARE_SID)
    same(d_q.to_host()[0], c["q"][0], name, tag, "sample_uniform")
    g.sample_uniform(d_d, 1, L, True, KEY, 7)
    same(d_d.to_host()[0], c["d"], name, tag, "sample_uniform with P")
    ct = np.stack([case["switch"]["ct"][0], case["switch"]["ct"][0]])
    d_ct = g.to_device(ct)
    g.expand_seeded(d_ct, 2, L, [KEY, KEY2], [SHARE_SID, SHARE_SID + 1])
    got = d_ct.to_host()
    same(got[:, 0], ct[:, 0], name, tag, "expand_seeded changed c0")
    same(got[0, 1], c["q"][0], name, tag, "expand_seeded", 0)
    same(got[1, 1], c["q2"], name, tag, "expand_seeded", 1)
    c = case["shamir"]
    d_shares = g.empty((5, L, N))
    g.share_key(g.to_device(c["sk"]), d_shares, L, 5, 3, KEY, SHARE_SID)
    same(d_shares.to_host(), c["want"], name, tag, "share_key")
    c = case["combine"]
    d_in, d_out = g.to_device(c["inp"]), g.empty((L, N))
    g.combine_key_shares(d_in, c["w"], d_out, 5, L)
    same(d_out.to_host(), c["want"], name, tag, "combine_key_shares")
    g.combine_key_shares(d_in, c["w"], d_in, 5, L)  # out = in[0]
    same(d_in.to_host()[0], c["want"], name, tag, "combine_key_shares in place")


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_shares(ctxs, name):
    g, o = ctxs(name)
    run_shares(g, o, name, "default")


# ---- 7: linear transforms ---------------------------------------------------------------------------------------------

def lt_elements(N):
    return [gal(N, 1), 1, 2 * N - 1, gal(N, -(N // 4 - 1))]


def linear_case(name):
    o = oracle(name)
    B = _batch(o)
    for nl in levels(name):
        random_case(o, name, nl, B, lt_elements(o.N))  # tests/test_linear_transform.py keeps it (read-only)
    return dict(B=B, vals=np.random.default_rng(1707).uniform(-1.0, 1.0, size=(2, o.N // 2)))


def run_linear(g, o, name, tag):
    case = cached(linear_case, name)
    N, L, K, B = g.N, g.L, g.K, case["B"]
    # encode_ext: the Q limbs are encode's; each P limb is the transform of the centred lift of limb 0's coefficients
    n, nl, scale = 2, min(L, 3), o.sf(1)
    d_vals, d_pt, d_ext = g.to_device(case["vals"]), g.empty((n, nl, N)), g.empty((n, nl + K, N))
    g.encode(d_vals, d_pt, n, nl, scale)
    g.encode_ext(d_vals, d_ext, n, nl, scale)
    pt, ext = d_pt.to_host(), d_ext.to_host()
    same(ext[:, :nl], pt, name, tag, "encode_ext, Q limbs")
    q0 = int(g.moduli[0])
    for b in range(n):
        c = o.ntt_inv(0, pt[b, 0]).astype(object)
        c = np.where(c > q0 // 2, c - q0, c)
        for k in range(K):
            want = o.ntt_fwd(L + k, np.array(c % int(g.moduli[L + k]), dtype=np.uint64))
            same(ext[b, nl + k], want, name, tag, "encode_ext, P limb", b, k)
    gs = lt_elements(N)
    for nl in levels(name):
        ct, evks, pts, want = random_case(o, name, nl, B, gs)
        got, d_ct = dev_lt(g, ct, evks, pts, gs, nl)
        same(got, want, name, tag, "linear_transform", nl)
        same(d_ct.to_host(), ct, name, tag, "linear_transform changed its input", nl)


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_linear_transforms(ctxs, name):
    g, o = ctxs(name)
    run_linear(g, o, name, "default")


SECTIONS = (test_plain_products_and_sums, test_weighted_aggregation, test_rotations, test_products, test_collective_keys,
            test_shares, test_linear_transforms)


def test_every_section_covers_every_table_entry():
    """No device needed: each section is parametrised over exactly the names of TABLE, and the subsets below are names of it."""
    for f in SECTIONS:
        over = [m.args[1] for m in f.pytestmark if m.name == "parametrize" and m.args[0] == "name"]
        assert len(over) == 1 and len(over[0]) == len(NAMES) and set(over[0]) == set(NAMES), f.__name__
        assert any(m.name == "gpu" for m in f.pytestmark), f.__name__
    assert set(BIG + tuple(EXTREME_LT) + tuple(EXTREME_KS) + ("dL",)) | {f[0] for f in FORKS} <= set(NAMES)
    fp_terms, pm_terms = tensor_cadences()
    assert TENSOR_TERMS > 2 * max(fp_terms, pm_terms)
    assert all(n > 0 for n in cadences())


# ---- extreme residues on the class patterns the table adds ---------------------------------------------------------------

LT_PATTERNS = ("q-1", "0/q-1", "outer")


def extreme_lt_inputs(o, nl, n_rot, pattern):
    """`extreme_case` of the feature test: every residue q - 1, or alternating 0 / q - 1.  "outer": uniform ciphertext and
    keys under plaintexts at q - 1 -- the inner sums of the first two are small or zero in half the rotations (constant
    and two-valued rows), these are uniform, so the outer sums take a product near q^2 / 2 in every rotation."""
    if pattern != "outer":
        return extreme_case(o, nl, n_rot, pattern == "0/q-1")
    rng = np.random.default_rng(1808)
    ids = list(range(nl)) + list(range(o.L, o.D))
    return rand_ct(rng, o, nl, 1), rand_evks(rng, o, n_rot), all_q_minus_1(o, ids, (n_rot,))


def extreme_lt_case(name):
    """One digit (nl = min(L, alpha)), more rotations than the longest run of any class between two folds, one unrotated
    term among them."""
    o = oracle(name)
    _, fp_rot, pm_rot = cadences()
    n_rot, nl = max(fp_rot, pm_rot) + 2, min(o.L, o.alpha)
    gs = [gal(o.N, r + 1) for r in range(n_rot)]
    gs[3] = 1
    case = dict(n_rot=n_rot, nl=nl, gs=gs)
    for pattern in LT_PATTERNS:
        ct, evks, pts = extreme_lt_inputs(o, nl, n_rot, pattern)
        case[pattern] = ref_linear_transform(o, ct[0], evks, pts, gs, nl)
    return case


@gpu
@pytest.mark.parametrize("pattern", LT_PATTERNS)
@pytest.mark.parametrize("name", EXTREME_LT)
def test_extreme_residues_through_the_linear_transform(ctxs, name, pattern):
    g, o = ctxs(name)
    case = cached(extreme_lt_case, name)
    _, fp_rot, pm_rot = cadences()
    assert case["n_rot"] > 2 * fp_rot and case["n_rot"] > pm_rot and g.alpha >= case["nl"]
    ct, evks, pts = extreme_lt_inputs(o, case["nl"], case["n_rot"], pattern)
    same(dev_lt(g, ct, evks, pts, case["gs"], case["nl"])[0][0], case[pattern], name, pattern)


def extreme_six_digit_case(name):
    o = oracle(name)
    gs = [gal(o.N, 1), 2 * o.N - 1]
    ct, evks, pts = extreme_case(o, o.L, len(gs), False)
    return dict(gs=gs, ct=ct, evks=evks, pts=pts, want=ref_linear_transform(o, ct[0], evks, pts, gs, o.L))


@gpu
def test_extreme_residues_past_the_inner_fold_on_six_digits(ctxs):
    """dL at nl = L: six digits and the c0 term, on fp64 limbs at N = 2^12, are more products than the fp64 inner sum takes
    between two reductions."""
    g, o = ctxs("dL")
    fp_terms, _, _ = cadences()
    assert g.beta == 6 and g.beta + 1 > fp_terms and FP64 in list(g.arith[:g.L])
    c = cached(extreme_six_digit_case, "dL")
    same(dev_lt(g, c["ct"], c["evks"], c["pts"], c["gs"], g.L)[0][0], c["want"], "dL")


def extreme_ks_case(name):
    """Every residue of ciphertexts and keys q - 1, at nl = L: the product through mult_relin, two clients at weight 1.0
    (M = sf: the largest constants) through reencrypt_wsum."""
    o = oracle(name)
    L, D = o.L, o.D
    ct = all_q_minus_1(o, list(range(L)), (1, 2))
    evk = all_q_minus_1(o, list(range(D)), (o.beta, 2))
    want = oracle_relinearize(o, py_tensor(o.moduli, ct, ct), evk)
    cts, evks = np.stack([ct, ct]), np.stack([evk, evk])
    scaled = np.stack([scaled_evk(o, evk, 1.0, 1)] * 2)
    return dict(ct=ct, evk=evk, relin=want[None], cts=cts, evks=evks, wsum=oracle_wsum(o, cts, scaled, [1.0, 1.0], 1, 0)[None])


@gpu
@pytest.mark.parametrize("name", EXTREME_KS)
def test_extreme_residues_through_mult_relin_and_reencrypt_wsum(ctxs, name):
    g, o = ctxs(name)
    c = cached(extreme_ks_case, name)
    L = g.L
    d_ct, d_out = g.to_device(c["ct"]), g.empty(c["ct"].shape)
    g.mult_relin(d_ct, g.to_device(c["ct"]), g.to_device(c["evk"]), d_out, 1, L)
    same(d_out.to_host(), c["relin"], name, "mult_relin")
    g.mult_relin(d_ct, d_ct, g.to_device(c["evk"]), d_out, 1, L)  # a is b: the square path
    same(d_out.to_host(), c["relin"], name, "mult_relin, square")
    got, _ = device_wsum(g, c["cts"], c["evks"], [1.0, 1.0], 1, L)
    same(got, c["wsum"], name, "reencrypt_wsum")


# ---- forks: the library switches on the entries whose classes they change -----------------------------------------------

FORK_SECTIONS = {"plain": run_plain, "products": run_products, "collective": run_collective, "shares": run_shares,
                 "linear": run_linear}


@gpu
@pytest.mark.parametrize("section", list(FORK_SECTIONS))
@pytest.mark.parametrize("name,switch,value,absent", FORKS)
def test_sections_under_the_library_switches(monkeypatch, name, switch, value, absent, section):
    """Switches are read once, when a context is created: the entry once more under the switch gives the reference's bits
    from the other arithmetic, or from the composed path."""
    from ppqsflhe_amd import Context
    args, shape, arith = TABLE[name]
    o = oracle(name)
    monkeypatch.setenv(switch, value)
    g2 = Context(args[0], args[1], args[2], device=0, **_kwargs(args))
    try:
        if absent is None:
            assert [int(x) for x in g2.arith] == arith, (name, switch, list(g2.arith))
        else:
            assert absent in arith and absent not in list(g2.arith), (name, switch, list(g2.arith))
        assert (g2.L, g2.K, g2.alpha, g2.beta) == shape and np.array_equal(g2.moduli, o.moduli), (name, switch)
        FORK_SECTIONS[section](g2, o, name, (switch, value))
    finally:
        g2.close()
