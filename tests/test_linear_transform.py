"""Encrypted linear transforms by diagonals, double hoisted (include/mkckks.h: "linear transforms by diagonals"; DESIGN.md
section 4 "linear transforms"; kernel: ppqsflhe_amd/csrc/lintrans_kernels.hpp).

    out[j] = sum_r diag_r[j] * in[(j + r) mod N/2]

Definition, bit for bit (m_i: modulus of extended slot i, d_j: the digits of c1, sigma_g: the gather `src_index`):

    A_b[i] = sum_r pt_r[i] ( sum_j sigma_{g_r}(d_j[i]) kb_{r,j}[i] + [i < nl] [P]_{q_i} sigma_{g_r}(c0[i]) )  mod m_i
    A_a[i] = sum_r pt_r[i] ( sum_j sigma_{g_r}(d_j[i]) ka_{r,j}[i] )                                          mod m_i
    (g_r = 1: the inner key sum is [i < nl] [P]_{q_i} c1[i] in A_a and absent from A_b)
    out = ( ModDown(A_b), ModDown(A_a) )

`ref_linear_transform` states it in exact integers between the oracle's ModUp and ModDown; every device result is compared
with it word for word.

Decoded values: the rescaled result must decode to sum_r diag_r * rot_r(x) within LT_BOUND = 4 x the largest error
`measure` gives for `ref_linear_transform` on the CPU oracle over seeds 0 .. 5 at the same parameters (run
`python -m tests.test_linear_transform` to print the figures; they are in DESIGN.md "linear transforms"); nothing in the bound
comes from a GPU result.  Beside it, the error of the composition (rotate, multiply, sum, rescale) on the CPU oracle:
    tiny: double hoisted 2^-36.74 .. 2^-36.39, composition 2^-36.74 .. 2^-36.39
    ref:  double hoisted 2^-34.19 .. 2^-33.80, composition 2^-34.19 .. 2^-33.80
The two agree to the printed digits at these parameters: with four diagonals at a 40-bit scale the error of both is the
rounding of the encoded diagonals and of the rescale, far above the key-switch noise that double hoisting enters once
instead of once per diagonal.
"""
import os
import re

import numpy as np
import pytest

from oracle.oracle import FastCpuContext, OracleContext
from tests.test_gpu_parity import CONFIGS, make_keys, rand_ct, rand_polys  # noqa: F401  (make_keys: through keyed_case)
from tests.test_rotation import gal, keyed_case, oracle_galois_key, oracle_rotate, rand_evks, src_index
from tests.test_slot_weights import py_product

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 4 x the largest of measure(name, seed)[0] for seed 0 .. 5
LT_BOUND = {"tiny": 4 * 2.0 ** -36.39, "ref": 4 * 2.0 ** -33.80}
STEPS = (0, 1, -3, 7)


def cadences():
    """The fold cadences of the kernel's arithmetic classes, read from its constants."""
    src = open(os.path.join(ROOT, "ppqsflhe_amd", "csrc", "lintrans_kernels.hpp")).read()
    m = re.search(r"LT_FP_TERMS = (\d+), LT_FP_ROT = (\d+), LT_PM_ROT = (\d+);", src)
    return tuple(int(x) for x in m.groups())


# ---- the definition in exact integers -----------------------------------------------------------------------------------

def ext_ids(o, nl):
    return list(range(nl)) + list(range(o.L, o.D))


def ref_linear_transform(o, ct, evks, pts, gs, nl):
    """ct u64[2][nl][N], evks u64[n_rot][beta][2][D][N], pts u64[n_rot][nl+K][N], gs: Galois elements -> u64[2][nl][N]."""
    N, ids = o.N, ext_ids(o, nl)
    dig = o.modup_digits(np.ascontiguousarray(ct[1]))
    P = 1
    for k in range(o.L, o.D):
        P *= int(o.moduli[k])
    acc = np.zeros((2, len(ids), N), dtype=object)
    for r, g in enumerate(gs):
        src = src_index(N, g)
        for i, lid in enumerate(ids):
            m = int(o.moduli[lid])
            if g == 1:
                if i >= nl:
                    continue
                inner = [(P % m) * ct[0, i].astype(object), (P % m) * ct[1, i].astype(object)]
            else:
                inner = [0, 0]
                for j in range(dig.shape[0]):
                    d = dig[j, i][src].astype(object)
                    inner[0] = inner[0] + d * evks[r, j, 0, lid].astype(object)
                    inner[1] = inner[1] + d * evks[r, j, 1, lid].astype(object)
                if i < nl:
                    inner[0] = inner[0] + (P % m) * ct[0, i][src].astype(object)
            pt = pts[r, i].astype(object)
            for k in range(2):
                acc[k, i] = (acc[k, i] + pt * (inner[k] % m)) % m
    return np.stack([o.moddown(acc[k].astype(np.uint64)) for k in range(2)])


def cpu_encode_ext(o, vals, scale, nl):
    """encode over the extended basis: the Q limbs of o.encode, the P limbs from the centred lift of limb 0."""
    pt = o.encode(vals, scale, nl)
    q0 = int(o.moduli[0])
    c = o.ntt_inv(0, pt[0]).astype(object)
    c = np.where(c > q0 // 2, c - q0, c)
    ext = [pt[i] for i in range(nl)]
    for k in range(o.L, o.D):
        ext.append(o.ntt_fwd(k, np.array(c % int(o.moduli[k]), dtype=np.uint64)))
    return np.stack(ext)


def lt_case(o, seed):
    """Keys for STEPS, diagonals, their plaintexts at sf(1) and the expected values."""
    case = keyed_case(o, seed, [r for r in STEPS if r])
    N, L = o.N, o.L
    diags = case["rng"].uniform(-1.0, 1.0, size=(len(STEPS), N // 2))
    case["diags"] = diags
    case["pts"] = np.stack([cpu_encode_ext(o, d, o.sf(1), L) for d in diags])
    case["gs"] = [gal(N, r) for r in STEPS]
    case["want"] = sum(diags[k] * np.roll(case["vals"], -r) for k, r in enumerate(STEPS))
    case["scale"] = o.sf_big(0) * o.sf(1) / float(o.moduli[L - 1])
    return case


def measure(name, seed):
    """(error of the double-hoisted transform, error of the composition): max over the slots of |decoded - expected| on the
    CPU oracle, both rescaled once."""
    a = CONFIGS[name]
    o = FastCpuContext(a[0], a[1], a[2], a[3], dnum=a[4])
    L = o.L
    case = lt_case(o, seed)
    evks = np.stack([oracle_galois_key(o, case, r) if r else np.zeros((o.beta, 2, o.D, o.N), dtype=np.uint64)
                     for r in STEPS])
    out = ref_linear_transform(o, case["ct"], evks, case["pts"], case["gs"], L)
    e_lt = np.abs(o.decrypt_decode(o.rescale(out), case["sk"], case["scale"]) - case["want"]).max()
    comp = None
    for k, r in enumerate(STEPS):
        rot = oracle_rotate(o, case["ct"], evks[k], case["gs"][k]) if r else case["ct"]
        term = py_product(o, rot, case["pts"][k][:L])
        comp = term if comp is None else o.eval_add(comp, term)
    e_comp = np.abs(o.decrypt_decode(o.rescale(comp), case["sk"], case["scale"]) - case["want"]).max()
    return e_lt, e_comp


# ---- GPU ----------------------------------------------------------------------------------------------------------------

# name: the Context arguments; the names of CONFIGS and two shapes of tests/test_digit_shapes.py (six digits of one limb)
SHAPES = dict(CONFIGS)
SHAPES["six9"] = (9, 4, 50, 60, 6)    # a ring below one tile (512 words), six digits, integer arithmetic only
SHAPES["six14"] = (14, 4, 50, 60, 6)  # six digits on a ring with fp64-class limbs: the inner sum passes its fold


def new_context(name):
    from ppqsflhe_amd import Context
    a = SHAPES[name]
    return Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)


@pytest.fixture(scope="module")
def ctxs():
    cache = {}

    def get(name):
        if name not in cache:
            a = SHAPES[name]
            cls = FastCpuContext if name in CONFIGS else OracleContext
            cache[name] = (new_context(name), cls(a[0], a[1], a[2], a[3], dnum=a[4]))
        return cache[name]

    yield get
    for g, _ in cache.values():
        g.close()


def dev_lt(g, ct, evks, pts, gs, nl):
    B = ct.shape[0]
    d_ct, d_out = g.to_device(ct), g.empty(ct.shape)
    g.linear_transform(d_ct, g.to_device(evks), g.to_device(pts), gs, d_out, B, nl)
    return d_out.to_host(), d_ct


def element_sets(N):
    return {"id": [1], "pos": [gal(N, 1), gal(N, 3)], "neg": [gal(N, -2), 1, gal(N, -(N // 4 - 1))],
            "conj": [2 * N - 1, gal(N, 5)], "dup": [gal(N, 2), gal(N, 2), 1, 1]}


_cases = {}


def random_case(o, name, nl, B, gs):
    """Uniform random residues and the reference result; computed once and shared (read-only)."""
    key = (name, nl, B, tuple(gs))
    if key not in _cases:
        rng = np.random.default_rng(900 + 17 * nl + B + len(gs) + o.N.bit_length())
        ct, evks = rand_ct(rng, o, nl, B), rand_evks(rng, o, len(gs))
        pts = rand_polys(rng, o, ext_ids(o, nl), len(gs))
        want = np.stack([ref_linear_transform(o, ct[b], evks, pts, gs, nl) for b in range(B)])
        for arr in (ct, evks, pts, want):
            arr.setflags(write=False)
        _cases[key] = (ct, evks, pts, want)
    return _cases[key]


# (shape, nl, n_ct, element set): tiny at nl = L and at a partial last digit (alpha = 3), every element set; ref at 3; the
# ring below a tile; c5s (alpha = 7: three digits, the last partial); c3 at 5 limbs; n11 (integer arithmetic only); the
# six-digit shapes
LT_CASES = [("tiny", 5, 1, "pos"), ("tiny", 4, 3, "neg"), ("tiny", 5, 1, "id"), ("tiny", 4, 1, "conj"), ("tiny", 2, 3, "dup"),
            ("ref", 3, 1, "neg"), ("six9", 6, 3, "neg"), ("six9", 3, 1, "conj"), ("c5s", 15, 1, "pos"), ("c3", 5, 1, "pos"),
            ("n11", 3, 3, "neg"), ("six14", 6, 1, "conj")]


@gpu
@pytest.mark.parametrize("name,nl,B,which", LT_CASES)
def test_linear_transform_is_the_definition_bit_for_bit(ctxs, name, nl, B, which):
    g, o = ctxs(name)
    gs = element_sets(g.N)[which]
    ct, evks, pts, want = random_case(o, name, nl, B, gs)
    got, d_ct = dev_lt(g, ct, evks, pts, gs, nl)
    assert np.array_equal(got, want), (name, nl, which)
    assert np.array_equal(d_ct.to_host(), ct)


@gpu
@pytest.mark.parametrize("name,nl", [("tiny", 4), ("ref", 3)])
@pytest.mark.parametrize("env", [{"MKCKKS_NO_FP64": "1"}, {"MKCKKS_NO_PM": "1"}, {"MKCKKS_GENERIC_NTT": "1"}, {"MKCKKS_CHUNK": "1"},
                                 {"MKCKKS_LT_ORDER": "1"}, {"MKCKKS_LT_ORDER": "2"}])
def test_linear_transform_under_the_library_switches(ctxs, monkeypatch, env, name, nl):
    """Switches are read once, when a context is created: a fresh context under each gives the same bits.  Three
    ciphertexts are more than one chunk under MKCKKS_CHUNK=1 and a walk of three under MKCKKS_LT_ORDER=1."""
    _, o = ctxs(name)
    B = 3 if name == "tiny" else 1
    gs = element_sets(o.N)["neg"]
    ct, evks, pts, want = random_case(o, name, nl, B, gs)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    g = new_context(name)
    try:
        assert np.array_equal(dev_lt(g, ct, evks, pts, gs, nl)[0], want), (name, env)
    finally:
        g.close()


def extreme_case(o, nl, n_rot, alternating):
    ids, N = ext_ids(o, nl), o.N
    idx = np.arange(N)

    def poly(lid, phase):
        q1 = np.uint64(int(o.moduli[lid]) - 1)
        if not alternating:
            return np.full(N, q1, dtype=np.uint64)
        return np.where((idx + phase) % 2 == 0, q1, np.uint64(0))

    ct = np.stack([np.stack([poly(i, k) for i in range(nl)]) for k in range(2)])[None]
    evks = np.stack([np.stack([np.stack([np.stack([poly(lid, r + j + k) for lid in range(o.D)]) for k in range(2)])
                               for j in range(o.beta)]) for r in range(n_rot)])
    pts = np.stack([np.stack([poly(lid, r) for lid in ids]) for r in range(n_rot)])
    return np.ascontiguousarray(ct), evks, pts


@gpu
@pytest.mark.parametrize("alternating", [False, True])
def test_extreme_residues_past_every_fold_cadence(ctxs, alternating):
    """tiny at a one-digit level: ciphertext, keys and plaintexts all q - 1, and alternating 0 / q - 1, with more rotations
    than the longest run of any class between two folds (the outer sums of fp64 and pseudo-Mersenne limbs fold more than
    once); one unrotated term among them."""
    g, o = ctxs("tiny")
    fp_terms, fp_rot, pm_rot = cadences()
    n_rot, nl = max(fp_rot, pm_rot) + 2, 2
    assert n_rot > 2 * fp_rot and g.alpha >= nl
    gs = [gal(g.N, r + 1) for r in range(n_rot)]
    gs[3] = 1
    ct, evks, pts = extreme_case(o, nl, n_rot, alternating)
    want = ref_linear_transform(o, ct[0], evks, pts, gs, nl)
    assert np.array_equal(dev_lt(g, ct, evks, pts, gs, nl)[0][0], want)


@gpu
def test_extreme_residues_past_the_inner_fold(ctxs):
    """Six digits and the c0 term are more products than the fp64 inner sum takes between two reductions."""
    g, o = ctxs("six14")
    fp_terms, _, _ = cadences()
    nl = g.L
    assert g.beta + 1 > fp_terms and g.beta == 6
    gs = [gal(g.N, 1), 2 * g.N - 1]
    ct, evks, pts = extreme_case(o, nl, len(gs), False)
    want = ref_linear_transform(o, ct[0], evks, pts, gs, nl)
    assert np.array_equal(dev_lt(g, ct, evks, pts, gs, nl)[0][0], want)


@gpu
def test_neighbours_of_the_output_and_empty_calls(ctxs):
    """Poisoned words around the output stay; n_rot = 0 and n_ct = 0 write nothing."""
    POISON = 0xA5A5A5A5A5A5A5A5
    g, o = ctxs("tiny")
    N, nl, B = g.N, 4, 3
    gs = element_sets(N)["neg"]
    ct, evks, pts, want = random_case(o, "tiny", nl, B, gs)
    words = B * 2 * nl * N
    d_big = g.to_device(np.full(words + 4 * N, POISON, dtype=np.uint64))
    d_out = d_big.view(2 * N, ct.shape)
    d_ct, d_evks, d_pts = g.to_device(ct), g.to_device(evks), g.to_device(pts)
    g.linear_transform(d_ct, d_evks, d_pts, gs, d_out, B, nl)
    big = d_big.to_host()
    assert np.array_equal(big[2 * N:2 * N + words].reshape(ct.shape), want)
    assert np.all(big[:2 * N] == POISON) and np.all(big[2 * N + words:] == POISON)
    assert np.array_equal(d_ct.to_host(), ct)
    g.linear_transform(d_ct, d_evks, d_pts, [], d_out, B, nl)
    g.linear_transform(d_ct, d_evks, d_pts, gs, d_out, 0, nl)
    assert np.array_equal(d_big.to_host(), big)


@gpu
@pytest.mark.parametrize("name", ["tiny", "ref", "c3"])
def test_encode_ext_extends_encode(ctxs, name):
    """The Q limbs are encode_batch's; each P limb is the transform of the centred lift of limb 0's coefficients."""
    g, o = ctxs(name)
    N, K, n = g.N, g.K, 2
    nl = min(g.L, 3)
    rng = np.random.default_rng(41)
    vals = rng.uniform(-1.0, 1.0, size=(n, N // 2))
    scale = o.sf(1)
    d_vals = g.to_device(vals)
    d_pt, d_ext = g.empty((n, nl, N)), g.empty((n, nl + K, N))
    g.encode(d_vals, d_pt, n, nl, scale)
    g.encode_ext(d_vals, d_ext, n, nl, scale)
    pt, ext = d_pt.to_host(), d_ext.to_host()
    assert np.array_equal(ext[:, :nl], pt)
    q0 = int(g.moduli[0])
    for b in range(n):
        c = o.ntt_inv(0, pt[b, 0]).astype(object)
        c = np.where(c > q0 // 2, c - q0, c)
        for k in range(K):
            lid = g.L + k
            want = o.ntt_fwd(lid, np.array(c % int(g.moduli[lid]), dtype=np.uint64))
            assert np.array_equal(ext[b, nl + k], want), (name, b, k)


@gpu
@pytest.mark.parametrize("name", ["tiny", "ref"])
def test_decoded_values_of_a_linear_transform(ctxs, name):
    """Real encode / encrypt under a generated key, the oracle's Galois keys; the diagonals encoded over the extended basis
    and the transform and the rescale on the device; decryption and decoding on the oracle."""
    g, o = ctxs(name)
    N, L = g.N, g.L
    case = lt_case(o, 5)
    evks = np.stack([oracle_galois_key(o, case, r) if r else np.zeros((o.beta, 2, o.D, N), dtype=np.uint64) for r in STEPS])
    d_pts = g.empty((len(STEPS), L + g.K, N))
    g.encode_ext(g.to_device(case["diags"]), d_pts, len(STEPS), L, o.sf(1))
    d_ct, d_out, d_res = g.to_device(case["ct"][None]), g.empty((1, 2, L, N)), g.empty((1, 2, L - 1, N))
    g.linear_transform(d_ct, g.to_device(evks), d_pts, case["gs"], d_out, 1, L)
    g.rescale(d_out, d_res, 1, L)
    err = np.abs(o.decrypt_decode(d_res.to_host()[0], case["sk"], case["scale"]) - case["want"]).max()
    print(f"{name}: linear transform error 2^{np.log2(err):.2f}, bound 2^{np.log2(LT_BOUND[name]):.2f}")
    assert err <= LT_BOUND[name], (name, err)


if __name__ == "__main__":
    for cfg in ("tiny", "ref"):
        errs = [measure(cfg, seed) for seed in range(6)]
        for seed, (el, ec) in enumerate(errs):
            print(f"{cfg} seed {seed}: double hoisted 2^{np.log2(el):.2f}, composition 2^{np.log2(ec):.2f}")
        print(f"{cfg}: double hoisted 2^{np.log2(min(e[0] for e in errs)):.2f} .. 2^{np.log2(max(e[0] for e in errs)):.2f}, "
              f"composition 2^{np.log2(min(e[1] for e in errs)):.2f} .. 2^{np.log2(max(e[1] for e in errs)):.2f}")
