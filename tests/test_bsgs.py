"""Baby-step giant-step linear transforms (include/mkckks.h: mkckks_linear_transform_bsgs_batch; DESIGN.md section 4 "linear
transforms"; kernels: ppqsflhe_amd/csrc/bsgs_kernels.hpp and the LT_BABY / LT_GIANT modes of lintrans_kernels.hpp).

    out = sum_G rot_G( sum_b rot_{-G}(diag_{G+b}) * rot_b(x) )

`ref_bsgs` states the definition of the header in exact Python integers between the oracle's `modup_digits` and `moddown`,
the way tests/test_linear_transform.py's `ref_linear_transform` does; every device result is compared with it word for word.

Decoded values: the rescaled result must decode to sum_r diag_r * rot_r(x) within BSGS_BOUND = 4 x the largest error
`measure` gives for `ref_bsgs` on the CPU oracle over seeds 0 .. 5 at the same parameters and with the same plan (n1 = 2,
giants {0, +2, -2}, step 3 absent; max_j sum_r |diag_r[j]| <= 4).  Run `python -m tests.test_bsgs` to print the figures; they
are in DESIGN.md "linear transforms"; nothing in the bound comes from a GPU result:
    tiny: 2^-36.52 .. 2^-35.81
    ref:  2^-34.10 .. 2^-33.90
"""
import os
import re

import numpy as np
import pytest

from oracle.oracle import FastCpuContext
from tests.test_gpu_parity import CONFIGS, rand_ct, rand_polys
from tests.test_lattice_evaluation import NAMES, _batch, oracle
from tests.test_lattice_evaluation import ctxs as lattice_ctxs  # noqa: F401  (fixture)
from tests.test_linear_transform import (cadences, cpu_encode_ext, ctxs, dev_lt, ext_ids, new_context,  # noqa: F401  (ctxs: fixture)
                                         random_case)
from tests.test_rotation import gal, keyed_case, oracle_galois_key, rand_evks, src_index

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 4 x the largest of measure(name, seed) for seed 0 .. 5
BSGS_BOUND = {"tiny": 4 * 2.0 ** -35.81, "ref": 4 * 2.0 ** -33.90}
DECODE_STEPS = (-2, -1, 0, 1, 2)  # n1 = 2: giants -2, 0, 2; (2, 1) = step 3 is absent


def baby_group():
    """The larger of the babies and the giants k_bsgs_inner keeps in registers, read from its constants."""
    src = open(os.path.join(ROOT, "ppqsflhe_amd", "csrc", "bsgs_kernels.hpp")).read()
    return max(int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1)) for name in ("BSGS_GROUP", "BSGS_GIANTS"))


# ---- the definition in exact integers -----------------------------------------------------------------------------------

def ref_bsgs(o, ct, bkeys, gb, gkeys, gg, pts, present, nl):
    """ct u64[2][nl][N]; bkeys u64[n1][beta][2][D][N] and gkeys u64[n2][..] (slots of an element 1 are not read); pts[t, b]
    u64[nl+K][N] (an array or a dict of the present entries); present [n2][n1] -> u64[2][nl][N]."""
    N, ids = o.N, ext_ids(o, nl)
    n1, n2, ext = len(gb), len(gg), len(ids)
    mods = [int(o.moduli[lid]) for lid in ids]
    P = 1
    for k in range(o.L, o.D):
        P *= int(o.moduli[k])

    def key_sums(dig, keys, src):
        """(sum_j sigma(d_j[i]) kb_j[i], sum_j sigma(d_j[i]) ka_j[i]) per extended slot, not reduced"""
        sb, sa = [0] * ext, [0] * ext
        for i, lid in enumerate(ids):
            for j in range(dig.shape[0]):
                d = dig[j, i][src].astype(object)
                sb[i] = sb[i] + d * keys[j, 0, lid].astype(object)
                sa[i] = sa[i] + d * keys[j, 1, lid].astype(object)
        return sb, sa

    dig = o.modup_digits(np.ascontiguousarray(ct[1]))
    zero = np.zeros(N, dtype=object)
    babies = {}
    for b, g in enumerate(gb):
        if not any(present[t][b] for t in range(n2)):
            continue  # not computed
        if g == 1:
            Bb = [(P % mods[i]) * ct[0, i].astype(object) % mods[i] if i < nl else zero for i in range(ext)]
            Ba = [(P % mods[i]) * ct[1, i].astype(object) % mods[i] if i < nl else zero for i in range(ext)]
        else:
            src = src_index(N, g)
            sb, sa = key_sums(dig, bkeys[b], src)
            Bb = [(sb[i] + ((P % mods[i]) * ct[0, i][src].astype(object) if i < nl else 0)) % mods[i] for i in range(ext)]
            Ba = [sa[i] % mods[i] for i in range(ext)]
        babies[b] = (Bb, Ba)
    acc = [[zero] * ext, [zero] * ext]
    for t, g in enumerate(gg):
        cols = [b for b in range(n1) if present[t][b]]
        if not cols:
            continue  # costs nothing
        U = [[0] * ext, [0] * ext]
        for b in cols:
            pt = pts[t, b]
            for i in range(ext):
                p = pt[i].astype(object)
                for k in range(2):
                    U[k][i] = U[k][i] + p * babies[b][k][i]
        U = [[np.asarray(U[k][i] % mods[i], dtype=object) for i in range(ext)] for k in range(2)]
        if g == 1:
            add = U
        else:
            src = src_index(N, g)
            v = o.moddown(np.stack(U[1]).astype(np.uint64))
            sb, sa = key_sums(o.modup_digits(np.ascontiguousarray(v)), gkeys[t], src)
            add = [[U[0][i][src] + sb[i] for i in range(ext)], sa]
        acc = [[(acc[k][i] + add[k][i]) % mods[i] for i in range(ext)] for k in range(2)]
    return np.stack([o.moddown(np.stack(acc[k]).astype(np.uint64)) for k in range(2)])


def plans(N):
    """name -> (gb, gg, present).  2x3: giants {1, +, -} and one absent entry; 4x3: an empty giant row (the unrotated one)
    and an empty baby column; 1x3 / 1x2: one baby; conj: a conjugation giant; dup: duplicate elements in both lists."""
    return {
        "2x3": ([1, gal(N, 1)], [1, gal(N, 2), gal(N, -2)], [[1, 1], [1, 0], [1, 1]]),
        "4x3": ([1, gal(N, 1), gal(N, 2), gal(N, 3)], [gal(N, 4), 1, gal(N, -4)], [[1, 1, 0, 1], [0, 0, 0, 0], [0, 1, 0, 1]]),
        "1x3": ([1], [1, gal(N, 3), gal(N, -(N // 4 - 1))], [[1], [1], [1]]),
        "1x2": ([gal(N, 1)], [gal(N, 2), 1], [[1], [1]]),
        "conj": ([1, gal(N, 1)], [2 * N - 1, 1], [[1, 1], [1, 1]]),
        "dup": ([gal(N, 2), gal(N, 2), 1, 1], [gal(N, 4), gal(N, 4), 1], [[1, 1, 1, 0], [0, 1, 0, 1], [1, 1, 1, 1]]),
    }


_cases = {}


def bsgs_case(o, name, nl, B, plan):
    """Uniform random residues (the key slots of elements 1 and the plaintext slots of absent entries included: reading one
    changes the result) and the reference result; computed once and shared (read-only)."""
    key = (name, nl, B, plan)
    if key not in _cases:
        gb, gg, present = plans(o.N)[plan]
        rng = np.random.default_rng(4100 + 31 * nl + B + 7 * len(plan) + o.N.bit_length())
        ct, bkeys, gkeys = rand_ct(rng, o, nl, B), rand_evks(rng, o, len(gb)), rand_evks(rng, o, len(gg))
        pts = rand_polys(rng, o, ext_ids(o, nl), len(gg) * len(gb)).reshape(len(gg), len(gb), -1, o.N)
        want = np.stack([ref_bsgs(o, ct[b], bkeys, gb, gkeys, gg, pts, present, nl) for b in range(B)])
        for arr in (ct, bkeys, gkeys, pts, want):
            arr.setflags(write=False)
        _cases[key] = (ct, bkeys, gb, gkeys, gg, pts, present, want)
    return _cases[key]


def dev_bsgs(g, ct, bkeys, gb, gkeys, gg, pts, present, nl):
    B = ct.shape[0]
    d_ct, d_out = g.to_device(ct), g.empty(ct.shape)
    d_bk, d_gk = (None if k is None else g.to_device(k) for k in (bkeys, gkeys))
    g.linear_transform_bsgs(d_ct, d_bk, gb, d_gk, gg, g.to_device(pts), present, d_out, B, nl)
    return d_out.to_host(), d_ct


# ---- GPU ----------------------------------------------------------------------------------------------------------------

# (shape, nl, n_ct, plan): tiny at nl = L and at a partial last digit (alpha = 3); ref at 3; the ring below a tile with six
# digits and at 3 limbs; c5s (three digits, the last partial); n11 (integer arithmetic only); six14 (the fp64 inner fold);
# c3 at 5 limbs, one ciphertext; three ciphertexts on tiny and six9
BSGS_CASES = [("tiny", 5, 1, "2x3"), ("tiny", 4, 3, "4x3"), ("tiny", 5, 1, "1x3"), ("tiny", 4, 1, "conj"), ("tiny", 4, 1, "dup"),
              ("ref", 3, 1, "2x3"), ("six9", 6, 3, "2x3"), ("six9", 3, 1, "conj"), ("c5s", 15, 1, "2x3"), ("n11", 3, 1, "4x3"),
              ("six14", 6, 1, "2x3"), ("c3", 5, 1, "1x2")]


@gpu
@pytest.mark.parametrize("name,nl,B,plan", BSGS_CASES)
def test_bsgs_is_the_definition_bit_for_bit(ctxs, name, nl, B, plan):
    g, o = ctxs(name)
    ct, bkeys, gb, gkeys, gg, pts, present, want = bsgs_case(o, name, nl, B, plan)
    got, d_ct = dev_bsgs(g, ct, bkeys, gb, gkeys, gg, pts, present, nl)
    assert np.array_equal(got, want), (name, nl, plan)
    assert np.array_equal(d_ct.to_host(), ct)


@gpu
@pytest.mark.parametrize("name,nl,B", [("tiny", 4, 3), ("ref", 3, 1)])
def test_one_identity_giant_is_the_direct_transform(ctxs, name, nl, B):
    """n2 = 1 with h_gg[0] = 1: the words of linear_transform on the same keys, plaintexts and elements, on the device."""
    g, o = ctxs(name)
    N = g.N
    gs = [gal(N, -2), 1, gal(N, -(N // 4 - 1))]
    ct, evks, pts, want = random_case(o, name, nl, B, gs)
    direct = dev_lt(g, ct, evks, pts, gs, nl)[0]
    got = dev_bsgs(g, ct, evks, gs, None, [1], pts[None], [[1] * len(gs)], nl)[0]
    assert np.array_equal(got, direct) and np.array_equal(got, want)


@gpu
@pytest.mark.parametrize("name,nl", [("tiny", 4), ("ref", 3)])
@pytest.mark.parametrize("env", [{"MKCKKS_BSGS_FUSED": "0"}, {"MKCKKS_NO_FP64": "1"}, {"MKCKKS_NO_PM": "1"},
                                 {"MKCKKS_GENERIC_NTT": "1"}, {"MKCKKS_CHUNK": "1"}, {"MKCKKS_BSGS_WS_MIB": "1"}])
def test_bsgs_under_the_library_switches(ctxs, monkeypatch, env, name, nl):
    """Switches are read once, when a context is created: a fresh context under each gives the same bits.  Three
    ciphertexts are three chunks under MKCKKS_CHUNK=1 and under a workspace cap of 1 MiB (one ciphertext needs more)."""
    _, o = ctxs(name)
    B, plan = (3, "4x3") if name == "tiny" else (1, "2x3")
    ct, bkeys, gb, gkeys, gg, pts, present, want = bsgs_case(o, name, nl, B, plan)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    g = new_context(name)
    try:
        assert np.array_equal(dev_bsgs(g, ct, bkeys, gb, gkeys, gg, pts, present, nl)[0], want), (name, env)
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("name", ["tiny", "six9"])
def test_the_composition_arm_on_every_plan(ctxs, monkeypatch, name):
    """MKCKKS_BSGS_FUSED=0 on every plan the shape has above (the references are shared): the same bits."""
    _, o = ctxs(name)
    monkeypatch.setenv("MKCKKS_BSGS_FUSED", "0")
    g = new_context(name)
    try:
        for shape, nl, B, plan in BSGS_CASES:
            if shape != name:
                continue
            ct, bkeys, gb, gkeys, gg, pts, present, want = bsgs_case(o, name, nl, B, plan)
            assert np.array_equal(dev_bsgs(g, ct, bkeys, gb, gkeys, gg, pts, present, nl)[0], want), (name, nl, plan)
    finally:
        g.close()


def extreme_plan(N, n):
    """n x n, past every cadence: giant 0 (keyed) has every baby present, so its inner sums fold more than once in every
    class and walk more than one register group; giant t > 0 has baby t alone; the n giants fold the outer sums.  All but
    two babies and two giants are unrotated duplicates: the cadences count terms, and the reference stays quick."""
    gb = [gal(N, 1)] + [1] * (n - 2) + [gal(N, -1)]
    gg = [gal(N, 2)] + [1] * (n - 2) + [2 * N - 1]
    present = [[1] * n] + [[1 if b == t else 0 for b in range(n)] for t in range(1, n)]
    return gb, gg, present


def extreme_inputs(o, nl, n, alternating):
    ids, N = ext_ids(o, nl), o.N
    idx = np.arange(N)

    def poly(lid, phase):
        q1 = np.uint64(int(o.moduli[lid]) - 1)
        if not alternating:
            return np.full(N, q1, dtype=np.uint64)
        return np.where((idx + phase) % 2 == 0, q1, np.uint64(0))

    ct = np.stack([np.stack([poly(i, k) for i in range(nl)]) for k in range(2)])[None]
    key = np.stack([np.stack([np.stack([poly(lid, j + k) for lid in range(o.D)]) for k in range(2)]) for j in range(o.beta)])
    keys = np.stack([key, np.roll(key, 1, axis=-1)])  # the two keyed elements of a list
    pts = [np.stack([poly(lid, r) for lid in ids]) for r in range(2)]
    return np.ascontiguousarray(ct), keys, pts


_extreme = {}


def extreme_case(o, name, nl, alternating):
    key = (name, nl, alternating)
    if key not in _extreme:
        fp_terms, fp_rot, pm_rot = cadences()
        n = max(fp_rot, pm_rot, baby_group()) + 2
        assert n > 2 * fp_rot and n > pm_rot and n > 2 * baby_group()
        gb, gg, present = extreme_plan(o.N, n)
        ct, keys, pt2 = extreme_inputs(o, nl, n, alternating)
        pts = {(t, b): pt2[(t + b) % 2] for t in range(n) for b in range(n) if present[t][b]}
        kslot = {0: 0, n - 1: 1}
        view = type("Keys", (), {"__getitem__": lambda self, k: keys[kslot[k]]})()  # the keys of slots 0 and n - 1
        want = ref_bsgs(o, ct[0], view, gb, view, gg, pts, present, nl)
        _extreme[key] = (n, ct, keys, kslot, gb, gg, pts, present, want)
    return _extreme[key]


@gpu
@pytest.mark.parametrize("alternating", [False, True])
@pytest.mark.parametrize("name,nl", [("tiny", 2), ("six14", 6)])
def test_extreme_residues_past_every_cadence(ctxs, name, nl, alternating):
    """Every word m_i - 1, and alternating 0 / m_i - 1: tiny at a one-digit level (all three classes), six14 with six
    digits (the fp64 inner fold under the baby and the giant sums).  The plaintext slots of absent entries are never
    written: the device array has them, the test uploads the present ones only."""
    g, o = ctxs(name)
    n, ct, keys, kslot, gb, gg, pts, present, want = extreme_case(o, name, nl, alternating)
    N, ext = g.N, nl + g.K
    d_keys = g.empty((n,) + keys.shape[1:])
    for slot, k in kslot.items():
        d_keys.view(slot * keys[0].size, keys[0].shape).upload(keys[k])
    d_pts = g.empty((n, n, ext, N))
    for (t, b), pt in pts.items():
        d_pts.view((t * n + b) * ext * N, (ext, N)).upload(pt)
    d_ct, d_out = g.to_device(ct), g.empty(ct.shape)
    g.linear_transform_bsgs(d_ct, d_keys, gb, d_keys, gg, d_pts, present, d_out, 1, nl)
    assert np.array_equal(d_out.to_host()[0], want)


@gpu
def test_neighbours_of_the_output_and_empty_calls(ctxs):
    """Poisoned words around the output stay; n_ct = 0 and a plan without a present entry write nothing."""
    POISON = 0xA5A5A5A5A5A5A5A5
    g, o = ctxs("tiny")
    N, nl, B = g.N, 4, 3
    ct, bkeys, gb, gkeys, gg, pts, present, want = bsgs_case(o, "tiny", nl, B, "4x3")
    words = B * 2 * nl * N
    d_big = g.to_device(np.full(words + 4 * N, POISON, dtype=np.uint64))
    d_out = d_big.view(2 * N, ct.shape)
    d_ct, d_bk, d_gk, d_pts = g.to_device(ct), g.to_device(bkeys), g.to_device(gkeys), g.to_device(pts)
    g.linear_transform_bsgs(d_ct, d_bk, gb, d_gk, gg, d_pts, present, d_out, B, nl)
    big = d_big.to_host()
    assert np.array_equal(big[2 * N:2 * N + words].reshape(ct.shape), want)
    assert np.all(big[:2 * N] == POISON) and np.all(big[2 * N + words:] == POISON)
    assert np.array_equal(d_ct.to_host(), ct)
    g.linear_transform_bsgs(d_ct, d_bk, gb, d_gk, gg, d_pts, present, d_out, 0, nl)
    g.linear_transform_bsgs(d_ct, d_bk, gb, d_gk, gg, d_pts, [[0] * len(gb)] * len(gg), d_out, B, nl)
    assert np.array_equal(d_big.to_host(), big)


def region_case(name):
    o = oracle(name)
    return bsgs_case(o, name, o.L, 1, "2x3")


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_bsgs_on_every_parameter_region(lattice_ctxs, name):
    """One case per parameter region of tests/test_parameter_lattice.py's TABLE, at nl = L."""
    g, o = lattice_ctxs(name)
    ct, bkeys, gb, gkeys, gg, pts, present, want = region_case(name)
    got, _ = dev_bsgs(g, ct, bkeys, gb, gkeys, gg, pts, present, g.L)
    assert np.array_equal(got, want), name


# ---- decoded values -----------------------------------------------------------------------------------------------------

def decode_case(o, seed):
    """Keys for the plan's steps, five diagonals (step 3 absent), their rolled plaintexts at sf(1) and the expected values."""
    N, L = o.N, o.L
    gb_steps, gg_steps = (0, 1), (0, 2, -2)
    case = keyed_case(o, seed, [1, 2, -2])
    diags = {r: case["rng"].uniform(-0.8, 0.8, size=N // 2) for r in DECODE_STEPS}
    assert np.abs(np.stack(list(diags.values()))).sum(axis=0).max() <= 4
    case["gb"], case["gg"] = [gal(N, b) for b in gb_steps], [gal(N, G) for G in gg_steps]
    case["present"] = [[1 if G + b in diags else 0 for b in gb_steps] for G in gg_steps]
    # the plaintext of (G, b): diag_{G+b} rolled right by G
    case["rolled"] = np.stack([np.stack([np.roll(diags[G + b], G) if G + b in diags else np.zeros(N // 2) for b in gb_steps])
                               for G in gg_steps])
    zero = np.zeros((o.beta, 2, o.D, N), dtype=np.uint64)
    case["bkeys"] = np.stack([oracle_galois_key(o, case, b) if b else zero for b in gb_steps])
    case["gkeys"] = np.stack([oracle_galois_key(o, case, G) if G else zero for G in gg_steps])
    case["want"] = sum(d * np.roll(case["vals"], -r) for r, d in diags.items())
    case["scale"] = o.sf_big(0) * o.sf(1) / float(o.moduli[L - 1])
    return case


def measure(name, seed):
    """max over the slots of |decoded - expected| of the integer definition on the CPU oracle, rescaled once."""
    a = CONFIGS[name]
    o = FastCpuContext(a[0], a[1], a[2], a[3], dnum=a[4])
    case = decode_case(o, seed)
    pts = np.stack([np.stack([cpu_encode_ext(o, v, o.sf(1), o.L) for v in row]) for row in case["rolled"]])
    out = ref_bsgs(o, case["ct"], case["bkeys"], case["gb"], case["gkeys"], case["gg"], pts, case["present"], o.L)
    return np.abs(o.decrypt_decode(o.rescale(out), case["sk"], case["scale"]) - case["want"]).max()


@gpu
@pytest.mark.parametrize("name", ["tiny", "ref"])
def test_decoded_values_of_a_bsgs_transform(ctxs, name):
    """Real encode / encrypt under a generated key, the oracle's Galois keys; the rolled diagonals encoded over the extended
    basis, the transform and the rescale on the device; decryption and decoding on the oracle."""
    g, o = ctxs(name)
    N, L = g.N, g.L
    case = decode_case(o, 5)
    n2, n1 = len(case["gg"]), len(case["gb"])
    d_pts = g.empty((n2, n1, L + g.K, N))
    g.encode_ext(g.to_device(case["rolled"].reshape(n2 * n1, N // 2)), d_pts, n2 * n1, L, o.sf(1))
    d_ct, d_out, d_res = g.to_device(case["ct"][None]), g.empty((1, 2, L, N)), g.empty((1, 2, L - 1, N))
    g.linear_transform_bsgs(d_ct, g.to_device(case["bkeys"]), case["gb"], g.to_device(case["gkeys"]), case["gg"], d_pts,
                            case["present"], d_out, 1, L)
    g.rescale(d_out, d_res, 1, L)
    err = np.abs(o.decrypt_decode(d_res.to_host()[0], case["sk"], case["scale"]) - case["want"]).max()
    print(f"{name}: bsgs transform error 2^{np.log2(err):.2f}, bound 2^{np.log2(BSGS_BOUND[name]):.2f}")
    assert err <= BSGS_BOUND[name], (name, err)


if __name__ == "__main__":
    for cfg in ("tiny", "ref"):
        errs = [measure(cfg, seed) for seed in range(6)]
        for seed, e in enumerate(errs):
            print(f"{cfg} seed {seed}: 2^{np.log2(e):.2f}")
        print(f"{cfg}: 2^{np.log2(min(errs)):.2f} .. 2^{np.log2(max(errs)):.2f}")
