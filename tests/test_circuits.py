"""Chained evaluation circuits: the output of one evaluation entry point is the input of the next.

The feature modules compare every entry point with exact Python integers on fresh or random ciphertexts at the standard scale of
their level.  This module composes the same references (ref_linear_transform, ref_bsgs, cpu_poly_eval, cpu_cheb_eval,
oracle_slot_sum, oracle_wsum, py_tensor, oracle_relinearize, the oracle's rescale / encode / decrypt_decode) into chains and
compares the device word for word after every step, and the decoded values with numpy float64 of the circuit on the slots.

One shape of its own, `chain` = (log_n 10, depth 6, 40-bit scaling, 60-bit first, dnum 2): 8 Q limbs, deep enough for
transform -> degree-3 polynomial -> transform -> product, small enough for Python integers.  Arithmetic classes and ring splits
are tests/test_lattice_*.py's business.

A. Off-standard scales.  poly_weights / cheb_weights / powers / cheb_ladder / poly_eval / cheb_eval with scale_in =
   sf(L - nl) f, f in {1 - 2^-12, 1 + 2^-20, 0.75, 1.5}, with the neighbouring levels' scales sf(L - nl -+ 1) at this limb
   count, and with the scale of a level cut (a standard ciphertext of 6 limbs read at 5).  At nl = L, where sf(0) is the
   scale of the 20-bit extra limb, the fresh scale sf_big(0) f is used beside it.  Host side on `chain` and `tiny`, to the last
   bit against py_weights / py_cheb_weights / py_ladder, with the refusals the restatements predict; device side on `chain`
   at nl = 6, words against cpu_poly_eval / cpu_cheb_eval called with that scale, inputs really encrypted at that scale.
B. Circuits (values uniform in [-1, 1], sum_r |diag_r[j]| <= 1, coefficients TANH[:4] / the degree-7 Chebyshev fit of tanh):
   1  fresh -> rescale -> linear_transform (steps 0, 1, -3) -> rescale -> poly_eval degree 3       (3 ciphertexts)
   1c the same with cheb_eval degree 7 on [-1, 1] as its last step
   2  fresh -> rescale -> poly_eval degree 3 -> linear_transform_bsgs (n1 = 2, giants {0, +2, -2}, step 3 absent; a
      noiseScaleDeg-1 input: no rescale before it) -> rescale -> slot_sum span 4 -> mult_relin with itself -> rescale
   3  three clients, scale_evk + reencrypt_wsum with weights (0.5, 0.3, 0.2) -> rescale -> rescale -> cheb_eval degree 7 on
      [-2, 3].  The weighted sum's rescale (hostlib.hpp scale_aggregate) leaves a noiseScaleDeg-2 aggregate of about 2^80 on 7
      limbs; evalPoly rescales such an input once more before it evaluates, and so does the circuit: at 2^80 the map of
      [-2, 3] onto [-1, 1] would have the constant rint(0.4) = 0, and the CPU chain itself decodes to a constant.
   Scales follow the hosts' header rules (ppqsflhe_amd/host: linearTransform.cpp, poly.hpp, product.hpp, hostlib.hpp
   scale_aggregate), in their order of double operations.  The word references upload the plaintexts of cpu_encode_ext (the
   device's encoder agrees with the oracle's only to scale * 2^-50, tests/test_gpu_parity.py); circuit 1 runs once more with the
   device's encode_ext for the decoded values.
C. State.  One Engine owns three grow-only arenas, the Galois-element buffers, a flag and four caches: the circuits in the
   orders (1, 2, 3) and (3, 2, 1) on one context and on fresh ones; small calls after calls that grew every arena, into
   buffers of all-ones words; refused calls between the steps of circuit 2; circuit 2 under MKCKKS_CHUNK=1 and
   MKCKKS_BSGS_WS_MIB=1.  Always the reference's words.

Bounds: 4 x the largest error of the same circuit on the CPU restatement chain over seeds 0 .. 5 at the same parameters (the
project's margin for the seed-to-seed spread of a slot maximum); `python -m tests.test_circuits` prints them.  Nothing in a bound
comes from a GPU result.  Measured on the CPU chains, seeds 0 .. 5:
    circuit 1:                2^-29.92 .. 2^-29.13
    circuit 1c:               2^-29.91 .. 2^-29.21
    circuit 2:                2^-26.01 .. 2^-24.06
    circuit 3:                2^-29.07 .. 2^-28.24
    A poly 3 (all scales):    2^-26.57 .. 2^-26.01    (section A encrypts at about 2^40 on 6 limbs: the fresh noise is
    A poly 7:                 2^-26.53 .. 2^-26.14     2^19 times larger against the scale than under sf_big(0))
    A cheb 7 on [-1, 1]:      2^-26.55 .. 2^-25.80
    A cheb 7 on [-2, 3]:      2^-26.89 .. 2^-26.03

Teeth ("Chained circuits"): poly_weights / cheb_weights starting their ladder from sf(L - nl) instead of
scale_in fails test_weights_and_ladder_scales_follow_the_scale_they_are_given on both shapes, without a device.

Wall time on an MI355X: the 14 GPU tests of the file 2.5 s, the CPU chains they share included (built once per module, read-only);
the 5 device-free tests 0.5 s on a CPU.
"""
import numpy as np
import pytest
from numpy.polynomial import chebyshev as npcheb

from oracle.oracle import FastCpuContext, sample_gauss, sample_ternary
from tests.test_bsgs import ref_bsgs
from tests.test_cheb import cpu_cheb_eval
from tests.test_cheb_surface import py_cheb_rewrite, py_cheb_weights
from tests.test_gpu_parity import CONFIGS, make_keys, make_rk_rand
from tests.test_lattice_evaluation import _freeze, cached  # noqa: F401  (_freeze: cached's)
from tests.test_lattice_poly import REFUSAL, cheb_refusal, ladder_fits, poly_refusal
from tests.test_linear_transform import cpu_encode_ext, ref_linear_transform
from tests.test_poly import TANH, cpu_poly_eval
from tests.test_poly_surface import py_ladder, py_plan, py_weights
from tests.test_product import oracle_relin_key, oracle_relinearize, py_tensor
from tests.test_rotation import gal, oracle_slot_sum, sigma_coeff
from tests.test_weighted_aggregation import oracle_wsum, scaled_evk

gpu = pytest.mark.gpu

CHAIN = (10, 6, 40, 60, 2)
SHAPES = {"chain": CHAIN, "tiny": CONFIGS["tiny"]}
FACTORS = (1 - 2.0 ** -12, 1 + 2.0 ** -20, 0.75, 1.5)
ONES = 0xFFFFFFFFFFFFFFFF
SEED = 5  # of the GPU tests; the bounds come from seeds 0 .. 5
WEIGHTS = (0.5, 0.3, 0.2)
LT_STEPS = (0, 1, -3)
BABY_STEPS, GIANT_STEPS, ABSENT = (0, 1), (0, 2, -2), 3  # n1 = 2; (2, 1) = step 3 is absent
SPAN = 4
INTERVAL = (-2.0, 3.0)
# the degree-7 series that interpolate tanh on [-1, 1] and on [-2, 3] (numpy.polynomial.chebyshev.chebinterpolate)
CHEB7 = [float(c) for c in npcheb.chebinterpolate(np.tanh, 7)]
CHEB7_MAPPED = [float(c) for c in npcheb.chebinterpolate(lambda u: np.tanh(0.5 * (5.0 * u + 1.0)), 7)]
# kind -> (coefficients, interval or None for the power basis)
KINDS = {"poly3": (TANH[:4], None), "poly7": (TANH[:8], None), "cheb7": (CHEB7, (-1.0, 1.0)), "mapped7": (CHEB7_MAPPED, INTERVAL)}
A_NL = 6  # the limb count of the device runs of section A: every kind fits, the mapped series with one limb left

# 4 x the largest CPU-chain error over seeds 0 .. 5 (module docstring; `python -m tests.test_circuits`)
BOUND = {"1": 4 * 2.0 ** -29.13, "1c": 4 * 2.0 ** -29.21, "2": 4 * 2.0 ** -24.06, "3": 4 * 2.0 ** -28.24}
A_BOUND = {"poly3": 4 * 2.0 ** -26.01, "poly7": 4 * 2.0 ** -26.14, "cheb7": 4 * 2.0 ** -25.80, "mapped7": 4 * 2.0 ** -26.03}


def same(got, want, *tag):
    assert np.array_equal(got, want), tag


def new_oracle(name):
    a = SHAPES[name]
    return FastCpuContext(a[0], a[1], a[2], a[3], dnum=a[4])


_ORACLES = {}


def oracle(name):
    if name not in _ORACLES:
        _ORACLES[name] = new_oracle(name)
    return _ORACLES[name]


def new_context(name, device=0):
    from ppqsflhe_amd import Context
    a = SHAPES[name]
    return Context(a[0], a[1], a[2], a[3], dnum=a[4], device=device)


def qf(c, i):
    return float(int(c.moduli[i]))


def log2_q(c, nl):
    return sum(np.log2(qf(c, i)) for i in range(nl))


# ---- A: the scales ------------------------------------------------------------------------------------------------------

def off_scales(c, nl):
    """[(tag, scale)]: sf(L - nl) f for the four factors, the two neighbouring levels' own scales at this limb count, and at
    nl = L the fresh scale sf_big(0) f as well (sf(0) belongs to the 20-bit extra limb)."""
    L = c.L
    out = [(("f", f), c.sf(L - nl) * f) for f in FACTORS]
    out += [(("level", lev), c.sf(lev)) for lev in (L - nl - 1, L - nl + 1) if 0 <= lev <= L - 1]
    if nl == L:
        out += [(("fresh", f), c.sf_big(0) * f) for f in FACTORS]
    return out


def eval_refusal(c, kind, nl, scale):
    coef, iv = KINDS[kind]
    return poly_refusal(c, coef, nl, scale) if iv is None else cheb_refusal(c, coef, iv[0], iv[1], nl, scale)


def fits_plan(kind, nl):
    coef, iv = KINDS[kind]
    nl_u = nl if iv in (None, (-1.0, 1.0)) else nl - 1
    return nl_u >= 1 and py_plan(len(coef) - 1, nl_u)["nl_out"] >= 1


@pytest.fixture(scope="module")
def hosts():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = new_context(name, device=-1)
        return cache[name]

    yield get
    for c in cache.values():
        c.close()


def host_eval(c, kind, nl, scale):
    """the evaluation on addresses that are not memory: a host-only context refuses before it asks for a device"""
    coef, iv = KINDS[kind]
    big = 1 << 40
    if iv is None:
        return c.poly_eval(big, 2 * big, coef, 3 * big, 1, nl, scale)
    return c.cheb_eval(big, 2 * big, coef, iv[0], iv[1], 3 * big, 1, nl, scale)


@pytest.mark.parametrize("name", list(SHAPES))
def test_weights_and_ladder_scales_follow_the_scale_they_are_given(hosts, name):
    """w, S_k and S_out to the last bit against py_weights, py_cheb_weights and py_ladder at every nl the plan accepts; the
    restatement at the level's standard scale gives other weights (what a library that ignored scale_in would return)."""
    from ppqsflhe_amd.binding import MkckksError
    c = hosts(name)
    L, big = c.L, 1 << 40
    seen = differs = off = 0
    for nl in range(1, L + 1):
        std = c.sf(L - nl)
        for tag, scale in off_scales(c, nl):
            for kind in ("poly3", "poly7", "cheb7"):
                coef, iv = KINDS[kind]
                if not fits_plan(kind, nl):
                    continue
                p = py_plan(len(coef) - 1, nl)
                call, py = (c.poly_weights, py_weights) if iv is None else (c.cheb_weights, py_cheb_weights)
                w, s_out = call(coef, nl, scale)
                want, want_s = py(c.moduli, L, c.sf, coef, nl, scale)
                assert s_out == want_s == c.sf(L - p["nl_out"]), (name, nl, tag, kind)
                same(w, want, name, nl, tag, kind)
                if scale != std:
                    off += 1
                    differs += not np.array_equal(want, py(c.moduli, L, c.sf, coef, nl, std)[0])
                seen += 1
                # the ladders: x^1 .. x^B and y^1 .. y^(G-1); a zero count reports limbs and scales and runs nothing
                lad = c.powers if iv is None else c.cheb_ladder
                nlx, sx = py_ladder(c.moduli, nl, p["B"], scale)
                nly, sy = py_ladder(c.moduli, nlx[-1], p["G"] - 1, sx[-1])
                for n0, n, s0, want_l in ((nl, p["B"], scale, (nlx, sx)), (nlx[-1], p["G"] - 1, sx[-1], (nly, sy))):
                    if iv is not None and not ladder_fits(c.moduli, n0, n, s0):
                        with pytest.raises(MkckksError) as e:
                            lad(big, 2 * big, 3 * big, 0, n0, n, s0)
                        assert e.value.code == -1 and REFUSAL in str(e.value), (name, nl, tag, kind)
                        continue
                    got_l = lad(big, 2 * big, 3 * big, 0, n0, n, s0)
                    assert got_l == want_l, (name, nl, tag, kind, got_l, want_l)
    assert seen > off > 0 and differs == off, (name, seen, off, differs)


@pytest.mark.parametrize("name", list(SHAPES))
def test_the_predicted_refusals_at_off_standard_scales_are_the_librarys(hosts, name):
    """A predicted refusal ("does not fit half the modulus of its level") comes with its text, everything else gets as far as
    asking for a device."""
    from ppqsflhe_amd.binding import MkckksError
    c = hosts(name)
    count = {None: 0, REFUSAL: 0}
    for nl in range(1, c.L + 1):
        for tag, scale in off_scales(c, nl):
            for kind in KINDS:
                if not fits_plan(kind, nl):
                    continue
                why = eval_refusal(c, kind, nl, scale)
                with pytest.raises(MkckksError) as e:
                    host_eval(c, kind, nl, scale)
                if why is None:
                    assert e.value.code == -2, (name, nl, tag, kind, str(e.value))
                else:
                    assert why == REFUSAL and e.value.code == -1 and why in str(e.value), (name, nl, tag, kind, str(e.value))
                count[why] += 1
    # at these scales neither shape meets a refusal (a scale of 2^19 at nl = L makes the weights larger, and the top levels
    # hold them); the branch stays for the scales a later shape may add
    assert count[None] > 0, count


def keys_case(o, seed):
    """One key pair with its relinearisation key and the Galois keys of every step the circuits rotate by."""
    rng = np.random.default_rng(9000 + seed)
    s, a, e = make_keys(o, rng)
    pk, sk = o.keygen(s, a, e)
    rlk = oracle_relin_key(o, sk, pk, *make_rk_rand(o, rng))
    gk = {r: o.rekeygen(sigma_coeff(s, gal(o.N, r)), pk, *make_rk_rand(o, rng)) for r in (1, 2, -2, -3)}
    return dict(s=s, pk=pk, sk=sk, rlk=rlk, gk=gk, rng=rng)


def encrypt(o, rng, pk, vals, scale, nl):
    N = o.N
    return o.encrypt(pk, o.encode(vals, scale, nl), sample_ternary(rng, N), sample_gauss(rng, N), sample_gauss(rng, N))


def values_of(kind, v):
    coef, iv = KINDS[kind]
    if iv is None:
        return np.polyval(list(coef)[::-1], v)
    return npcheb.chebval((2.0 * v - (iv[0] + iv[1])) / (iv[1] - iv[0]), coef)


def cpu_eval(o, kind, ct, rlk, scale):
    coef, iv = KINDS[kind]
    if iv is None:
        return cpu_poly_eval(o, ct, rlk, coef, scale)
    return cpu_cheb_eval(o, ct, rlk, coef, iv[0], iv[1], scale)


def level_cut(o):
    """(nl, scale) of a standard ciphertext at A_NL limbs read one limb lower: A_NL - 1 limbs at the scale of A_NL.  (On
    `chain` sf(1) = sf(2) to the last bit, so the cut from L - 1 to L - 2 limbs would leave a standard scale.)"""
    return A_NL - 1, o.sf(o.L - A_NL)


def scale_cases(o, seed, kinds=tuple(KINDS)):
    """Section A on the CPU: per (kind, tag) an input really encrypted at that scale on A_NL limbs, the words of the CPU chain
    called with that scale, S_out and the decoded error.  The level cut is a ciphertext at the standard scale of A_NL limbs
    read at A_NL - 1."""
    K = keys_case(o, seed)
    rng, L = K["rng"], o.L
    out = {}
    for kind in kinds:
        iv = KINDS[kind][1]
        lo, hi = iv if iv else (-1.0, 1.0)
        for tag, scale in off_scales(o, A_NL):
            assert eval_refusal(o, kind, A_NL, scale) is None, (kind, tag)
            v = rng.uniform(lo, hi, size=o.N // 2)
            ct = encrypt(o, rng, K["pk"], v, scale, A_NL)
            words, s_out = cpu_eval(o, kind, ct, K["rlk"], scale)
            err = np.abs(o.decrypt_decode(words, K["sk"], s_out) - values_of(kind, v)).max()
            out[kind, tag] = dict(ct=ct, scale=scale, nl=A_NL, words=words, s_out=s_out, err=err, v=v)
    if "poly3" not in kinds:
        return dict(keys=K, cases=out)
    nl, scale = level_cut(o)
    assert scale != o.sf(L - nl) and eval_refusal(o, "poly3", nl, scale) is None
    v = rng.uniform(-1.0, 1.0, size=o.N // 2)
    ct = np.ascontiguousarray(encrypt(o, rng, K["pk"], v, scale, nl + 1)[:, :nl])
    words, s_out = cpu_eval(o, "poly3", ct, K["rlk"], scale)
    err = np.abs(o.decrypt_decode(words, K["sk"], s_out) - values_of("poly3", v)).max()
    out["poly3", ("cut", nl)] = dict(ct=ct, scale=scale, nl=nl, words=words, s_out=s_out, err=err, v=v)
    return dict(keys=K, cases=out)


def scale_case_chain(kind):
    def build(name):
        return scale_cases(oracle(name), SEED, (kind,))
    build.__name__ = "scale_case_" + kind
    return build


SCALE_CASES = {kind: scale_case_chain(kind) for kind in KINDS}


# ---- B: the circuits' plans: scales, limbs, refusals and headroom from the plaintext values alone -------------------------------

def circuit_values(N, seed):
    """The plaintext side: values, diagonals, and numpy float64 of every hop."""
    rng = np.random.default_rng(7000 + seed)
    half = N // 2
    V = {}
    # circuit 1: three ciphertexts, diagonals with sum_r |diag_r[j]| <= 1
    x1 = rng.uniform(-1.0, 1.0, size=(3, half))
    d1 = rng.uniform(-1.0, 1.0, size=(len(LT_STEPS), half))
    d1 /= np.maximum(1.0, np.abs(d1).sum(axis=0))
    y1 = sum(d1[k][None] * np.roll(x1, -r, axis=1) for k, r in enumerate(LT_STEPS))
    V["1"] = dict(x=x1, diags=d1, y=y1, out=values_of("poly3", y1), out_c=values_of("cheb7", y1))
    # circuit 2: one ciphertext; diagonals of the steps G + b except the absent one
    x2 = rng.uniform(-1.0, 1.0, size=half)
    steps = sorted({G + b for G in GIANT_STEPS for b in BABY_STEPS} - {ABSENT})
    d2 = {r: v for r, v in zip(steps, rng.uniform(-1.0, 1.0, size=(len(steps), half)))}
    norm = np.maximum(1.0, sum(np.abs(v) for v in d2.values()))
    d2 = {r: v / norm for r, v in d2.items()}
    a2 = values_of("poly3", x2)
    y2 = sum(d * np.roll(a2, -r) for r, d in d2.items())
    z2 = sum(np.roll(y2, -k) for k in range(SPAN))
    rolled = np.stack([np.stack([np.roll(d2[G + b], G) if G + b in d2 else np.zeros(half) for b in BABY_STEPS]) for G in GIANT_STEPS])
    present = [[1 if G + b in d2 else 0 for b in BABY_STEPS] for G in GIANT_STEPS]
    V["2"] = dict(x=x2, diags=d2, rolled=rolled, present=present, a=a2, y=y2, z=z2, out=z2 * z2)
    # circuit 3: three clients
    x3 = rng.uniform(-1.0, 1.0, size=(3, half))
    m3 = sum(w * x for w, x in zip(WEIGHTS, x3))
    V["3"] = dict(x=x3, m=m3, out=values_of("mapped7", m3))
    return V


def circuit_plan(c, V):
    """Per circuit: limbs and scales of every hop by the hosts' header rules (in their order of double operations), the
    refusal the restatements predict for each evaluation (None everywhere) and the headroom rule of every hop as
    (hop, bits needed, bits the limbs hold): need < have - 1 is include/mkckks.h's rule."""
    L = c.L
    S0 = c.sf_big(0)
    S1 = S0 / qf(c, L - 1)                       # product.hpp product_rescale
    amax = lambda x: float(np.abs(x).max())
    rows = lambda d: float(np.abs(d).sum(axis=0).max())
    P = {}
    # circuit 1: a noiseScaleDeg-1 input at level 1: plaintexts at sf(level), scale S * sf(level), then the rescale
    nl = L - 1
    pt1 = c.sf(1)
    St = S1 * pt1                                # linearTransform.cpp: first.scale * sf(first.level)
    Su = St / qf(c, nl - 1)
    room = [("transform", np.log2(S1) + np.log2(pt1) + np.log2(rows(V["1"]["diags"]) * amax(V["1"]["x"])), log2_q(c, nl))]
    P["1"] = dict(nl_in=L, nl_lt=nl, pt_scale=pt1, S_lt_in=S1, S_lt=St, nl_eval=nl - 1, S_eval=Su, room=room, evals=[])
    for kind, key in (("poly3", "1"), ("cheb7", "1c")):
        coef = KINDS[kind][0]
        p = py_plan(len(coef) - 1, nl - 1)
        P["1"]["evals"].append((kind, nl - 1, Su))
        P["1"]["nl_out" + key[1:]] = p["nl_out"]
        room.append(eval_room(c, kind, nl - 1, amax(V["1"]["y"])))
    # circuit 2
    nl = L - 1
    p = py_plan(3, nl)
    nl_p, Sp = p["nl_out"], c.sf(L - p["nl_out"])  # poly.hpp poly_result: the standard scale of the output's level
    pt2 = c.sf(L - nl_p)                         # a noiseScaleDeg-1 input at level L - nl_p
    St = Sp * pt2
    Su = St / qf(c, nl_p - 1)
    Sq = Su * Su                                 # product.hpp product_result
    So = Sq / qf(c, nl_p - 2)
    d2 = np.stack(list(V["2"]["diags"].values()))
    room = [eval_room(c, "poly3", nl, amax(V["2"]["x"])),
            ("transform", np.log2(Sp) + np.log2(pt2) + np.log2(rows(d2) * amax(V["2"]["a"])), log2_q(c, nl_p)),
            ("slot sum", np.log2(Su) + np.log2(amax(V["2"]["z"])), log2_q(c, nl_p - 1)),
            ("product", np.log2(Sq) + 2 * np.log2(amax(V["2"]["z"])), log2_q(c, nl_p - 1))]
    P["2"] = dict(nl_in=L, nl_eval=nl, S_eval=S1, nl_lt=nl_p, S_lt_in=Sp, pt_scale=pt2, S_lt=St, nl_sum=nl_p - 1, S_sum=Su, S_prod=Sq,
                  nl_out=nl_p - 2, S_out=So, room=room, evals=[("poly3", nl, S1)])
    # circuit 3: hostlib.hpp scale_aggregate on noiseScaleDeg-2 inputs at level 0 leaves a noiseScaleDeg-2 aggregate at
    # level 1 (about 2^80 on this shape), which evalPoly rescales before it evaluates (product.hpp product_rescale)
    sf_level = 1                                 # weights_sf_level: level + 1
    Sw = S0 / qf(c, L - 1) * c.sf(1)
    Se = Sw / qf(c, L - 2)
    coef, iv = KINDS["mapped7"]
    pm = py_plan(len(coef) - 1, L - 3)
    room = [("weighted sum", np.log2(S0) + np.log2(c.sf(sf_level)) + np.log2(amax(V["3"]["m"])), log2_q(c, L)),
            eval_room(c, "mapped7", L - 2, amax(V["3"]["m"]))]
    P["3"] = dict(nl_in=L, sf_level=sf_level, S_agg=Sw, nl_eval=L - 2, S_eval=Se, nl_out=pm["nl_out"], room=room,
                  evals=[("mapped7", L - 2, Se)])
    for key in P:
        P[key]["refusals"] = [eval_refusal(c, kind, nl, s) for kind, nl, s in P[key]["evals"]]
    return P


def eval_room(c, kind, nl, a_max):
    """The outer sum's headroom: Sigma * sum_k |c_k| A^k (power basis, |x| <= A) or Sigma * sum |m_{j,i}| (Chebyshev block,
    |T_k| <= 1 on the interval, which must hold the values) below half the modulus of nl_T limbs."""
    coef, iv = KINDS[kind]
    nl_u = nl if iv in (None, (-1.0, 1.0)) else nl - 1
    p = py_plan(len(coef) - 1, nl_u)
    sigma = np.log2(c.sf(c.L - p["nl_out"])) + np.log2(qf(c, p["nl_T"] - 1)) + np.log2(qf(c, p["nl_T"] - 2))
    if iv is None:
        mass = sum(abs(ck) * a_max ** k for k, ck in enumerate(coef))
    else:
        assert a_max <= max(abs(iv[0]), abs(iv[1]))  # the callers' values lie in the interval
        mass = sum(abs(v) for row in py_cheb_rewrite([float(x) for x in coef], p["B"], p["G"]) for v in row)
    return (kind, sigma + np.log2(mass), log2_q(c, p["nl_T"]))


def test_the_circuits_keep_every_plan_refusal_and_headroom_rule(hosts):
    """Device-free: for every circuit and for every scale of section A's device runs, the restatements predict no refusal, the
    library agrees (a host-only context gets as far as asking for a device), the limbs fit, and the numpy values keep the
    headroom rule of each hop.  Seeds 0 .. 5: the inputs the bounds are measured on, and the GPU tests' own."""
    from ppqsflhe_amd.binding import MkckksError
    c = hosts("chain")
    assert (c.N, c.L) == (1024, 8)
    for seed in range(6):
        P = circuit_plan(c, circuit_values(c.N, seed))
        for key, plan in P.items():
            assert plan["refusals"] == [None] * len(plan["evals"]), (seed, key, plan["refusals"])
            for hop, need, have in plan["room"]:
                assert need < have - 1, (seed, key, hop, need, have)
            for kind, nl, scale in plan["evals"]:
                with pytest.raises(MkckksError) as e:
                    host_eval(c, kind, nl, scale)
                assert e.value.code == -2, (seed, key, kind, str(e.value))
        assert P["1"]["nl_out"] == 3 and P["1"]["nl_outc"] == 2 and P["2"]["nl_out"] == 2 and P["3"]["nl_out"] == 1
        # the hosts' rules, followed hop by hop, land every evaluation on the standard scale of its level to the last bit
        # (sf(l + 1) = sf(l)^2 / q is how the levels' scales are defined): the off-standard scales are section A's
        for key, plan in P.items():
            for kind, nl, scale in plan["evals"]:
                assert scale == c.sf(c.L - nl), (key, kind)
        assert P["2"]["S_sum"] == c.sf(c.L - P["2"]["nl_sum"]) and P["2"]["S_out"] == c.sf(c.L - P["2"]["nl_out"])
    for kind in KINDS:
        cut = [(("cut", level_cut(c)[0]), level_cut(c)[1])] if kind == "poly3" else []
        for tag, scale in off_scales(c, A_NL) + cut:
            nl = tag[1] if tag[0] == "cut" else A_NL
            assert fits_plan(kind, nl) and eval_refusal(c, kind, nl, scale) is None, (kind, tag)
            lo, hi = KINDS[kind][1] or (-1.0, 1.0)  # section A draws its values from the interval
            hop, need, have = eval_room(c, kind, nl, max(abs(lo), abs(hi)))
            assert need < have - 1, (kind, tag, need, have)


# ---- B: the CPU restatement chains --------------------------------------------------------------------------------------------

def circuit_refs(o, seed, which=("1", "2", "3")):
    """Inputs, keys, the words after every step of every circuit and the decoded error of each, from the oracle alone."""
    N, L = o.N, o.L
    K = keys_case(o, seed)
    rng = K["rng"]
    V = circuit_values(N, seed)
    P = circuit_plan(o, V)
    zero_key = np.zeros((o.beta, 2, o.D, N), dtype=np.uint64)
    R = dict(keys=K, values=V, plan=P)
    dec = lambda ct, scale: o.decrypt_decode(ct, K["sk"], scale)
    if "1" in which:
        p = P["1"]
        x = np.stack([encrypt(o, rng, K["pk"], v, o.sf_big(0), L) for v in V["1"]["x"]])
        r = np.stack([o.rescale(ct) for ct in x])
        pts = np.stack([cpu_encode_ext(o, d, p["pt_scale"], p["nl_lt"]) for d in V["1"]["diags"]])
        gs = [gal(N, s) for s in LT_STEPS]
        evks = np.stack([K["gk"][s] if s else zero_key for s in LT_STEPS])
        t = np.stack([ref_linear_transform(o, ct, evks, pts, gs, p["nl_lt"]) for ct in r])
        u = np.stack([o.rescale(ct) for ct in t])
        outs = [cpu_poly_eval(o, ct, K["rlk"], KINDS["poly3"][0], p["S_eval"]) for ct in u]
        outc = [cpu_cheb_eval(o, ct, K["rlk"], KINDS["cheb7"][0], -1.0, 1.0, p["S_eval"]) for ct in u]
        R["1"] = dict(x=x, r=r, pts=pts, gs=gs, evks=evks, t=t, u=u, out=np.stack([w for w, _ in outs]), s_out=outs[0][1],
                      out_c=np.stack([w for w, _ in outc]), s_out_c=outc[0][1])
        R["1"]["err"] = max(np.abs(dec(w, s) - V["1"]["out"][b]).max() for b, (w, s) in enumerate(outs))
        R["1"]["err_c"] = max(np.abs(dec(w, s) - V["1"]["out_c"][b]).max() for b, (w, s) in enumerate(outc))
    if "2" in which:
        p = P["2"]
        x = encrypt(o, rng, K["pk"], V["2"]["x"], o.sf_big(0), L)
        r = o.rescale(x)
        a, s_a = cpu_poly_eval(o, r, K["rlk"], KINDS["poly3"][0], p["S_eval"])
        assert s_a == p["S_lt_in"] and a.shape[1] == p["nl_lt"]
        pts = np.stack([np.stack([cpu_encode_ext(o, v, p["pt_scale"], p["nl_lt"]) for v in row]) for row in V["2"]["rolled"]])
        gb, gg = [gal(N, b) for b in BABY_STEPS], [gal(N, G) for G in GIANT_STEPS]
        bkeys = np.stack([K["gk"][b] if b else zero_key for b in BABY_STEPS])
        gkeys = np.stack([K["gk"][G] if G else zero_key for G in GIANT_STEPS])
        t = ref_bsgs(o, a, bkeys, gb, gkeys, gg, pts, V["2"]["present"], p["nl_lt"])
        u = o.rescale(t)
        skeys = np.stack([K["gk"][1], K["gk"][2]])
        z = oracle_slot_sum(o, u, skeys, SPAN)
        q = oracle_relinearize(o, py_tensor(o.moduli[:p["nl_sum"]], z[None], z[None]), K["rlk"])
        out = o.rescale(q)
        R["2"] = dict(x=x, r=r, a=a, pts=pts, gb=gb, gg=gg, bkeys=bkeys, gkeys=gkeys, t=t, u=u, skeys=skeys, z=z, q=q, out=out,
                      s_out=p["S_out"])
        R["2"]["err"] = np.abs(dec(out, p["S_out"]) - V["2"]["out"]).max()
    if "3" in which:
        p = P["3"]
        clients = []
        for _ in range(3):
            s, a, e = make_keys(o, rng)
            pk, _ = o.keygen(s, a, e)
            clients.append((s, pk))
        x = np.stack([encrypt(o, rng, clients[k][1], V["3"]["x"][k], o.sf_big(0), L) for k in range(3)])
        evks = np.stack([o.rekeygen(clients[k][0], K["pk"], *make_rk_rand(o, rng)) for k in range(3)])
        scaled = [scaled_evk(o, evks[k], WEIGHTS[k], p["sf_level"]) for k in range(3)]
        agg = oracle_wsum(o, x[:, None], scaled, WEIGHTS, p["sf_level"], 0)
        r = o.rescale(agg)
        assert np.abs(dec(r, p["S_agg"]) - V["3"]["m"]).max() < 2.0 ** -30  # the aggregate's header scale decodes it
        r2 = o.rescale(r)
        out, s_out = cpu_cheb_eval(o, r2, K["rlk"], KINDS["mapped7"][0], INTERVAL[0], INTERVAL[1], p["S_eval"])
        R["3"] = dict(x=x, evks=evks, scaled=np.stack(scaled), agg=agg, r=r, r2=r2, out=out, s_out=s_out)
        R["3"]["err"] = np.abs(dec(out, s_out) - V["3"]["out"]).max()
    return R


def chain_refs(name):
    return circuit_refs(oracle(name), SEED)


def refs():
    return cached(chain_refs, "chain")


# ---- the circuits on the device ------------------------------------------------------------------------------------------------

def buf(g, shape, fill):
    return g.empty(shape) if fill is None else g.to_device(np.full(shape, fill, dtype=np.uint64))


def dev_eval(g, kind, d_ct, d_rlk, d_out, n_ct, nl, scale):
    coef, iv = KINDS[kind]
    if iv is None:
        return g.poly_eval(d_ct, d_rlk, coef, d_out, n_ct, nl, scale)
    return g.cheb_eval(d_ct, d_rlk, coef, iv[0], iv[1], d_out, n_ct, nl, scale)


def dev_circuit1_tail(g, R, d_t, kind, fill=None):
    """the last two steps: rescale, then the activation; returns {stage: words}"""
    c, p, N = R["1"], R["plan"]["1"], g.N
    nl, B = p["nl_lt"], 3
    nl_out = p["nl_out" if kind == "poly3" else "nl_outc"]
    d_u, d_out = buf(g, (B, 2, nl - 1, N), fill), buf(g, (B, 2, nl_out, N), fill)
    g.rescale(d_t, d_u, B, nl)
    s_out = dev_eval(g, kind, d_u, g.to_device(R["keys"]["rlk"]), d_out, B, nl - 1, p["S_eval"])
    assert s_out == c["s_out" if kind == "poly3" else "s_out_c"]
    return {"u": d_u.to_host(), "out" if kind == "poly3" else "out_c": d_out.to_host()}


def dev_circuit1(g, R, kind="poly3", device_encode=False):
    c, p, N, L = R["1"], R["plan"]["1"], g.N, g.L
    nl, B = p["nl_lt"], 3
    d_r, d_t = g.empty((B, 2, nl, N)), g.empty((B, 2, nl, N))
    g.rescale(g.to_device(c["x"]), d_r, B, L)
    if device_encode:
        d_pts = g.empty((len(LT_STEPS), nl + g.K, N))
        g.encode_ext(g.to_device(R["values"]["1"]["diags"]), d_pts, len(LT_STEPS), nl, p["pt_scale"])
    else:
        d_pts = g.to_device(c["pts"])
    g.linear_transform(d_r, g.to_device(c["evks"]), d_pts, c["gs"], d_t, B, nl)
    got = {"r": d_r.to_host(), "t": d_t.to_host()}
    got.update(dev_circuit1_tail(g, R, d_t, kind))
    return got


def dev_circuit2(g, R, between=lambda g, step: None):
    """`between(g, step)` runs after every step: the refused calls of the state tests"""
    c, p, N, L = R["2"], R["plan"]["2"], g.N, g.L
    nl, nl_a = p["nl_eval"], p["nl_lt"]
    d_rlk = g.to_device(R["keys"]["rlk"])
    d_r, d_a, d_t = g.empty((1, 2, nl, N)), g.empty((1, 2, nl_a, N)), g.empty((1, 2, nl_a, N))
    d_u, d_z, d_o = g.empty((1, 2, nl_a - 1, N)), g.empty((1, 2, nl_a - 1, N)), g.empty((1, 2, nl_a - 2, N))
    g.rescale(g.to_device(c["x"][None]), d_r, 1, L)
    between(g, "rescale")
    s_a = dev_eval(g, "poly3", d_r, d_rlk, d_a, 1, nl, p["S_eval"])
    assert s_a == p["S_lt_in"]
    between(g, "poly_eval")
    g.linear_transform_bsgs(d_a, g.to_device(c["bkeys"]), c["gb"], g.to_device(c["gkeys"]), c["gg"], g.to_device(c["pts"]),
                            R["values"]["2"]["present"], d_t, 1, nl_a)
    between(g, "bsgs")
    g.rescale(d_t, d_u, 1, nl_a)
    between(g, "rescale 2")
    g.slot_sum(d_u, g.to_device(c["skeys"]), d_z, 1, nl_a - 1, SPAN)
    between(g, "slot_sum")
    d_q = g.empty((1, 2, nl_a - 1, N))
    g.mult_relin(d_z, d_z, d_rlk, d_q, 1, nl_a - 1)
    between(g, "mult_relin")
    g.rescale(d_q, d_o, 1, nl_a - 1)
    return {k: d.to_host()[0] for k, d in (("r", d_r), ("a", d_a), ("t", d_t), ("u", d_u), ("z", d_z), ("q", d_q), ("out", d_o))}


def dev_circuit3(g, R):
    c, p, N, L = R["3"], R["plan"]["3"], g.N, g.L
    d_scaled, d_agg = g.empty(c["evks"].shape), g.empty((1, 2, L, N))
    g.scale_evk(g.to_device(c["evks"]), d_scaled, 3, WEIGHTS, p["sf_level"])
    g.reencrypt_wsum(g.to_device(c["x"][:, None]), d_scaled, d_agg, 3, 1, L, WEIGHTS, p["sf_level"])
    d_r, d_r2, d_o = g.empty((1, 2, L - 1, N)), g.empty((1, 2, L - 2, N)), g.empty((1, 2, p["nl_out"], N))
    g.rescale(d_agg, d_r, 1, L)
    g.rescale(d_r, d_r2, 1, L - 1)
    s_out = dev_eval(g, "mapped7", d_r2, g.to_device(R["keys"]["rlk"]), d_o, 1, L - 2, p["S_eval"])
    assert s_out == c["s_out"]
    return {"scaled": d_scaled.to_host(), "agg": d_agg.to_host()[0], "r": d_r.to_host()[0], "r2": d_r2.to_host()[0],
            "out": d_o.to_host()[0]}


RUN = {"1": dev_circuit1, "1c": lambda g, R: dev_circuit1(g, R, "cheb7"), "2": dev_circuit2, "3": dev_circuit3}


def check_words(got, R, key, *tag):
    for stage, words in got.items():
        same(words, R[key[0]][stage], key, stage, *tag)


def decoded_error(o, R, key, words):
    """max over slots (and ciphertexts) of |decoded - numpy float64 of the circuit|"""
    want = R["values"][key[0]]["out_c" if key == "1c" else "out"]
    s_out = R[key[0]]["s_out_c" if key == "1c" else "s_out"]
    sk = R["keys"]["sk"]
    if words.ndim == 4:
        return max(np.abs(o.decrypt_decode(words[b], sk, s_out) - want[b]).max() for b in range(words.shape[0]))
    return np.abs(o.decrypt_decode(words, sk, s_out) - want).max()


@pytest.fixture(scope="module")
def shared():
    """one device context for the module: every test that does not ask for a fresh one runs on it, in file order"""
    g = new_context("chain")
    yield g
    g.close()


@gpu
@pytest.mark.parametrize("kind", list(KINDS))
def test_evaluations_at_off_standard_scales(shared, kind):
    """poly_eval degree 3 and 7, cheb_eval degree 7 on [-1, 1] and on [-2, 3] with scale_in off the standard scale of the
    level, and (degree 3) the scale a level cut leaves: S_out and the words of the CPU chain called with that scale; the decoded
    values of an input encrypted at that scale."""
    g, o = shared, oracle("chain")
    case = cached(SCALE_CASES[kind], "chain")
    d_rlk = g.to_device(case["keys"]["rlk"])
    assert len(case["cases"]) == len(FACTORS) + 2 + (kind == "poly3")
    for (k, tag), c in case["cases"].items():
        d_ct = g.to_device(c["ct"][None])
        d_out = g.empty((1,) + c["words"].shape)
        s_out = dev_eval(g, k, d_ct, d_rlk, d_out, 1, c["nl"], c["scale"])
        assert s_out == c["s_out"] == g.sf(g.L - c["words"].shape[1]), (k, tag)
        got = d_out.to_host()[0]
        same(got, c["words"], k, tag)
        same(d_ct.to_host()[0], c["ct"], k, tag, "changed its input")
        err = np.abs(o.decrypt_decode(got, case["keys"]["sk"], s_out) - values_of(k, c["v"])).max()
        print(f"{k} {tag}: error 2^{np.log2(err):.2f}, bound 2^{np.log2(A_BOUND[k]):.2f}")
        assert err <= A_BOUND[k], (k, tag, err)


@gpu
@pytest.mark.parametrize("key", list(RUN))
def test_circuits_are_their_restatement_chains(shared, key):
    """Words after every step, and the decoded values against numpy float64 of the circuit."""
    g, o, R = shared, oracle("chain"), refs()
    got = RUN[key](g, R)
    check_words(got, R, key)
    err = decoded_error(o, R, key, got["out_c" if key == "1c" else "out"])
    print(f"circuit {key}: error 2^{np.log2(err):.2f}, bound 2^{np.log2(BOUND[key]):.2f}")
    assert err <= BOUND[key], (key, err)


@gpu
def test_circuit_1_with_plaintexts_encoded_on_the_device(shared):
    """encode_ext on the device agrees with the oracle's encoder to scale * 2^-50, not to the bit: the steps before the
    transform keep the reference's words, the decoded values keep the bound."""
    g, o, R = shared, oracle("chain"), refs()
    got = dev_circuit1(g, R, device_encode=True)
    same(got["r"], R["1"]["r"])
    err = decoded_error(o, R, "1", got["out"])
    print(f"circuit 1, device encode_ext: error 2^{np.log2(err):.2f}, bound 2^{np.log2(BOUND['1']):.2f}")
    assert err <= BOUND["1"], err


# ---- C: state --------------------------------------------------------------------------------------------------------------------

@gpu
def test_circuits_in_both_orders_on_one_context_and_on_fresh_ones(shared):
    """(1, 2, 3) then (3, 2, 1) on the shared context, which the tests above have used; each once more on a context of its
    own: three runs of a circuit, the same words, the reference's."""
    R = refs()
    for order in (("1", "2", "3"), ("3", "2", "1")):
        for key in order:
            check_words(RUN[key](shared, R), R, key, order)
    for key in ("1", "2", "3"):
        g = new_context("chain")
        try:
            check_words(RUN[key](g, R), R, key, "fresh")
        finally:
            g.close()


@gpu
def test_small_calls_after_large_ones_into_buffers_of_ones():
    """A fresh context; calls that grow every arena (linear_transform_bsgs and poly_eval degree 7 with 3 ciphertexts at
    nl = L, reencrypt_wsum with 3 clients, galois_keygen); then circuit 1's last two steps at 7 -> 6 -> 3 limbs into
    buffers pre-filled with all-ones words: the words of a fresh context, the reference's."""
    R, o = refs(), oracle("chain")
    c2, c3, K = R["2"], R["3"], R["keys"]
    g = new_context("chain")
    try:
        N, L, B = g.N, g.L, 3
        rng = np.random.default_rng(9100)
        from tests.test_gpu_parity import rand_ct, rand_polys
        big = rand_ct(rng, g, L, B)
        pts = rand_polys(rng, g, list(range(L)) + list(range(g.L, g.D)), 6).reshape(3, 2, L + g.K, N)
        d_out = buf(g, (B, 2, L, N), ONES)
        g.linear_transform_bsgs(g.to_device(big), g.to_device(c2["bkeys"]), c2["gb"], g.to_device(c2["gkeys"]), c2["gg"],
                                g.to_device(pts), R["values"]["2"]["present"], d_out, B, L)
        p7 = g.poly_plan(7, L)
        d_p = buf(g, (B, 2, p7["nl_out"], N), ONES)
        g.poly_eval(g.to_device(big), g.to_device(K["rlk"]), KINDS["poly7"][0], d_p, B, L, g.sf_big(0))
        d_scaled, d_agg = buf(g, c3["evks"].shape, ONES), buf(g, (1, 2, L, N), ONES)
        g.scale_evk(g.to_device(c3["evks"]), d_scaled, 3, WEIGHTS, 1)
        g.reencrypt_wsum(g.to_device(c3["x"][:, None]), d_scaled, d_agg, 3, 1, L, WEIGHTS, 1)
        same(d_agg.to_host()[0], c3["agg"], "the large weighted sum")
        rk = make_rk_rand(o, rng)
        d_gk = buf(g, (g.beta, 2, g.D, N), ONES)
        g.galois_keygen(g.to_device(K["s"]), g.to_device(K["pk"]), *[g.to_device(x) for x in rk], gal(N, 1), d_gk)
        same(d_gk.to_host(), o.rekeygen(sigma_coeff(K["s"], gal(N, 1)), K["pk"], *rk), "the large key generation")
        for kind in ("poly3", "cheb7"):
            got = dev_circuit1_tail(g, R, g.to_device(R["1"]["t"]), kind, fill=ONES)
            check_words(got, R, "1", "after large calls", kind)
    finally:
        g.close()


def refused(call, text):
    from ppqsflhe_amd.binding import MkckksError
    with pytest.raises(MkckksError) as e:
        call()
    assert e.value.code == -1 and text in str(e.value), (text, str(e.value))


@gpu
def test_refused_calls_between_the_steps_leave_the_circuit_alone():
    """After every step of circuit 2, on a fresh context: a poly_eval that "needs 4 limbs", a cheb_eval whose weight "does not
    fit", a ladder step that does not fit, a weighted key switch whose output lies over client 0 (refused inside the engine,
    after a device is there) and a poly_eval whose output overlaps its input: refusals tests/test_poly.py, tests/test_cheb.py and
    tests/test_weighted_aggregation.py assert on a device.  The circuit's words do not change."""
    R = refs()
    g = new_context("chain")
    try:
        N, L = g.N, g.L
        d_ct, d_res = g.empty((1, 2, L, N)), g.empty((1, 2, L, N))
        d_key = g.empty((g.beta, 2, g.D, N))
        seen = []

        def between(g, step):
            refused(lambda: g.poly_eval(d_ct, d_key, KINDS["poly3"][0], d_res, 1, 3, g.sf(L - 3)), "needs 4 limbs")
            refused(lambda: g.cheb_eval(d_ct, d_key, KINDS["cheb7"][0], -1.0, 1.0, d_res, 1, 5, 2.0 ** 75), "does not fit")
            refused(lambda: g.cheb_ladder(d_ct, d_key, d_res, 1, 2, 2, 2.0 ** 60), "does not fit")
            refused(lambda: g.reencrypt_wsum(d_ct, d_key, d_ct, 1, 1, L, [0.5], 1), "")
            refused(lambda: g.poly_eval(d_ct, d_key, KINDS["poly3"][0], d_ct, 1, L, g.sf_big(0)), "overlaps")
            seen.append(step)

        check_words(dev_circuit2(g, R, between), R, "2", "refusals between the steps")
        assert len(seen) == 6
    finally:
        g.close()


@gpu
@pytest.mark.parametrize("switch", ["MKCKKS_CHUNK", "MKCKKS_BSGS_WS_MIB"])
def test_circuit_2_under_the_library_switches(monkeypatch, switch):
    """Switches are read once, when a context is created: a fresh context under each gives the reference's words."""
    R = refs()
    monkeypatch.setenv(switch, "1")
    g = new_context("chain")
    try:
        check_words(dev_circuit2(g, R), R, "2", switch)
    finally:
        g.close()


# ---- the figures behind the bounds -------------------------------------------------------------------------------------------------

def measure_circuits(seed):
    """{circuit: error} of the CPU restatement chains at `chain`"""
    R = circuit_refs(new_oracle("chain"), seed)
    return {"1": R["1"]["err"], "1c": R["1"]["err_c"], "2": R["2"]["err"], "3": R["3"]["err"]}


def measure_scales(seed):
    """{kind: largest error over the scales of section A} of the CPU chains at `chain`"""
    S = scale_cases(new_oracle("chain"), seed)["cases"]
    return {kind: max(c["err"] for (k, _), c in S.items() if k == kind) for kind in KINDS}


if __name__ == "__main__":
    for what, measure in (("circuit", measure_circuits), ("A", measure_scales)):
        errs = [measure(seed) for seed in range(6)]
        for key in errs[0]:
            e = [x[key] for x in errs]
            print(f"{what} {key}: " + " ".join(f"2^{np.log2(v):.2f}" for v in e) + f"  ->  2^{np.log2(min(e)):.2f} .. 2^{np.log2(max(e)):.2f}")
