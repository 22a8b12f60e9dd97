"""Chains of the evaluation hosts, and the header bookkeeping between them.

Every host writes limbs, level, scale and noiseScaleDeg by a rule of its own (ppqsflhe_amd/host: product.hpp for cipherProduct,
poly.hpp for evalPoly, the comment at the top of linearTransform.cpp with hostlib.hpp's weights_sf_level, hostlib.hpp's
scale_aggregate for aggregateEncryptedWeights / serverRound; slotSum and changeCipherDomain keep the header).  `hop` below
restates those rules in Python doubles, in the hosts' order of operations.

On the GPU, at the `chain` parameters of tests/test_circuits.py (genCC: depth 6, ScalingModSize 40, RingDim 1024,
NumLargeDigits 2; two layers of 300 and 5 values):
  A  linearTransform --block (4 x 4) -> evalPoly --coeffs (degree 3) -> linearTransform --bsgs 2 (a noiseScaleDeg-1 input) ->
     slotSum --span 4 -> cipherProduct with itself -> decryptModelWeights
  B  two clients: REkeyGen, changeCipherDomain, serverRound --weights -> evalPoly --cheb -2,3 (degree 7) -> decryptModelWeights
After every hop the first ciphertext header of the output is read and limbs, level, noiseScaleDeg, slots and (with == on the
double) scale are held against `hop`; the decrypted values are held against numpy float64 within the bounds of circuits 2 and
3 of tests/test_circuits.py (4 x the largest error of the CPU restatement chains; nothing in them comes from a GPU result).

Without a device: the scale-agreement survey.  cipherProduct compares its operands' scales with !=, and two routes to the same
(limbs, level, noiseScaleDeg) compute the scale by different double expressions.  For every entry of
tests/test_parameter_lattice.py's TABLE and for `chain`, `tiny` and `ref`, every route of up to three hops from a fresh
ciphertext is walked with `hop` on a host-only context's sf and moduli, and the routes that meet are compared.  Result: no pair
differs on any accepted parameter set (the levels' scales are defined by the same recurrence sf(l + 1) = sf(l)^2 / q the hops
follow, with the same operations in the same order), so cipherProduct's comparison stands and this test is its guard.

Teeth ("Chained circuits"): linearTransform writing scale * sf(level + 1) for a noiseScaleDeg-1 input fails
chain A at the header of its third hop; evalPoly passing the scale before its own rescale fails both chains at the decrypted
values.  Wall time on an MI355X: 3.8 s per chain (about ten host processes each); the 27 device-free tests 0.3 s."""
import base64
import json
import struct

import numpy as np
import pytest
from numpy.polynomial import chebyshev as npcheb

from tests.test_circuits import BOUND, CHAIN, CHEB7_MAPPED, INTERVAL, SPAN
from tests.test_cli_hosts import _weights, run
from tests.test_gpu_parity import CONFIGS
from tests.test_parameter_lattice import TABLE, _kwargs
from tests.test_poly import TANH
from tests.test_poly_surface import py_plan
from tests.test_seeded_ciphertexts import mkws_to_json
from tests.test_slot_weights_cli import ok

gpu = pytest.mark.gpu
N, SLOTS, L = 1024, 512, 8
N_DENSE, N_BIAS = 300, 5
COEFFS = ",".join(repr(c) for c in TANH[:4])
CHEB = ",".join(repr(c) for c in CHEB7_MAPPED)
DIAG_STEPS = (-2, -1, 0, 1, 2)
CLIENT_WEIGHTS = (3.0, 1.0)  # the in-domain client first


# ---- the hosts' header rules ---------------------------------------------------------------------------------------------

def hop(c, h, op):
    """(limbs, level, noiseScaleDeg, scale) after host `op` on a ciphertext with header h, or None where the host refuses for
    want of limbs.  c: a context for sf and moduli.
      "lt" / "agg"   linearTransform, aggregateEncryptedWeights and serverRound (plain mean, --weights, --slot-weights): a
                     plaintext product at sf(weights_sf_level); ONE rescale on a noiseScaleDeg-2 input, scale / q_last *
                     sf(level + 1), noiseScaleDeg 2; none on a noiseScaleDeg-1 input: scale * sf(level), the degree rises
      "prod"         cipherProduct: product.hpp product_rescale on a noiseScaleDeg-2 operand, then S * S, noiseScaleDeg 2
      (kind, d, m)   evalPoly: product_rescale first; poly.hpp poly_result: depth limbs dropped (one more for a mapped
                     interval), the standard scale of the output's level, noiseScaleDeg 1
      "keep"         slotSum, changeCipherDomain: the header is the input's"""
    nl, level, deg, S = h
    q = lambda i: float(int(c.moduli[i]))
    if op == "keep":
        return h
    if op in ("lt", "agg"):
        if deg == 2:
            return None if nl < 2 else (nl - 1, level + 1, 2, S / q(nl - 1) * c.sf(level + 1))
        return (nl, level, deg + 1, S * c.sf(level))
    if deg == 2:
        if nl < 2:
            return None
        nl, level, S = nl - 1, level + 1, S / q(nl - 1)
    if op == "prod":
        return (nl, level, 2, S * S)
    kind, degree, mapped = op
    depth = py_plan(degree, 64)["depth"] + (1 if mapped else 0)
    if nl < depth + 1:
        return None
    return (nl - depth, level + depth, 1, c.sf(c.L - (nl - depth)))


OPS = ("lt", "prod", ("poly", 3, False), ("poly", 7, False), ("cheb", 2, False), ("cheb", 3, True))


def survey(c, hops=3):
    """(states reached, pairs compared, [(state, {scale: a route that gives it})] of the states whose routes disagree)"""
    frontier = [((), (c.L, 0, 2, c.sf_big(0)))]
    reach = {}
    for _ in range(hops):
        nxt = []
        for route, h in frontier:
            for op in OPS:
                r = hop(c, h, op)
                if r is None or r[2] > 2:  # every host refuses a noiseScaleDeg above 2
                    continue
                nxt.append((route + (op,), r))
                reach.setdefault(r[:3], []).append((route + (op,), r[3]))
        frontier = nxt
    pairs, differ = 0, []
    for state, routes in reach.items():
        pairs += len(routes) * (len(routes) - 1) // 2
        by_scale = {}
        for route, s in routes:
            by_scale.setdefault(s, route)
        if len(by_scale) > 1:
            differ.append((state, by_scale))
    return len(reach), pairs, differ


def survey_shapes():
    shapes = {name: (a[0][0], a[0][1], a[0][2], _kwargs(a[0])) for name, a in TABLE.items()}
    for name, a in (("tiny", CONFIGS["tiny"]), ("ref", CONFIGS["ref"]), ("chain", CHAIN)):
        shapes[name] = (a[0], a[1], a[2], dict(first_bits=a[3], dnum=a[4]))
    return shapes


@pytest.mark.parametrize("name", list(survey_shapes()))
def test_routes_to_the_same_header_agree_on_the_scale_to_the_last_bit(name):
    """Device-free.  Were a pair to differ, cipherProduct would refuse operands that agree mathematically: product_mismatch
    (product.hpp) would then need a relative tolerance of (double operations on the longest route) x 2^-53."""
    from ppqsflhe_amd import Context
    log_n, depth, bits, kw = survey_shapes()[name]
    c = Context(log_n, depth, bits, device=-1, **kw)
    try:
        states, pairs, differ = survey(c)
        assert states >= 3 and pairs >= 30, (name, states, pairs)
        assert differ == [], (name, differ)
    finally:
        c.close()


# ---- GPU: the chains ---------------------------------------------------------------------------------------------------------

def chain_cc(d):
    cfg = d / "config_cc.json"
    cfg.write_text(json.dumps({"MultiplicativeDepth": 6, "ScalingModSize": 40, "BatchSize": SLOTS, "RingDim": N, "NumLargeDigits": 2,
                               "PREMode": "INDCPA"}))
    ok(run("genCC", cfg, d / "CC.json"))
    return d / "CC.json"


def first_header(d, enc):
    """(limbs, level, noiseScaleDeg, scale), slots of the first ciphertext of the first layer's values[]"""
    env = d / (enc.name + ".env.json")
    mkws_to_json(enc, env)
    blob = base64.b64decode(json.load(open(env))["weights_summary"][0]["values"][0])
    hdr = struct.unpack("<4sIIIIIIIdII", blob[:48])
    assert hdr[0] == b"MKCK" and hdr[3] == N and hdr[5] == 2 and len(blob) == 48 + 8 * 2 * hdr[4] * N, hdr
    return (hdr[4], hdr[6], hdr[7], hdr[8]), hdr[9]


def matrix():
    m = np.random.default_rng(91).uniform(-1.0, 1.0, size=(4, 4))
    m /= np.abs(m).sum(axis=1, keepdims=True)  # row absolute sums 1: sum_r |diag_r[j]| <= 1
    return np.trunc(m * 1024) / 1024


def diagonals():
    d = np.random.default_rng(92).uniform(-1.0, 1.0, size=(len(DIAG_STEPS), SLOTS))
    d /= np.maximum(1.0, np.abs(d).sum(axis=0))
    return dict(zip(DIAG_STEPS, np.trunc(d * 4096) / 4096))


M, DIAGS = matrix(), diagonals()


def padded(v):
    out = np.zeros(SLOTS)
    out[:len(v)] = v
    return out


def chain_a_values(v):
    """numpy float64 of chain A on the slots of one ciphertext (zero padded, as the encoder pads)"""
    x = padded(v)
    y = (x.reshape(-1, 4) @ M.T).reshape(-1)
    a = np.polyval(TANH[:4][::-1], y)
    t = sum(dg * np.roll(a, -r) for r, dg in DIAGS.items())
    z = sum(np.roll(t, -k) for k in range(SPAN))
    return (z * z)[:len(v)]


@pytest.fixture(scope="module")
def host():
    from ppqsflhe_amd import Context
    c = Context(CHAIN[0], CHAIN[1], CHAIN[2], CHAIN[3], dnum=CHAIN[4], device=-1)
    yield c
    c.close()


def walk(d, c, h, steps):
    """run the hops; after each, the output's first header is `hop`'s, the scale with == on the double"""
    for prog, args, out, op in steps:
        ok(run(prog, *args))
        want = hop(c, h, op)
        got, slots = first_header(d, out)
        assert want is not None and got == want and slots == SLOTS, (prog, got, want, slots)
        h = got
    return h


@gpu
def test_chain_a_transform_activation_transform_sum_product(tmp_path, host):
    d, c = tmp_path, host
    cc = chain_cc(d)
    assert np.abs(M).sum(axis=1).max() <= 1 and sum(np.abs(v) for v in DIAGS.values()).max() <= 1
    rng = np.random.default_rng(2027)
    layers = [("dense", rng.uniform(-1.0, 1.0, N_DENSE)), ("bias", rng.uniform(-1.0, 1.0, N_BIAS))]
    (d / "matrix.json").write_text(json.dumps({"matrix": M.tolist()}))
    (d / "diag.json").write_text(json.dumps({"diagonals": [{"step": r, "values": v.tolist()} for r, v in DIAGS.items()]}))
    r = ok(run("linearTransform", cc, "--bsgs-steps", "2", d / "diag.json"))
    plan_steps = [int(s) for s in r.stdout.strip().split("steps=")[1].split(",")]
    steps = sorted(set(plan_steps) | {-3, -2, -1, 1, 2, 3})  # the plan's, the 4 x 4 blocks' diagonals, the slot sum's 1 and 2
    ok(run("keyGen", cc, d / "pk", d / "sk"))
    ok(run("rotKeyGen", cc, d / "sk", d / "pk", d / "rot", "--steps", ",".join(map(str, steps))))
    ok(run("relinKeyGen", cc, d / "sk", d / "pk", d / "relin"))
    ok(run("encryptModelWeights", cc, d / "pk", _weights(d, "w.json", layers), d / "h0.mkws"))
    fresh, slots = first_header(d, d / "h0.mkws")
    assert fresh == (L, 0, 2, c.sf_big(0)) and slots == SLOTS, fresh
    h = [d / f"h{k}.mkws" for k in range(6)]
    last = walk(d, c, fresh, [
        ("linearTransform", (cc, d / "rot", "--block", d / "matrix.json", h[0], h[1]), h[1], "lt"),
        ("evalPoly", (cc, d / "relin", h[1], h[2], "--coeffs", COEFFS), h[2], ("poly", 3, False)),
        ("linearTransform", (cc, d / "rot", d / "diag.json", h[2], h[3], "--bsgs", "2"), h[3], "lt"),
        ("slotSum", (cc, d / "rot", h[3], h[4], "--span", str(SPAN)), h[4], "keep"),
        ("cipherProduct", (cc, d / "relin", h[4], h[4], h[5]), h[5], "prod")])
    assert last[:3] == (2, 6, 2), last  # 8 -> 7 (transform) -> 6 -> 3 (activation) -> 3 (degree rises) -> 2 (product's rescale)
    ok(run("decryptModelWeights", cc, d / "sk", h[5], d / "dec.json"))
    dec = json.load(open(d / "dec.json"))["weights_summary"]
    for li, (name, v) in enumerate(layers):
        err = np.abs(np.array(dec[li]["values"]) - chain_a_values(v)).max()
        print(f"chain A {name}: |decrypted - numpy| = 2^{np.log2(err):.2f}, bound 2^{np.log2(BOUND['2']):.2f}")
        assert dec[li]["layer"] == name and err <= BOUND["2"], (name, err)


@gpu
def test_chain_b_weighted_round_then_a_series_on_an_interval(tmp_path, host):
    d, c = tmp_path, host
    cc = chain_cc(d)
    rng = np.random.default_rng(2028)
    vals = [[("dense", rng.uniform(-1.0, 1.0, N_DENSE)), ("bias", rng.uniform(-1.0, 1.0, N_BIAS))] for _ in range(2)]
    for k in range(2):
        ok(run("keyGen", cc, d / f"pk{k}", d / f"sk{k}"))
        ok(run("encryptModelWeights", cc, d / f"pk{k}", _weights(d, f"w{k}.json", vals[k]), d / f"enc{k}.mkws"))
    ok(run("relinKeyGen", cc, d / "sk1", d / "pk1", d / "relin"))
    ok(run("REkeyGen", cc, d / "sk0", d / "pk1", d / "rk0"))
    fresh, _ = first_header(d, d / "enc0.mkws")
    assert fresh == (L, 0, 2, c.sf_big(0)), fresh
    w = ",".join(repr(x) for x in CLIENT_WEIGHTS)
    last = walk(d, c, fresh, [
        ("changeCipherDomain", (cc, d / "rk0", d / "enc0.mkws", d / "pre0.mkws"), d / "pre0.mkws", "keep"),
        ("serverRound", (cc, d / "agg.mkws", "-", d / "enc1.mkws", "-", d / "pre0.mkws", "--weights", w), d / "agg.mkws", "agg"),
        ("evalPoly", (cc, d / "relin", d / "agg.mkws", d / "act.mkws", "--cheb", "%r,%r" % INTERVAL, "--coeffs", CHEB), d / "act.mkws",
         ("cheb", 7, True))])
    assert last[:3] == (1, 7, 1), last  # 8 -> 7 (the round's rescale) -> 6 (evalPoly's) -> 5 (the map) -> 1
    # the fused weighted key switch gives the same header
    ok(run("serverRound", cc, d / "agg2.mkws", "-", d / "enc1.mkws", d / "rk0", d / "enc0.mkws", "--weights", w))
    assert first_header(d, d / "agg2.mkws") == first_header(d, d / "agg.mkws")
    ok(run("decryptModelWeights", cc, d / "sk1", d / "act.mkws", d / "dec.json"))
    dec = json.load(open(d / "dec.json"))["weights_summary"]
    wn = np.array(CLIENT_WEIGHTS) / sum(CLIENT_WEIGHTS)
    for li in range(2):
        m = wn[0] * vals[1][li][1] + wn[1] * vals[0][li][1]
        want = npcheb.chebval((2.0 * m - (INTERVAL[0] + INTERVAL[1])) / (INTERVAL[1] - INTERVAL[0]), CHEB7_MAPPED)
        err = np.abs(np.array(dec[li]["values"]) - want).max()
        print(f"chain B layer {li}: |decrypted - numpy| = 2^{np.log2(err):.2f}, bound 2^{np.log2(BOUND['3']):.2f}")
        assert err <= BOUND["3"], (li, err)
