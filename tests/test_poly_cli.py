"""evalPoly.  Without a GPU: the argv contract and everything evalPoly refuses before it opens a device (a bad --coeffs
list, a key container of another kind, a degree whose plan does not fit the input's limbs), on crafted containers -- only
headers are read that early.  On the GPU, one round at the "tiny" parameters (N = 2^10, depth 3, 40-bit scaling, 2
digits): genCC -> keyGen -> relinKeyGen -> encryptModelWeights -> evalPoly --coeffs (degree 3) -> decryptModelWeights; the
bound is that of tests/test_poly.py (4 x the largest error of the CPU chain at these parameters)."""
import base64
import json
import os
import struct

import numpy as np
import pytest

from tests.test_cli_hosts import BIN, _weights, run, write_key_container
from tests.test_poly import POLY_BOUND, TANH
from tests.test_product_cli import KIND_CT, KIND_RELIN, KIND_RK, KIND_ROTKEYS, ct_blob, envelope
from tests.test_seeded_ciphertexts import mkws_to_json
from tests.test_slot_weights_cli import ok

gpu = pytest.mark.gpu
USAGE = "<cc_path> <relinkey> <input_encfile> <output_encfile> --coeffs c0,c1,...,cd [--max-abs A]"
N, SLOTS, L = 1024, 512, 5
COEFFS = ",".join(repr(c) for c in TANH[:4])


def tiny_cc(d):
    cfg = d / "config_cc.json"
    cfg.write_text(json.dumps({"MultiplicativeDepth": 3, "ScalingModSize": 40, "BatchSize": SLOTS, "RingDim": N, "NumLargeDigits": 2,
                               "PREMode": "INDCPA"}))
    ok(run("genCC", cfg, d / "CC.json"))
    return d / "CC.json"


def test_evalpoly_is_built_and_states_its_usage():
    assert os.access(os.path.join(BIN, "evalPoly"), os.X_OK), "evalPoly not built (make -C ppqsflhe_amd/host)"
    for args in ((), ("a",), ("a", "b", "c", "d"), ("a", "b", "c", "d", "--coeffs"), ("a", "b", "c", "d", "--max-abs", "2"),
                 ("a", "b", "c", "d", "--coeffs", "1,2,3", "--coeffs", "1,2,3"), ("a", "b", "c", "d", "--coeffs", "1,2,3", "--other", "1")):
        r = run("evalPoly", *args)
        assert r.returncode == 1 and "Usage:" in r.stderr and USAGE in r.stderr, (args, r.stderr)


def test_refusals_decided_before_a_device_is_opened(tmp_path):
    cc = tiny_cc(tmp_path)
    out = tmp_path / "out.json"
    key = tmp_path / "relin.key"
    write_key_container(key, KIND_RELIN, N, 8, 4, np.zeros(4, dtype=np.uint64))
    fresh = envelope(tmp_path / "a.json", [ct_blob(limbs=5, level=0, noise_deg=2, scale=2.0 ** 80, slots=SLOTS)] * 3)

    def refused(args, msg):
        r = run("evalPoly", *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stdout + r.stderr)
        assert not os.path.exists(out), args

    # the coefficient list
    for bad, msg in (("1,2", "the degree must be in [2, 63], got 2 coefficient(s)"), ("1,,3", "--coeffs: empty entry 1"),
                     ("1,x,3", "--coeffs: entry 1 (x) is not a finite number"), ("1,2,inf", "is not a finite number"),
                     (",".join(["1"] * 65), "the degree must be in [2, 63]")):
        refused((cc, key, fresh, out, "--coeffs", bad), "[evalpoly] ERROR: " + msg if msg.startswith("--") else msg)
    for bad in ("0", "-1", "x", "nan", "1e999"):
        refused((cc, key, fresh, out, "--coeffs", COEFFS, "--max-abs", bad), "[evalpoly] ERROR: --max-abs needs a positive number")
    refused((tmp_path / "nocc", key, fresh, out, "--coeffs", COEFFS), "[evalpoly] ERROR: Failed to load CryptoContext from")
    # the key container: absent, no container, and the other kinds by name
    refused((cc, tmp_path / "nokey", fresh, out, "--coeffs", COEFFS), "[evalpoly] ERROR: Failed to load the relinearisation key from")
    for kind, name in ((KIND_RK, "a re-encryption key"), (KIND_ROTKEYS, "a rotation-key file"), (2, "a public key")):
        other = tmp_path / f"kind{kind}.key"
        write_key_container(other, kind, N, 8, 4, np.zeros(4, dtype=np.uint64))
        refused((cc, other, fresh, out, "--coeffs", COEFFS), f"is {name}, not a relinearisation key")
    refused((cc, key, tmp_path / "noin", out, "--coeffs", COEFFS), "[evalpoly] ERROR: Could not open input encrypted weights file")
    # a degree that does not fit the limbs: a fresh ciphertext has 5 limbs, 4 after its rescale; degree 7 needs 5, 15 needs 7
    deg = lambda d: ",".join(["0.5"] * (d + 1))
    refused((cc, key, fresh, out, "--coeffs", deg(7)),
            "[evalpoly] ERROR: degree 7 needs 5 limbs (depth 4 and one limb for the result), the input has 4 after the rescale")
    refused((cc, key, fresh, out, "--coeffs", deg(15)), "degree 15 needs 7 limbs")
    low = envelope(tmp_path / "low.json", [ct_blob(limbs=3, level=2, noise_deg=1, scale=2.0 ** 40, slots=SLOTS)] * 3)
    refused((cc, key, low, out, "--coeffs", COEFFS), "[evalpoly] ERROR: degree 3 needs 4 limbs (depth 3 and one limb for the result), the input has 3")
    # ciphertexts that differ, and a field that holds none
    mixed = envelope(tmp_path / "m.json", [ct_blob(limbs=5, slots=SLOTS), ct_blob(limbs=5, slots=SLOTS), ct_blob(limbs=4, slots=SLOTS)])
    refused((cc, key, mixed, out, "--coeffs", COEFFS), "[evalpoly] ERROR: the ciphertexts of the input differ in limbs")
    bad = envelope(tmp_path / "bad.json", [ct_blob(limbs=5, slots=SLOTS), "AAAA", ct_blob(limbs=5, slots=SLOTS)])
    refused((cc, key, bad, out, "--coeffs", COEFFS), "[evalpoly] ERROR: the input holds a field that is no ciphertext")


N_DENSE, N_BIAS = 300, 5


@pytest.fixture(scope="module")
def deployment(tmp_path_factory):
    d = tmp_path_factory.mktemp("poly")
    cc = tiny_cc(d)
    rng = np.random.default_rng(2026)
    layers = [("dense", rng.uniform(-1.0, 1.0, N_DENSE)), ("bias", rng.uniform(-1.0, 1.0, N_BIAS))]
    ok(run("keyGen", cc, d / "pk", d / "sk"))
    ok(run("relinKeyGen", cc, d / "sk", d / "pk", d / "relin"))
    ok(run("encryptModelWeights", cc, d / "pk", _weights(d, "a.json", layers), d / "a.mkws"))
    return d, cc, layers


@gpu
def test_evalpoly_round_decrypts_to_the_polynomial(deployment):
    from ppqsflhe_amd import Context
    d, cc, layers = deployment
    r = ok(run("evalPoly", cc, d / "relin", d / "a.mkws", d / "p.mkws", "--coeffs", COEFFS))
    assert "degree 3" in r.stdout and "B 2, G 2, 2 relinearisation(s), 4 -> 1 limb(s)" in r.stdout, r.stdout
    ok(run("decryptModelWeights", cc, d / "sk", d / "p.mkws", d / "p.json"))
    dec = json.load(open(d / "p.json"))["weights_summary"]
    poly = lambda v: np.polyval(TANH[:4][::-1], v)
    for li, (name, v) in enumerate(layers):
        err = np.abs(np.array(dec[li]["values"]) - poly(v)).max()
        print(f"{name}: |decrypted - p(x)| = 2^{np.log2(err):.2f}, bound 2^{np.log2(POLY_BOUND[('tiny', 3)]):.2f}")
        assert dec[li]["layer"] == name and err <= POLY_BOUND[("tiny", 3)], (name, err)
        assert abs(dec[li]["mean"] - poly(float(np.mean(v)))) <= POLY_BOUND[("tiny", 3)]
        assert abs(dec[li]["std_dev"] - poly(float(np.std(v)))) <= POLY_BOUND[("tiny", 3)]
    # the header of the result: nl_out = 1 limb, level L - nl_out, the standard scale of that level, noiseScaleDeg 1
    mkws_to_json(d / "p.mkws", d / "p_env.json")
    blob = base64.b64decode(json.load(open(d / "p_env.json"))["weights_summary"][0]["values"][0])
    assert len(blob) == 48 + 8 * 2 * 1 * N
    hdr = struct.unpack("<4sIIIIIIIdII", blob[:48])
    h = Context(10, 3, 40, 60, dnum=2, device=-1)
    try:
        assert hdr[2] == KIND_CT and hdr[3] == N and hdr[4] == 1 and hdr[6] == L - 1 and hdr[7] == 1 and hdr[9] == SLOTS, hdr
        assert hdr[8] == h.sf(L - 1)
    finally:
        h.close()


@gpu
def test_evalpoly_refusals_on_real_files(deployment):
    d, cc, layers = deployment
    out = d / "x.mkws"

    def refused(args, msg):
        r = run("evalPoly", *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stdout + r.stderr)
        assert not os.path.exists(out), args

    ok(run("rotKeyGen", cc, d / "sk", d / "pk", d / "rot", "--sum", 2))
    refused((cc, d / "rot", d / "a.mkws", out, "--coeffs", COEFFS), "is a rotation-key file, not a relinearisation key")
    refused((cc, d / "relin", d / "a.mkws", out, "--coeffs", ",".join(["0.5"] * 8)), "degree 7 needs 5 limbs")
    # Sigma is about 2^120 on limbs of 140 bits: |x| <= 1000 needs 120 + log2(1e9 / 3) = 148 bits
    refused((cc, d / "relin", d / "a.mkws", out, "--coeffs", COEFFS, "--max-abs", 1000), "[evalpoly] ERROR: no headroom: the outer sum needs")
    ok(run("evalPoly", cc, d / "relin", d / "a.mkws", d / "ok.mkws", "--coeffs", COEFFS, "--max-abs", 8))
