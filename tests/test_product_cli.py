"""relinKeyGen and cipherProduct.  Without a GPU: the argv contracts and everything cipherProduct refuses before it opens
a device (operands that differ, by the name of the header field; a key container of another kind; a noiseScaleDeg-2
operand with one limb), on crafted containers -- only headers are read that early.  On the GPU: keyGen -> relinKeyGen,
rotKeyGen --sum -> encryptModelWeights x 2 -> cipherProduct -> slotSum -> decryptModelWeights at the reference parameters
(N = 2^14, depth 2, 40-bit scaling), JSON and MKWS envelopes; the bounds are those of tests/test_product.py (4 x the
largest error of the CPU oracle's composition at these parameters)."""
import base64
import json
import os
import struct

import numpy as np
import pytest

from tests.test_cli_hosts import BIN, _small_cc, _weights, run, write_key_container
from tests.test_product import PRODUCT_BOUND
from tests.test_seeded_ciphertexts import mkws_to_json
from tests.test_slot_weights_cli import ok, same

gpu = pytest.mark.gpu
N, SLOTS = 16384, 8192
KIND_CT, KIND_RK, KIND_ROTKEYS, KIND_RELIN = 1, 4, 9, 10
USAGE = {"relinKeyGen": "<cc.json> <privkey> <pubkey> <relinkey_out>",
         "cipherProduct": "<cc_path> <relinkey> <input_encfile_A> <input_encfile_B> <output_encfile>"}


def ct_blob(limbs=4, level=0, noise_deg=2, scale=2.0 ** 80, slots=SLOTS):
    """The 48-byte container header of a ciphertext (hostlib.hpp BlobHeader), base64, without a payload."""
    hdr = struct.pack("<4sIIIIIIIdII", b"MKCK", 1, KIND_CT, N, limbs, 2, level, noise_deg, scale, slots, 0)
    return base64.b64encode(hdr).decode()


def envelope(path, blobs, layer="dense"):
    """A JSON envelope of one layer whose mean, std_dev and values[] are `blobs` (3 or more)."""
    path.write_text(json.dumps({"weights_summary": [{"layer": layer, "shape": [len(blobs) - 2], "mean": blobs[0],
                                                     "std_dev": blobs[1], "values": list(blobs[2:])}]}))
    return path


def test_hosts_are_built_and_state_their_usage():
    for prog, usage in USAGE.items():
        assert os.access(os.path.join(BIN, prog), os.X_OK), f"{prog} not built (make -C ppqsflhe_amd/host)"
        for args in ((), ("a",), ("a", "b", "c"), ("a", "b", "c", "d", "e", "f", "g")):
            r = run(prog, *args)
            assert r.returncode == 1 and "Usage:" in r.stderr and usage in r.stderr, (prog, args, r.stderr)


def test_refusals_decided_before_a_device_is_opened(tmp_path):
    cc = _small_cc(tmp_path)
    out = tmp_path / "out.json"
    key = tmp_path / "relin.key"
    write_key_container(key, KIND_RELIN, N, 7, 4, np.zeros(4, dtype=np.uint64))
    good = [ct_blob()] * 3
    a = envelope(tmp_path / "a.json", good)

    def refused(args, msg):
        r = run("cipherProduct", *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stdout + r.stderr)
        assert not os.path.exists(out), args

    r = run("relinKeyGen", tmp_path / "nocc", "sk", "pk", out)
    assert r.returncode == 1 and "[relinkeygen] ERROR: Failed to load CryptoContext from" in r.stderr and not os.path.exists(out)
    refused((tmp_path / "nocc", key, a, a, out), "[product] ERROR: Failed to load CryptoContext from")
    # the key container: absent, no container, and the other kinds by name
    refused((cc, tmp_path / "nokey", a, a, out), "[product] ERROR: Failed to load the relinearisation key from")
    (tmp_path / "junk.key").write_text("not a key container, but longer than one header: " + "x" * 64)
    refused((cc, tmp_path / "junk.key", a, a, out), "[product] ERROR: Failed to load the relinearisation key from")
    for kind, name in ((KIND_RK, "a re-encryption key"), (KIND_ROTKEYS, "a rotation-key file"), (2, "a public key")):
        other = tmp_path / f"kind{kind}.key"
        write_key_container(other, kind, N, 7, 4, np.zeros(4, dtype=np.uint64))
        refused((cc, other, a, a, out), f"is {name}, not a relinearisation key")
    # the inputs
    refused((cc, key, tmp_path / "noa", a, out), "[product] ERROR: Could not open input encrypted weights file")
    refused((cc, key, a, tmp_path / "nob", out), "[product] ERROR: Could not open input encrypted weights file")
    # operands that differ, by field
    for field, kw in (("limbs", dict(limbs=3)), ("level", dict(level=1)), ("scale", dict(scale=2.0 ** 79)),
                      ("noiseScaleDeg", dict(noise_deg=1)), ("slots", dict(slots=4096))):
        b = envelope(tmp_path / f"b_{field}.json", [ct_blob(**kw)] * 3)
        refused((cc, key, a, b, out), f"[product] ERROR: the operands differ in {field} ")
        refused((cc, key, b, a, out), f"[product] ERROR: the operands differ in {field} ")
        mixed = envelope(tmp_path / f"m_{field}.json", [ct_blob(), ct_blob(), ct_blob(**kw)])
        refused((cc, key, mixed, a, out), f"[product] ERROR: the ciphertexts of operand A differ in {field}")
        refused((cc, key, a, mixed, out), f"[product] ERROR: the ciphertexts of operand B differ in {field}")
        refused((cc, key, mixed, mixed, out), f"[product] ERROR: the ciphertexts of operand A differ in {field}")
    # a noiseScaleDeg-2 operand on its last limb, as a pair and as a square
    one = envelope(tmp_path / "one.json", [ct_blob(limbs=1, level=3)] * 3)
    one_b = envelope(tmp_path / "one_b.json", [ct_blob(limbs=1, level=3)] * 3)
    refused((cc, key, one, one_b, out), "[product] ERROR: no limb left to rescale")
    refused((cc, key, one, one, out), "[product] ERROR: no limb left to rescale")
    # a field that holds no ciphertext
    bad = envelope(tmp_path / "bad.json", [ct_blob(), "AAAA", ct_blob()])
    refused((cc, key, bad, a, out), "[product] ERROR: operand A holds a field that is no ciphertext")


N_DENSE, N_BIAS = 700, 5


@pytest.fixture(scope="module")
def deployment(tmp_path_factory):
    d = tmp_path_factory.mktemp("prod")
    cc = _small_cc(d)
    rng = np.random.default_rng(2025)
    la = [("dense", rng.uniform(-0.3, 0.3, N_DENSE)), ("bias", rng.uniform(-0.3, 0.3, N_BIAS))]
    lb = [("dense", rng.uniform(-0.3, 0.3, N_DENSE)), ("bias", rng.uniform(-0.3, 0.3, N_BIAS))]
    ok(run("keyGen", cc, d / "pk", d / "sk"))
    r = ok(run("relinKeyGen", cc, d / "sk", d / "pk", d / "relin"))
    assert "[relinkeygen] Relinearisation key saved to" in r.stdout
    ok(run("rotKeyGen", cc, d / "sk", d / "pk", d / "rot_sum", "--sum", SLOTS))
    ok(run("encryptModelWeights", cc, d / "pk", _weights(d, "a.json", la), d / "a.mkws"))
    ok(run("encryptModelWeights", cc, d / "pk", _weights(d, "b.json", lb), d / "b.mkws"))
    return d, cc, la, lb


def decrypted(d, cc, enc, name):
    ok(run("decryptModelWeights", cc, d / "sk", enc, d / name))
    return json.load(open(d / name))["weights_summary"]


@gpu
def test_product_then_slot_sum_decrypts_to_the_inner_product(deployment):
    d, cc, la, lb = deployment
    r = ok(run("cipherProduct", cc, d / "relin", d / "a.mkws", d / "b.mkws", d / "ab.mkws"))
    assert "on 3 limb(s), scale 2^" in r.stdout and "(squares)" not in r.stdout, r.stdout
    dec = decrypted(d, cc, d / "ab.mkws", "ab.json")
    for li, ((name, va), (_, vb)) in enumerate(zip(la, lb)):
        err = np.abs(np.array(dec[li]["values"]) - va * vb).max()
        print(f"{name}: |decrypted - a * b| = 2^{np.log2(err):.2f}")
        assert dec[li]["layer"] == name and err <= PRODUCT_BOUND["ref"][0], (name, err)
        assert abs(dec[li]["mean"] - float(np.mean(va)) * float(np.mean(vb))) <= PRODUCT_BOUND["ref"][0]
    ok(run("slotSum", cc, d / "rot_sum", d / "ab.mkws", d / "ip.mkws"))
    dec = decrypted(d, cc, d / "ip.mkws", "ip.json")
    for li, ((name, va), (_, vb)) in enumerate(zip(la, lb)):
        want = float(np.dot(va, vb))
        err = np.abs(np.array(dec[li]["values"]) - want).max()
        print(f"{name}: |decrypted - <a, b>| = 2^{np.log2(err):.2f} (inner product {want:.6f})")
        assert err <= PRODUCT_BOUND["ref"][1], (name, err)


@gpu
def test_the_same_path_twice_squares_and_gives_the_squared_norm(deployment):
    d, cc, la, lb = deployment
    r = ok(run("cipherProduct", cc, d / "relin", d / "a.mkws", d / "a.mkws", d / "aa.mkws"))
    assert "(squares)" in r.stdout, r.stdout
    ok(run("slotSum", cc, d / "rot_sum", d / "aa.mkws", d / "norm.mkws"))
    dec = decrypted(d, cc, d / "norm.mkws", "norm.json")
    for li, (name, va) in enumerate(la):
        err = np.abs(np.array(dec[li]["values"]) - float(np.dot(va, va))).max()
        print(f"{name}: |decrypted - |a|^2| = 2^{np.log2(err):.2f}")
        assert err <= PRODUCT_BOUND["ref"][2], (name, err)
    # a copy of the file under another name takes the general path and gives the same containers
    (d / "a_copy.mkws").write_bytes(open(d / "a.mkws", "rb").read())
    ok(run("cipherProduct", cc, d / "relin", d / "a.mkws", d / "a_copy.mkws", d / "aa2.mkws"))
    assert same(d / "aa.mkws", d / "aa2.mkws")


@gpu
def test_json_and_mkws_inputs_give_the_same_ciphertext_bytes(deployment):
    d, cc, la, lb = deployment
    mkws_to_json(d / "a.mkws", d / "a_env.json")
    mkws_to_json(d / "b.mkws", d / "b_env.json")
    ok(run("cipherProduct", cc, d / "relin", d / "a.mkws", d / "b.mkws", d / "p.mkws"))
    ok(run("cipherProduct", cc, d / "relin", d / "a_env.json", d / "b_env.json", d / "p.json"))
    ok(run("cipherProduct", cc, d / "relin", d / "a_env.json", d / "b.mkws", d / "p_mixed.json"))  # the form of input A
    mkws_to_json(d / "p.mkws", d / "p_from_mkws.json")
    a, b = json.load(open(d / "p.json")), json.load(open(d / "p_from_mkws.json"))
    assert a == b == json.load(open(d / "p_mixed.json")) and len(a["weights_summary"]) == 2
    blob = base64.b64decode(a["weights_summary"][0]["values"][0])
    assert len(blob) == 48 + 8 * 2 * 3 * N  # 3 limbs after the operands' rescale
    hdr = struct.unpack("<4sIIIIIIIdII", blob[:48])
    assert hdr[2] == KIND_CT and hdr[4] == 3 and hdr[6] == 1 and hdr[7] == 2 and hdr[9] == SLOTS, hdr
    assert 2.0 ** 79 < hdr[8] < 2.0 ** 81  # S^2 with S = 2^80 / q_3, q_3 a 40-bit modulus


@gpu
def test_key_kinds_are_not_interchangeable(deployment):
    d, cc, la, lb = deployment
    ok(run("keyGen", cc, d / "pk2", d / "sk2"))
    ok(run("REkeyGen", cc, d / "sk", d / "pk2", d / "rk12"))
    for other, name in ((d / "rk12", "a re-encryption key"), (d / "rot_sum", "a rotation-key file"), (d / "pk", "a public key")):
        r = run("cipherProduct", cc, other, d / "a.mkws", d / "b.mkws", d / "x.mkws")
        assert r.returncode == 1 and f"is {name}, not a relinearisation key" in r.stderr, r.stderr
        assert not os.path.exists(d / "x.mkws")
    r = run("changeCipherDomain", cc, d / "relin", d / "a.mkws", d / "x.mkws")
    assert r.returncode == 1 and not os.path.exists(d / "x.mkws"), r.stdout + r.stderr
    r = run("slotSum", cc, d / "relin", d / "a.mkws", d / "x.mkws")
    assert r.returncode == 1 and "is not a rotation-key file" in r.stderr and not os.path.exists(d / "x.mkws")
