"""rotKeyGen and slotSum on the GPU: keyGen -> rotKeyGen --sum -> encryptModelWeights -> slotSum --slot-weights ->
decryptModelWeights on a two-layer summary at the reference parameters (N = 2^14, depth 2, 40-bit scaling).  After the
per-slot product and the full-span slot sum every slot of a layer's ciphertext holds the inner product of the layer's
values with its factors, so every decrypted value of a layer is that one number.  The bound is the inner-product bound of
tests/test_rotation.py (4 x the largest error of the CPU oracle's composition at these parameters)."""
import base64
import json
import os

import numpy as np
import pytest

from tests.test_cli_hosts import _small_cc, _weights, run
from tests.test_rotation import SUM_BOUND
from tests.test_seeded_ciphertexts import mkws_to_json
from tests.test_slot_weights_cli import factors, ok, same

pytestmark = pytest.mark.gpu
N_DENSE, N_BIAS, SLOTS = 700, 5, 8192
BOUND = SUM_BOUND["ref"][1]


@pytest.fixture(scope="module")
def deployment(tmp_path_factory):
    d = tmp_path_factory.mktemp("rot")
    cc = _small_cc(d)
    rng = np.random.default_rng(2024)
    layers = [("dense", rng.uniform(-0.3, 0.3, N_DENSE)), ("bias", rng.uniform(-0.3, 0.3, N_BIAS))]
    w = [("dense", 0.5, 0.25, rng.uniform(0.0, 1.0, N_DENSE)), ("bias", 1.0, 0.0, rng.uniform(0.0, 1.0, N_BIAS))]
    ok(run("keyGen", cc, d / "pk", d / "sk"))
    r = ok(run("rotKeyGen", cc, d / "sk", d / "pk", d / "rot_sum", "--sum", SLOTS))
    assert "[rotkeygen] 13 rotation key(s) saved" in r.stdout, r.stdout
    plain = _weights(d, "w.json", layers)
    ok(run("encryptModelWeights", cc, d / "pk", plain, d / "enc.mkws"))
    return d, cc, layers, w, factors(d, "ref_vector.json", w)


def decrypted(d, cc, enc, name):
    ok(run("decryptModelWeights", cc, d / "sk", enc, d / name))
    return json.load(open(d / name))["weights_summary"]


def test_slot_sum_with_slot_weights_decrypts_to_the_inner_product(deployment):
    d, cc, layers, w, fac = deployment
    r = ok(run("slotSum", cc, d / "rot_sum", d / "enc.mkws", d / "ip.mkws", "--slot-weights", fac))
    assert "span 8192, 13 rotation(s) each, after the per-slot product" in r.stdout, r.stdout
    dec = decrypted(d, cc, d / "ip.mkws", "ip.json")
    for li, ((name, vals), (_, fm, fs, fv)) in enumerate(zip(layers, w)):
        want = float(np.dot(vals, fv))
        got = np.array(dec[li]["values"])
        assert dec[li]["layer"] == name and got.shape == (len(vals),)
        err = np.abs(got - want).max()
        print(f"{name}: |decrypted - <values, factors>| = 2^{np.log2(err):.2f} (inner product {want:.6f})")
        assert err <= BOUND, (name, err)
        assert abs(dec[li]["mean"] - float(np.mean(vals)) * fm) <= BOUND
        assert abs(dec[li]["std_dev"] - float(np.std(vals)) * fs) <= BOUND


def test_plain_slot_sum_and_a_partial_span(deployment):
    """Without --slot-weights every slot holds the sum of the layer's values; --span 8 leaves windowed sums: value j is
    v[j] + ... + v[j + 7] (zero padded past the layer's end)."""
    d, cc, layers, w, fac = deployment
    ok(run("slotSum", cc, d / "rot_sum", d / "enc.mkws", d / "sum.mkws"))
    dec = decrypted(d, cc, d / "sum.mkws", "sum.json")
    for li, (name, vals) in enumerate(layers):
        assert np.abs(np.array(dec[li]["values"]) - float(np.sum(vals))).max() <= SUM_BOUND["ref"][0], name
    ok(run("slotSum", cc, d / "rot_sum", d / "enc.mkws", d / "win.mkws", "--span", "8"))
    dec = decrypted(d, cc, d / "win.mkws", "win.json")
    for li, (name, vals) in enumerate(layers):
        padded = np.concatenate([vals, np.zeros(8)])
        want = np.array([padded[j:j + 8].sum() for j in range(len(vals))])
        assert np.abs(np.array(dec[li]["values"]) - want).max() <= SUM_BOUND["ref"][0], name


def test_json_and_mkws_inputs_give_the_same_ciphertext_bytes(deployment):
    """ONE encryption in both envelope forms (the MKWS file re-written as JSON with base64 blobs): the outputs keep their
    input's form and hold the same ciphertext containers; a span of 1 returns the input's containers."""
    d, cc, layers, w, fac = deployment
    mkws_to_json(d / "enc.mkws", d / "enc.json")
    ok(run("slotSum", cc, d / "rot_sum", d / "enc.mkws", d / "ip2.mkws", "--slot-weights", fac))
    ok(run("slotSum", cc, d / "rot_sum", d / "enc.json", d / "ip2.json", "--slot-weights", fac))
    mkws_to_json(d / "ip2.mkws", d / "ip2_from_mkws.json")
    a, b = json.load(open(d / "ip2.json")), json.load(open(d / "ip2_from_mkws.json"))
    assert a == b and len(a["weights_summary"]) == 2
    assert len(base64.b64decode(a["weights_summary"][0]["values"][0])) == 48 + 8 * 2 * 3 * 16384  # 3 limbs after the rescale
    ok(run("slotSum", cc, d / "rot_sum", d / "enc.mkws", d / "ip3.mkws", "--slot-weights", fac))
    assert same(d / "ip2.mkws", d / "ip3.mkws")  # no randomness on the server side
    ok(run("slotSum", cc, d / "rot_sum", d / "enc.json", d / "copy.json", "--span", "1"))
    assert json.load(open(d / "copy.json")) == json.load(open(d / "enc.json"))


def test_a_key_file_that_lacks_a_step_is_refused_by_name(deployment):
    d, cc, layers, w, fac = deployment
    ok(run("rotKeyGen", cc, d / "sk", d / "pk", d / "rot_few", "--steps", "1,2,-3,8"))
    r = run("slotSum", cc, d / "rot_few", d / "enc.mkws", d / "x.mkws")
    assert r.returncode == 1 and "[slotsum] ERROR" in r.stderr and "have no key for step 4 (Galois element 625)" in r.stderr, r.stderr
    assert not os.path.exists(d / "x.mkws")
    ok(run("slotSum", cc, d / "rot_few", d / "enc.mkws", d / "four.mkws", "--span", "4"))   # steps 1 and 2 are there
    ok(run("slotSum", cc, d / "rot_sum", d / "enc.mkws", d / "four_ref.mkws", "--span", "4"))
    a, b = decrypted(d, cc, d / "four.mkws", "four.json"), decrypted(d, cc, d / "four_ref.mkws", "four_ref.json")
    for li in range(2):  # other key randomness, the same sums
        assert np.abs(np.array(a[li]["values"]) - np.array(b[li]["values"])).max() <= 2 * SUM_BOUND["ref"][0]
    r = run("slotSum", cc, d / "pk", d / "enc.mkws", d / "x.mkws")  # a file that is no rotation-key file
    assert r.returncode == 1 and "is not a rotation-key file" in r.stderr and not os.path.exists(d / "x.mkws")
