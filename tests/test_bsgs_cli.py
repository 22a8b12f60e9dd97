"""linearTransform --bsgs on the GPU, at the reference parameters (N = 2^14, depth 2, 40-bit scaling): keyGen -> rotKeyGen
--steps with exactly the list `linearTransform --bsgs-steps 4` prints for an 8 x 8 matrix (6 keys where the direct form needs
14) -> encryptModelWeights -> linearTransform --block ... --bsgs 4 -> decryptModelWeights.  The decrypted values are compared
with numpy under BSGS_BOUND of tests/test_bsgs.py (4 x the largest error of the integer definition on the CPU oracle at these
parameters; the matrix keeps every row's absolute sum, and with it sum_r |diag_r[j]|, within the 4 of that measurement).
Without --bsgs the same key file is refused by the name of a missing step (today's message), and a key file that lacks one
giant step is refused by that step's name."""
import json
import os

import numpy as np
import pytest

from tests.test_bsgs import BSGS_BOUND
from tests.test_cli_hosts import _small_cc, _weights, run
from tests.test_slot_weights_cli import ok, same

pytestmark = pytest.mark.gpu
N_DENSE, N_BIAS = 704, 8
BOUND = BSGS_BOUND["ref"]


def matrix():
    m = np.random.default_rng(88).uniform(-1.0, 1.0, size=(8, 8))
    m *= 3.5 / np.abs(m).sum(axis=1, keepdims=True)  # row absolute sums 3.5
    return np.round(m * 1024) / 1024


M = matrix()


@pytest.fixture(scope="module")
def deployment(tmp_path_factory):
    d = tmp_path_factory.mktemp("bsgs")
    cc = _small_cc(d)
    assert np.abs(M).sum(axis=1).max() <= 4
    rng = np.random.default_rng(2026)
    layers = [("dense", rng.uniform(-0.3, 0.3, N_DENSE)), ("bias", rng.uniform(-0.3, 0.3, N_BIAS))]
    (d / "matrix.json").write_text(json.dumps({"matrix": M.tolist()}))
    r = ok(run("linearTransform", cc, "--bsgs-steps", "4", "--block", d / "matrix.json"))
    steps = r.stdout.strip().split("steps=")[1]
    assert steps == "1,2,3,-8,-4,4"
    ok(run("keyGen", cc, d / "pk", d / "sk"))
    ok(run("rotKeyGen", cc, d / "sk", d / "pk", d / "rot", "--steps", steps))
    ok(run("encryptModelWeights", cc, d / "pk", _weights(d, "w.json", layers), d / "enc.mkws"))
    return d, cc, layers


def blockwise(vals):
    return (vals.reshape(-1, 8) @ M.T).reshape(-1)


def test_bsgs_block_transform_decrypts_to_the_dense_product(deployment):
    d, cc, layers = deployment
    r = ok(run("linearTransform", cc, d / "rot", "--block", d / "matrix.json", d / "enc.mkws", d / "lt.mkws", "--bsgs", "4"))
    assert "15 diagonal(s) each, 8192 slots" in r.stdout and "bsgs n1=4: 3 baby and 3 giant key(s)" in r.stdout, r.stdout
    ok(run("decryptModelWeights", cc, d / "sk", d / "lt.mkws", d / "lt.json"))
    dec = json.load(open(d / "lt.json"))["weights_summary"]
    for li, (name, vals) in enumerate(layers):
        got = np.array(dec[li]["values"])
        assert dec[li]["layer"] == name and got.shape == vals.shape
        err = np.abs(got - blockwise(vals)).max()
        print(f"{name}: |decrypted - M x| = 2^{np.log2(err):.2f}, bound 2^{np.log2(BOUND):.2f}")
        assert err <= BOUND, (name, err)
    ok(run("linearTransform", cc, d / "rot", "--block", d / "matrix.json", d / "enc.mkws", d / "lt2.mkws", "--bsgs", "4"))
    assert same(d / "lt.mkws", d / "lt2.mkws")  # no randomness on the server side


def test_the_direct_form_needs_the_keys_the_plan_saves(deployment):
    d, cc, layers = deployment
    r = run("linearTransform", cc, d / "rot", "--block", d / "matrix.json", d / "enc.mkws", d / "x.mkws")
    assert r.returncode == 1 and "[lintrans] ERROR" in r.stderr and "have no key for step -7 (Galois element" in r.stderr, r.stderr
    assert not os.path.exists(d / "x.mkws")


def test_a_key_file_that_lacks_a_giant_step_is_refused_by_name(deployment):
    d, cc, layers = deployment
    ok(run("rotKeyGen", cc, d / "sk", d / "pk", d / "rot_few", "--steps", "1,2,3,-8,4"))
    r = run("linearTransform", cc, d / "rot_few", "--block", d / "matrix.json", d / "enc.mkws", d / "y.mkws", "--bsgs", "4")
    assert r.returncode == 1 and "[lintrans] ERROR" in r.stderr and "have no key for step -4 (Galois element" in r.stderr, r.stderr
    assert not os.path.exists(d / "y.mkws")
