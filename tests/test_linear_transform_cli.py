"""linearTransform on the GPU: keyGen -> rotKeyGen --steps -> encryptModelWeights -> linearTransform --block ->
decryptModelWeights on a two-layer summary at the reference parameters (N = 2^14, depth 2, 40-bit scaling).  A 4 x 4 public
matrix is applied to every aligned block of four values; the decrypted values are compared with numpy under the bound of
tests/test_linear_transform.py (4 x the largest error of the definition on the CPU oracle at these parameters; the matrix
keeps sum_r |diag_r[j]| below the 4 of that measurement).  A key file that lacks a step is refused by the step's name."""
import json
import os

import numpy as np
import pytest

from tests.test_cli_hosts import _small_cc, _weights, run
from tests.test_linear_transform import LT_BOUND
from tests.test_slot_weights_cli import ok, same

pytestmark = pytest.mark.gpu
N_DENSE, N_BIAS = 700, 8
BOUND = LT_BOUND["ref"]
M = np.array([[0.5, -0.25, 0.125, 1.0], [0.0, 0.75, -0.5, 0.25], [-1.0, 0.5, 0.25, 0.0], [0.375, 0.0, -0.625, 0.5]])


@pytest.fixture(scope="module")
def deployment(tmp_path_factory):
    d = tmp_path_factory.mktemp("lintrans")
    cc = _small_cc(d)
    rng = np.random.default_rng(2025)
    layers = [("dense", rng.uniform(-0.3, 0.3, N_DENSE)), ("bias", rng.uniform(-0.3, 0.3, N_BIAS))]
    ok(run("keyGen", cc, d / "pk", d / "sk"))
    ok(run("rotKeyGen", cc, d / "sk", d / "pk", d / "rot", "--steps", "-3,-2,-1,1,2,3"))
    ok(run("encryptModelWeights", cc, d / "pk", _weights(d, "w.json", layers), d / "enc.mkws"))
    (d / "matrix.json").write_text(json.dumps({"matrix": M.tolist()}))
    return d, cc, layers


def decrypted(d, cc, enc, name):
    ok(run("decryptModelWeights", cc, d / "sk", enc, d / name))
    return json.load(open(d / name))["weights_summary"]


def blockwise(vals):
    return (vals.reshape(-1, 4) @ M.T).reshape(-1)


def test_block_transform_decrypts_to_the_dense_product(deployment):
    d, cc, layers = deployment
    r = ok(run("linearTransform", cc, d / "rot", "--block", d / "matrix.json", d / "enc.mkws", d / "lt.mkws"))
    assert "7 diagonal(s) each, 8192 slots" in r.stdout, r.stdout
    dec = decrypted(d, cc, d / "lt.mkws", "lt.json")
    for li, (name, vals) in enumerate(layers):
        got = np.array(dec[li]["values"])
        assert dec[li]["layer"] == name and got.shape == vals.shape
        err = np.abs(got - blockwise(vals)).max()
        print(f"{name}: |decrypted - M x| = 2^{np.log2(err):.2f}, bound 2^{np.log2(BOUND):.2f}")
        assert err <= BOUND, (name, err)
        assert abs(dec[li]["mean"] - M[0, 0] * float(np.mean(vals))) <= BOUND  # slot 0 of (mean, 0, 0, 0)
    ok(run("linearTransform", cc, d / "rot", "--block", d / "matrix.json", d / "enc.mkws", d / "lt2.mkws"))
    assert same(d / "lt.mkws", d / "lt2.mkws")  # no randomness on the server side


def test_a_diagonals_file_with_step_zero_alone_needs_no_key(deployment):
    """{"diagonals"}: a masked identity (step 0) and a rotation by one; the first with a key file that has no key at all
    for it."""
    d, cc, layers = deployment
    mask = [1.0, 0.0] * 4
    (d / "id.json").write_text(json.dumps({"diagonals": [{"step": 0, "values": mask}]}))
    ok(run("linearTransform", cc, d / "rot", d / "id.json", d / "enc.mkws", d / "id.mkws"))
    dec = decrypted(d, cc, d / "id.mkws", "id_dec.json")
    want = np.zeros(N_BIAS)
    want[:8:2] = layers[1][1][:8:2]
    assert np.abs(np.array(dec[1]["values"]) - want).max() <= BOUND
    (d / "rot1.json").write_text(json.dumps({"diagonals": [{"step": 1, "values": [2.0] * 7}, {"step": 0, "values": [1.0]}]}))
    ok(run("linearTransform", cc, d / "rot", d / "rot1.json", d / "enc.mkws", d / "r1.mkws"))
    dec = decrypted(d, cc, d / "r1.mkws", "r1_dec.json")
    v = layers[1][1]
    want = np.concatenate([2.0 * v[1:8], [0.0]])
    want[0] += v[0]
    assert np.abs(np.array(dec[1]["values"]) - want).max() <= BOUND


def test_a_key_file_that_lacks_a_step_is_refused_by_name(deployment):
    d, cc, layers = deployment
    ok(run("rotKeyGen", cc, d / "sk", d / "pk", d / "rot_few", "--steps", "-3,-2,-1,1,3"))
    r = run("linearTransform", cc, d / "rot_few", "--block", d / "matrix.json", d / "enc.mkws", d / "x.mkws")
    assert r.returncode == 1 and "[lintrans] ERROR" in r.stderr and "have no key for step 2 (Galois element 25)" in r.stderr, r.stderr
    assert not os.path.exists(d / "x.mkws")
    r = run("linearTransform", cc, d / "pk", "--block", d / "matrix.json", d / "enc.mkws", d / "x.mkws")
    assert r.returncode == 1 and "is not a rotation-key file" in r.stderr and not os.path.exists(d / "x.mkws")
