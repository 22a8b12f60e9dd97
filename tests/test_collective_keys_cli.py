"""The collective evaluation keys through the binaries, at the reference parameters (N = 2^14, depth 2, 40-bit scaling,
MKWS): three parties make a joint key (keyGen / keyGen --join), its relinearisation key in two rounds (REkeyGen to the
joint key -> fuseEvalKeys -> relinKeyGen --share -> fuseEvalKeys) and its slot-sum keys in one (rotKeyGen --sum --share
-> fuseEvalKeys); two files encrypted under the joint key are multiplied and slot-summed by the server and opened by
partialDecrypt x 3 + fuseDecryptions: nobody ever holds the joint secret.  The bound is that of
tests/test_collective_keys.py (4 x the largest error of the CPU oracle's chain at these parameters) plus 6 standard
deviations of the partial decryptions' smudging noise (the noise rule of tests/test_threshold_decrypt.py)."""
import json
import os
import struct

import numpy as np
import pytest

from tests.test_cli_hosts import _small_cc, _weights, read_key_container, run
from tests.test_collective_keys import COLLECTIVE_BOUND
from tests.test_seeded_ciphertexts import read_mkws
from tests.test_slot_weights_cli import ok, same

pytestmark = pytest.mark.gpu
N, SLOTS, PARTIES = 16384, 8192, 3
KIND_RK, KIND_ROTKEYS, KIND_RELIN, KIND_ROT_SHARE, KIND_RELIN_SHARE = 4, 9, 10, 11, 12
N_DENSE, N_BIAS = 700, 5


@pytest.fixture(scope="module")
def deployment(tmp_path_factory):
    d = tmp_path_factory.mktemp("collective")
    cc = _small_cc(d)
    rng = np.random.default_rng(2026)
    la = [("dense", rng.uniform(-0.3, 0.3, N_DENSE)), ("bias", rng.uniform(-0.3, 0.3, N_BIAS))]
    lb = [("dense", rng.uniform(-0.3, 0.3, N_DENSE)), ("bias", rng.uniform(-0.3, 0.3, N_BIAS))]
    ok(run("keyGen", cc, d / "pk0", d / "sk0"))
    for p in range(1, PARTIES):
        ok(run("keyGen", cc, d / f"pk{p}", d / f"sk{p}", "--join", d / f"pk{p - 1}"))
    joint = d / f"pk{PARTIES - 1}"
    parties = range(PARTIES)
    # relinearisation key: round 1, sum, round 2, sum
    for p in parties:
        ok(run("REkeyGen", cc, d / f"sk{p}", joint, d / f"r1_{p}"))
    r = ok(run("fuseEvalKeys", cc, d / "key1", *(d / f"r1_{p}" for p in parties)))
    assert f"[fuseevalkeys] Round-1 key of {PARTIES} parties saved to" in r.stdout
    for p in parties:
        r = ok(run("relinKeyGen", cc, d / f"sk{p}", d / "key1", d / f"r2_{p}", "--share"))
        assert "[relinkeygen] Relinearisation-key share saved to" in r.stdout
    r = ok(run("fuseEvalKeys", cc, d / "relin", *(d / f"r2_{p}" for p in parties)))
    assert f"[fuseevalkeys] Relinearisation key of {PARTIES} parties saved to" in r.stdout
    # slot-sum keys: one round, sum
    for p in parties:
        r = ok(run("rotKeyGen", cc, d / f"sk{p}", joint, d / f"rot_{p}", "--sum", SLOTS, "--share"))
        assert "13 rotation-key share(s) saved to" in r.stdout
    r = ok(run("fuseEvalKeys", cc, d / "rot", *(d / f"rot_{p}" for p in parties)))
    assert f"[fuseevalkeys] 13 rotation key(s) of {PARTIES} parties saved to" in r.stdout
    ok(run("encryptModelWeights", cc, joint, _weights(d, "a.json", la), d / "a.mkws"))
    ok(run("encryptModelWeights", cc, joint, _weights(d, "b.json", lb), d / "b.mkws"))
    return d, cc, la, lb


def kind_of(path):
    return struct.unpack("<4sII", open(path, "rb").read(12))[2]


def test_the_containers_have_their_kinds_and_the_sizes_of_the_keys_they_become(deployment):
    d, cc, _, _ = deployment
    assert [kind_of(d / f) for f in ("r1_0", "key1", "r2_0", "relin", "rot_0", "rot")] == \
        [KIND_RK, KIND_RK, KIND_RELIN_SHARE, KIND_RELIN, KIND_ROT_SHARE, KIND_ROTKEYS]
    assert os.path.getsize(d / "r2_0") == os.path.getsize(d / "relin") == os.path.getsize(d / "key1")
    assert os.path.getsize(d / "rot_0") == os.path.getsize(d / "rot")
    # the sum is the sum: key1 against the three round-1 keys, word for word (a modulus exceeds every residue, so
    # sum - key1 is 0, q, or 2 q: the same multiple-of-q set in every word of a limb, and below 3 * 2^60)
    _, _, D, parts, k1 = read_key_container(d / "key1")
    acc = np.zeros(k1.shape, dtype=object)
    for p in range(PARTIES):
        acc += read_key_container(d / f"r1_{p}")[4].astype(object)
    diff = acc - k1.astype(object)
    for i in range(D):
        steps = sorted(set(diff[:, i].ravel().tolist()))
        q = next(x for x in steps if x)
        assert q > int(k1[:, i].max()) and all(x in (0, q, 2 * q) for x in steps), (i, steps[:4])
    # the order of the shares does not matter; shares are drawn afresh
    ok(run("fuseEvalKeys", cc, d / "relin_b", d / "r2_2", d / "r2_0", d / "r2_1"))
    assert same(d / "relin", d / "relin_b")
    ok(run("relinKeyGen", cc, d / "sk0", d / "key1", d / "r2_0b", "--share"))
    assert not same(d / "r2_0", d / "r2_0b")


def test_joint_key_product_and_slot_sum_open_to_the_inner_product(deployment):
    d, cc, la, lb = deployment
    ok(run("cipherProduct", cc, d / "relin", d / "a.mkws", d / "b.mkws", d / "ab.mkws"))
    ok(run("slotSum", cc, d / "rot", d / "ab.mkws", d / "ip.mkws"))
    sigma_bits = 20  # partialDecrypt's default smudging
    for p in range(PARTIES):
        ok(run("partialDecrypt", cc, d / f"sk{p}", d / "ip.mkws", d / f"sh{p}.mkws", *(["--lead"] if p == 0 else [])))
    ok(run("fuseDecryptions", cc, *(d / f"sh{p}.mkws" for p in range(PARTIES)), d / "ip.json"))
    dec = json.load(open(d / "ip.json"))["weights_summary"]
    scale = struct.unpack("<4sIIIIIIIdII", read_mkws(d / "ip.mkws")[1][0][:48])[8]
    sd = np.sqrt(PARTIES * 4.0 ** sigma_bits * N / 2.0) / scale
    for li, ((name, va), (_, vb)) in enumerate(zip(la, lb)):
        want = float(np.dot(va, vb))
        err = np.abs(np.array(dec[li]["values"]) - want).max()
        print(f"{name}: |opened - <a, b>| = 2^{np.log2(err):.2f} (inner product {want:.6f}; smudging sd 2^{np.log2(sd):.2f})")
        assert dec[li]["layer"] == name and err <= COLLECTIVE_BOUND["ref"][1] + 6 * sd, (name, err)
    # one party alone opens nothing
    ok(run("decryptModelWeights", cc, d / "sk0", d / "ip.mkws", d / "one.json"))
    one = json.load(open(d / "one.json"))["weights_summary"]
    assert np.abs(np.array(one[0]["values"]) - float(np.dot(la[0][1], lb[0][1]))).max() > 1


def test_a_lone_share_is_refused_by_name(deployment):
    d, cc, _, _ = deployment
    out = d / "x.mkws"
    r = run("cipherProduct", cc, d / "r2_0", d / "a.mkws", d / "b.mkws", out)
    assert r.returncode == 1 and "is a relinearisation-key share, not a relinearisation key" in r.stderr, r.stderr
    r = run("cipherProduct", cc, d / "key1", d / "a.mkws", d / "b.mkws", out)
    assert r.returncode == 1 and "is a re-encryption key, not a relinearisation key" in r.stderr, r.stderr
    r = run("slotSum", cc, d / "rot_0", d / "a.mkws", out)
    assert r.returncode == 1 and "is a rotation-key share, not a rotation-key file" in r.stderr, r.stderr
    r = run("slotSum", cc, d / "r2_0", d / "a.mkws", out)
    assert r.returncode == 1 and "is not a rotation-key file" in r.stderr, r.stderr
    r = run("relinKeyGen", cc, d / "sk0", d / "relin", d / "x.key", "--share")
    assert r.returncode == 1 and "is a relinearisation key, not the round-1 key" in r.stderr, r.stderr
    assert not os.path.exists(out) and not os.path.exists(d / "x.key")
