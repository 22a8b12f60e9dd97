"""--slot-weights of serverRound / aggregateEncryptedWeights on the GPU: a round whose clients cover different coordinates
divided per coordinate by the number of clients that cover it, through the per-client programs, the synchronous path, the
MKWS pipeline and --rounds (where the encoded factors stay resident), and the refusals that need ciphertexts."""
import json
import os

import numpy as np
import pytest

from tests.test_cli_hosts import _small_cc, _weights, run

pytestmark = pytest.mark.gpu
N_CLIENTS, TARGET = 3, 2
N_DENSE, N_BIAS, BATCH = 700, 5, 256  # 700 values = ciphertexts of 256, 256 and 188 values


def ok(r):
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def same(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


def factors(d, name, layers):
    """A --slot-weights file: [(layer, mean factor, std_dev factor, value factors)]."""
    p = d / name
    p.write_text(json.dumps({"weights_summary": [
        {"layer": n, "shape": [len(v)], "mean": float(m), "std_dev": float(sd), "values": [float(x) for x in v]}
        for n, m, sd, v in layers]}))
    return p


@pytest.fixture(scope="module")
def deployment(tmp_path_factory):
    """Three clients' keys and encrypted weights (MKWS, 256 values per ciphertext); client c sends zeros at the coordinates
    j < 600 of "dense" with j % 4 == c.  Re-encryption keys of clients 0 and 1 into client 2's domain and their
    re-encrypted files: made once for the module."""
    d = tmp_path_factory.mktemp("slotw")
    cc = _small_cc(d, batch=BATCH)
    rng = np.random.default_rng(64)
    j = np.arange(N_DENSE)
    cover = np.stack([~((j < 600) & (j % 4 == c)) for c in range(N_CLIENTS)])
    vals = []
    for c in range(N_CLIENTS):
        dense = rng.uniform(-0.3, 0.3, N_DENSE) * cover[c]
        vals.append([("dense", dense), ("bias", rng.uniform(-0.3, 0.3, N_BIAS))])
    for c in range(N_CLIENTS):
        ok(run("keyGen", cc, d / f"pk{c}", d / f"sk{c}"))
        ok(run("encryptModelWeights", cc, d / f"pk{c}", _weights(d, f"w{c}.json", vals[c]), d / f"enc{c}.mkws"))
    for c in range(N_CLIENTS - 1):
        ok(run("REkeyGen", cc, d / f"sk{c}", d / f"pk{TARGET}", d / f"rk{c}"))
        ok(run("changeCipherDomain", cc, d / f"rk{c}", d / f"enc{c}.mkws", d / f"pre{c}.mkws"))
    args = ["-", d / f"enc{TARGET}.mkws", d / "rk0", d / "enc0.mkws", d / "rk1", d / "enc1.mkws"]
    count = cover.sum(axis=0)
    assert count.min() == 2 and count.max() == 3
    third = 1.0 / N_CLIENTS
    het = factors(d, "het.json", [("dense", third, third, 1.0 / count), ("bias", third, third, np.full(N_BIAS, third))])
    flat = factors(d, "flat.json", [("dense", third, third, np.full(N_DENSE, third)), ("bias", third, third, np.full(N_BIAS, third))])
    return d, cc, vals, args, count, het, flat


def decrypted(d, cc, agg, name):
    ok(run("decryptModelWeights", cc, d / f"sk{TARGET}", d / agg, d / name))
    return json.load(open(d / name))["weights_summary"]


def test_heterogeneous_round_is_the_mean_over_the_covering_clients(deployment):
    """serverRound against changeCipherDomain + aggregateEncryptedWeights: the same bytes, and they decrypt to the
    per-coordinate mean over the clients that cover a coordinate (not to the plain mean)."""
    d, cc, vals, args, count, het, flat = deployment
    ok(run("serverRound", cc, d / "hetA.mkws", *args, "--slot-weights", het))
    ok(run("aggregateEncryptedWeights", cc, d / f"enc{TARGET}.mkws", d / "pre0.mkws", d / "hetB.mkws", d / "pre1.mkws",
           "--slot-weights", het))
    assert same(d / "hetA.mkws", d / "hetB.mkws")
    ok(run("serverRound", cc, d / "hetC.mkws", "--slot-weights", het, *args))  # the option may stand anywhere after the output file
    assert same(d / "hetA.mkws", d / "hetC.mkws")
    dec = decrypted(d, cc, "hetA.mkws", "hetA.json")
    total = sum(np.asarray(vals[c][0][1]) for c in range(N_CLIENTS))
    err = np.abs(np.array(dec[0]["values"]) - total / count).max()
    print(f"dense: |decrypted - mean over the covering clients| = 2^{np.log2(err):.2f}")
    assert err < 2.0 ** -25, err
    assert np.abs(np.array(dec[0]["values"]) - total / N_CLIENTS).max() > 2.0 ** -10  # where a client sat out, not the plain mean
    bias = sum(np.asarray(vals[c][1][1]) for c in range(N_CLIENTS)) / N_CLIENTS
    assert np.abs(np.array(dec[1]["values"]) - bias).max() < 2.0 ** -25
    means = sum(float(np.mean(vals[c][0][1])) for c in range(N_CLIENTS)) / N_CLIENTS
    assert abs(dec[0]["mean"] - means) < 2.0 ** -25


def test_factors_of_one_nth_equal_the_plain_round(deployment):
    d, cc, vals, args, count, het, flat = deployment
    ok(run("serverRound", cc, d / "flat.mkws", *args, "--slot-weights", flat))
    ok(run("serverRound", cc, d / "plain.mkws", *args))
    a, b = decrypted(d, cc, "flat.mkws", "flat_dec.json"), decrypted(d, cc, "plain.mkws", "plain_dec.json")
    for li in range(2):
        assert np.abs(np.array(a[li]["values"]) - np.array(b[li]["values"])).max() < 2.0 ** -25, li
        assert abs(a[li]["mean"] - b[li]["mean"]) < 2.0 ** -25 and abs(a[li]["std_dev"] - b[li]["std_dev"]) < 2.0 ** -25
    # the headers agree: the result sits where the plain round's does (limbs, level, scale, noiseScaleDeg)
    assert os.path.getsize(d / "flat.mkws") == os.path.getsize(d / "plain.mkws")


def test_two_rounds_keep_the_encoded_factors_resident(deployment):
    d, cc, vals, args, count, het, flat = deployment
    rounds = d / "rounds.txt"
    rounds.write_text("".join(" ".join(map(str, [d / out, *args, "--slot-weights", f])) + "\n"
                              for out, f in (("r1.mkws", het), ("r2.mkws", het), ("r3.mkws", flat), ("r4.mkws", het))))
    rr = ok(run("serverRound", cc, "--rounds", rounds))
    assert "[round] 4 rounds, " in rr.stdout
    assert rr.stdout.count("plaintext(s) encoded") == 3 and rr.stdout.count("plaintext(s) resident") == 1
    ok(run("serverRound", cc, d / "one_het.mkws", *args, "--slot-weights", het))
    ok(run("serverRound", cc, d / "one_flat.mkws", *args, "--slot-weights", flat))
    for r in ("r1.mkws", "r2.mkws", "r4.mkws"):
        assert same(d / r, d / "one_het.mkws"), r
    assert same(d / "r3.mkws", d / "one_flat.mkws") and not same(d / "r3.mkws", d / "r1.mkws")


def test_pipeline_writes_the_bytes_of_the_synchronous_path(deployment):
    d, cc, vals, args, count, het, flat = deployment
    ra = ok(run("serverRound", cc, d / "syncA.mkws", *args, "--slot-weights", het, env={"MKCKKS_SYNC_IO": "1"}))
    rb = ok(run("serverRound", cc, d / "pipeB.mkws", *args, "--slot-weights", het))
    assert "[round] timing:" in rb.stdout and "[round] timing:" not in ra.stdout
    assert same(d / "syncA.mkws", d / "pipeB.mkws")
    rc = ok(run("serverRound", cc, d / "pipeC.mkws", *args, "--slot-weights", het, env={"MKCKKS_ROUND_CHUNK": "3"}))
    assert "chunks of 3" in rc.stdout and same(d / "syncA.mkws", d / "pipeC.mkws")  # chunks that do not divide the 8 items


def test_refusals_that_need_the_round(deployment):
    """A layer of the round the file lacks, another shape, another value count, no headroom for max|factor|: exit 1, the
    program's ERROR line, no output file -- on both I/O paths and in aggregateEncryptedWeights."""
    d, cc, vals, args, count, het, flat = deployment
    third = 1.0 / 3
    bad = [(factors(d, "nolayer.json", [("dense", third, third, np.full(N_DENSE, third))]), "layer bias of the round is absent"),
           (factors(d, "huge.json", [("dense", third, third, np.full(N_DENSE, 2.0 ** 70)), ("bias", third, third, np.full(N_BIAS, third))]),
            "no headroom")]
    shape = json.load(open(flat))
    shape["weights_summary"][1]["shape"] = [1, N_BIAS]
    (d / "shape.json").write_text(json.dumps(shape))
    bad.append((d / "shape.json", "layer bias has another shape"))
    short = json.load(open(flat))
    short["weights_summary"][0]["values"] = short["weights_summary"][0]["values"][:2 * BATCH]  # the shape stays, a ciphertext is missing
    (d / "count.json").write_text(json.dumps(short))
    bad.append((d / "count.json", "512 value(s) = 2 ciphertext(s) in the file, the round has 3"))
    for f, msg in bad:
        for env in ({}, {"MKCKKS_SYNC_IO": "1"}):
            r = run("serverRound", cc, d / "x.mkws", *args, "--slot-weights", f, env=env)
            assert r.returncode == 1 and "[round] ERROR" in r.stderr and msg in r.stderr, (msg, r.stderr)
            assert not os.path.exists(d / "x.mkws")
        r = run("aggregateEncryptedWeights", cc, d / f"enc{TARGET}.mkws", d / "pre0.mkws", d / "x.mkws", d / "pre1.mkws", "--slot-weights", f)
        assert r.returncode == 1 and "[agg] ERROR" in r.stderr and msg in r.stderr, (msg, r.stderr)
        assert not os.path.exists(d / "x.mkws")
    # aggregates of aggregates are down to 2 limbs (100 bits) at a scale of ~2^80: times sf ~ 2^40 there is no room for factors of 1/2
    ok(run("serverRound", cc, d / "lvl1.mkws", *args))
    ok(run("serverRound", cc, d / "lvl2.mkws", "-", d / "lvl1.mkws", "-", d / "lvl1.mkws"))
    r = run("serverRound", cc, d / "x.mkws", "-", d / "lvl2.mkws", "-", d / "lvl2.mkws", "--slot-weights", flat)
    assert r.returncode == 1 and "[round] ERROR" in r.stderr and "no headroom" in r.stderr, r.stderr
    assert not os.path.exists(d / "x.mkws")
