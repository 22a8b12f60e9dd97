"""--weights of serverRound / aggregateEncryptedWeights on the GPU: the weighted mean by sample count, through the
synchronous path, the MKWS pipeline and --rounds (where scaled key copies are kept), and the refusals."""
import json
import os

import numpy as np
import pytest

from tests.test_cli_hosts import _small_cc, _weights, run

pytestmark = pytest.mark.gpu
N_CLIENTS, TARGET = 3, 2


def ok(r):
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def same(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


@pytest.fixture(scope="module")
def deployment(tmp_path_factory):
    """Three clients' keys and encrypted weights (MKWS), re-encryption keys of clients 0 and 1 into client 2's domain and
    their re-encrypted files: made once for the module."""
    d = tmp_path_factory.mktemp("weighted")
    cc = _small_cc(d)
    rng = np.random.default_rng(63)
    vals = [[("dense", rng.uniform(-0.3, 0.3, 700)), ("bias", rng.uniform(-0.3, 0.3, 5))] for _ in range(N_CLIENTS)]
    for c in range(N_CLIENTS):
        ok(run("keyGen", cc, d / f"pk{c}", d / f"sk{c}"))
        ok(run("encryptModelWeights", cc, d / f"pk{c}", _weights(d, f"w{c}.json", vals[c]), d / f"enc{c}.mkws"))
    for c in range(N_CLIENTS - 1):
        ok(run("REkeyGen", cc, d / f"sk{c}", d / f"pk{TARGET}", d / f"rk{c}"))
        ok(run("changeCipherDomain", cc, d / f"rk{c}", d / f"enc{c}.mkws", d / f"pre{c}.mkws"))
    # argument order of every round below: the in-domain client first, then clients 0 and 1 with their keys
    args = ["-", d / f"enc{TARGET}.mkws", d / "rk0", d / "enc0.mkws", d / "rk1", d / "enc1.mkws"]
    order = [TARGET, 0, 1]
    return d, cc, vals, args, order


def weighted_mean(vals, order, counts, layer):
    w = np.asarray(counts, dtype=np.float64)
    return sum(w[k] / w.sum() * np.asarray(vals[c][layer][1]) for k, c in enumerate(order))


def test_weighted_round_decrypts_to_the_weighted_mean_on_both_io_paths(deployment):
    d, cc, vals, args, order = deployment
    ra = ok(run("serverRound", cc, d / "aggA.mkws", *args, "--weights", "3,1,4", env={"MKCKKS_SYNC_IO": "1"}))
    rb = ok(run("serverRound", cc, d / "aggB.mkws", *args, "--weights", "3,1,4"))
    assert "[round] timing:" in rb.stdout and "[round] timing:" not in ra.stdout
    assert same(d / "aggA.mkws", d / "aggB.mkws")
    ok(run("decryptModelWeights", cc, d / f"sk{TARGET}", d / "aggB.mkws", d / "dec.json"))
    dec = json.load(open(d / "dec.json"))["weights_summary"]
    for li in range(2):
        err = np.abs(np.array(dec[li]["values"]) - weighted_mean(vals, order, [3, 1, 4], li)).max()
        print(f"layer {li}: |decrypted - weighted mean| = 2^{np.log2(err):.2f}")
        assert err < 2.0 ** -25, (li, err)
    # the option may stand anywhere after the output file, and sample counts need no normalising
    ok(run("serverRound", cc, d / "aggC.mkws", "--weights", "0.375,0.125,0.5", *args))
    ok(run("decryptModelWeights", cc, d / f"sk{TARGET}", d / "aggC.mkws", d / "decC.json"))
    decC = json.load(open(d / "decC.json"))["weights_summary"]
    assert np.abs(np.array(decC[0]["values"]) - weighted_mean(vals, order, [3, 1, 4], 0)).max() < 2.0 ** -25
    # it is not the plain mean
    assert np.abs(np.array(dec[0]["values"]) - weighted_mean(vals, order, [1, 1, 1], 0)).max() > 2.0 ** -10


def test_aggregate_weights_equals_server_round_with_in_domain_clients(deployment):
    d, cc, vals, args, order = deployment
    files = [d / f"enc{TARGET}.mkws", d / "pre0.mkws", d / "pre1.mkws"]
    ok(run("aggregateEncryptedWeights", cc, files[0], files[1], d / "inA.mkws", files[2], "--weights", "3,1,4"))
    for name, env in (("inB.mkws", {}), ("inC.mkws", {"MKCKKS_SYNC_IO": "1"})):
        ok(run("serverRound", cc, d / name, "-", files[0], "-", files[1], "-", files[2], "--weights", "3,1,4", env=env))
        assert same(d / "inA.mkws", d / name), name
    ok(run("decryptModelWeights", cc, d / f"sk{TARGET}", d / "inA.mkws", d / "decA.json"))
    dec = json.load(open(d / "decA.json"))["weights_summary"]
    assert np.abs(np.array(dec[0]["values"]) - weighted_mean(vals, order, [3, 1, 4], 0)).max() < 2.0 ** -25


def test_rounds_with_changing_weights_remake_the_scaled_keys(deployment):
    """Two rounds in one process that name the same keys and files but carry different weights, then the first weights
    again, then none: every round's output is that of a one-shot run with its line's weights (a scaled key kept from
    the round before would give a wrong aggregate without any error)."""
    d, cc, vals, args, order = deployment
    lines = [("r1.mkws", "3,1,4"), ("r2.mkws", "1,5,2"), ("r3.mkws", "3,1,4"), ("r4.mkws", None), ("r5.mkws", "1,5,2")]
    rounds = d / "rounds.txt"
    rounds.write_text("".join(" ".join(map(str, [d / out, *args] + (["--weights", w] if w else []))) + "\n" for out, w in lines))
    rr = ok(run("serverRound", cc, "--rounds", rounds))
    assert "[round] 5 rounds, " in rr.stdout
    for w, one in (("3,1,4", "one_a.mkws"), ("1,5,2", "one_b.mkws"), (None, "one_c.mkws")):
        ok(run("serverRound", cc, d / one, *args, *(["--weights", w] if w else [])))
    assert same(d / "r1.mkws", d / "one_a.mkws") and same(d / "r3.mkws", d / "one_a.mkws")
    assert same(d / "r2.mkws", d / "one_b.mkws") and same(d / "r5.mkws", d / "one_b.mkws")
    assert same(d / "r4.mkws", d / "one_c.mkws")
    assert not same(d / "r1.mkws", d / "r2.mkws") and not same(d / "r1.mkws", d / "r4.mkws")


def test_without_weights_the_round_is_the_per_client_programs(deployment):
    d, cc, vals, args, order = deployment
    ok(run("aggregateEncryptedWeights", cc, d / f"enc{TARGET}.mkws", d / "pre0.mkws", d / "plainA.mkws", d / "pre1.mkws"))
    ok(run("serverRound", cc, d / "plainB.mkws", *args))
    ok(run("serverRound", cc, d / "plainC.mkws", *args, env={"MKCKKS_SYNC_IO": "1"}))
    assert same(d / "plainA.mkws", d / "plainB.mkws") and same(d / "plainA.mkws", d / "plainC.mkws")


def test_weighted_round_refusals(deployment):
    d, cc, vals, args, order = deployment
    for value, msg in (("3,1", "2 value(s) for 3 client(s)"), ("3,1,4,1", "4 value(s) for 3 client(s)"),
                       ("3,-1,4", "a weight is negative"), ("3,nan,4", "non-negative numbers"), ("3,,4", "non-negative numbers"),
                       ("0,0,0", "must not all be zero")):
        for env in ({}, {"MKCKKS_SYNC_IO": "1"}):
            r = run("serverRound", cc, d / "x.mkws", *args, "--weights", value, env=env)
            assert r.returncode == 1 and "[round] ERROR" in r.stderr and msg in r.stderr, (value, r.stderr)
    r = run("serverRound", cc, d / "x.mkws", *args, "--weights")  # no value
    assert r.returncode == 1 and "Usage:" in r.stderr
    # no headroom: aggregates of aggregates are down to 2 limbs (100 bits) at a scale of ~2^80; times sf ~ 2^40 that is over
    ok(run("serverRound", cc, d / "lvl1.mkws", *args))
    ok(run("serverRound", cc, d / "lvl2.mkws", "-", d / "lvl1.mkws", "-", d / "lvl1.mkws"))
    for env in ({}, {"MKCKKS_SYNC_IO": "1"}):
        r = run("serverRound", cc, d / "x.mkws", "-", d / "lvl2.mkws", "-", d / "lvl2.mkws", "--weights", "1,1", env=env)
        assert r.returncode == 1 and "[round] ERROR" in r.stderr and "no headroom" in r.stderr, r.stderr
    r = run("aggregateEncryptedWeights", cc, d / "lvl2.mkws", d / "lvl2.mkws", d / "x.mkws", "--weights", "1,1")
    assert r.returncode == 1 and "[agg] ERROR" in r.stderr and "no headroom" in r.stderr, r.stderr
    assert not os.path.exists(d / "x.mkws")
    ok(run("serverRound", cc, d / "lvl2w.mkws", "-", d / "lvl1.mkws", "-", d / "lvl1.mkws", "--weights", "1,3"))  # 3 limbs: room
