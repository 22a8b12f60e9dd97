"""The baby-step giant-step plan of linearTransform --bsgs (ppqsflhe_amd/host/bsgs.hpp), without a GPU: bsgs_selftest built
with -fsanitize=address,undefined as a stand-alone program (the plan rule on the steps of a 128 x 128 and a 4 x 4 block, a
repeated step, steps at +-slots/2, the plan's own formula against the diagonal method, the refusals); the roll of the
plaintexts against numpy through the program's `plan` mode; `linearTransform --bsgs-steps` on a --block file and on a
diagonals file, which needs no device and no key file."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppqsflhe_amd", "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
EXES = ("build/bsgs_selftest", "build/asan/bsgs_selftest")


@pytest.fixture(scope="module")
def selftests():
    r = subprocess.run(["make", "-C", HOST, "-s", "build/bsgs_selftest", "bsgs-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return [os.path.join(HOST, e) for e in EXES]


def clean(r):
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    return r


def test_plan_rule_and_refusals_under_sanitizers(selftests):
    for exe in selftests:
        r = clean(subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=600))
        assert "bsgs_selftest ok" in r.stdout and "FAIL" not in r.stdout, r.stdout


def reduce_step(r, slots):
    m = r % slots
    return m - slots if m > slots // 2 else m


@pytest.mark.parametrize("slots,n1,steps", [(16, "4", [1, 5, 1, 0, -11, -2]), (16, "4", [8, -8, 7, -7]), (32, "auto", list(range(-3, 4))),
                                            (64, "8", [0, 3, 9, -9, 31, -31, 17])])
def test_the_roll_of_the_plaintexts_against_numpy(selftests, tmp_path, slots, n1, steps):
    """p_{G,b} = roll(diag_{G+b}, G) (numpy rolls right for a positive shift), the values of a repeated step summed; then
    sum_G roll(sum_b p_{G,b} * roll(x, -b), -G) is the diagonal method's sum_r diag_r * roll(x, -r)."""
    rng = np.random.default_rng(len(steps) + slots)
    vals = [rng.integers(-8, 9, size=int(rng.integers(1, slots + 1))).astype(float) for _ in steps]
    doc = tmp_path / "d.json"
    doc.write_text(json.dumps({"diagonals": [{"step": r, "values": v.tolist()} for r, v in zip(steps, vals)]}))
    diag = {}
    for r, v in zip(steps, vals):
        diag.setdefault(reduce_step(r, slots), np.zeros(slots))[:len(v)] += v
    plans = []
    for exe in selftests:
        r = clean(subprocess.run([exe, "plan", str(slots), n1, str(doc)], capture_output=True, text=True, env=ENV, timeout=600))
        plans.append(json.loads(r.stdout))
    assert plans[0] == plans[1]
    p = plans[0]
    k1, giants = p["n1"], p["giants"]
    if n1 != "auto":
        assert k1 == int(n1)
    assert giants == sorted({r - r % k1 for r in diag})  # Python's % is the floor modulus
    present = np.array(p["present"]).reshape(len(giants), k1)
    values = np.array(p["values"]).reshape(len(giants), k1, slots)
    x = rng.integers(-8, 9, size=slots).astype(float)
    got = np.zeros(slots)
    for t, G in enumerate(giants):
        inner = np.zeros(slots)
        for b in range(k1):
            assert bool(present[t, b]) == (G + b in diag), (G, b)
            want = np.roll(diag[G + b], G) if G + b in diag else np.zeros(slots)
            assert np.array_equal(values[t, b], want), (G, b)
            inner += values[t, b] * np.roll(x, -b)
        got += np.roll(inner, -G)
    assert np.array_equal(got, sum(d * np.roll(x, -r) for r, d in diag.items()))
    bs = sorted({r % k1 for r in diag} - {0})
    assert p["steps"] == bs + [G for G in giants if G and G not in bs]


def test_bsgs_steps_prints_the_key_list_without_a_device(tmp_path):
    """`linearTransform <cc> --bsgs-steps <n1|auto> ...`: one line, the list rotKeyGen --steps takes (step 0 not listed)."""
    from tests.test_cli_hosts import BIN, _small_cc, run
    assert os.access(os.path.join(BIN, "linearTransform"), os.X_OK), "linearTransform not built (make -C ppqsflhe_amd/host)"
    cc = _small_cc(tmp_path)

    def doc(name, obj):
        p = tmp_path / name
        p.write_text(json.dumps(obj))
        return p

    m8 = doc("m8.json", {"matrix": np.eye(8).tolist()})
    r = run("linearTransform", cc, "--bsgs-steps", "4", "--block", m8)
    assert r.returncode == 0 and r.stdout.strip() == "[lintrans] bsgs n1=4 babies=3 giants=3 steps=1,2,3,-8,-4,4", r.stdout + r.stderr
    m128 = doc("m128.json", {"matrix": np.ones((128, 128)).tolist()})
    r = run("linearTransform", cc, "--bsgs-steps", "auto", "--block", m128)
    assert r.returncode == 0 and r.stdout.startswith("[lintrans] bsgs n1=16 babies=15 giants=15 steps=1,2,3,"), r.stdout + r.stderr
    assert len(r.stdout.strip().split("steps=")[1].split(",")) == 30
    r = run("linearTransform", cc, "--bsgs-steps", "32", "--block", m128)
    assert r.returncode == 0 and "n1=32 babies=31 giants=7 " in r.stdout, r.stdout + r.stderr
    dg = doc("d.json", {"diagonals": [{"step": r, "values": [1.0]} for r in (-3, -2, -1, 0, 1, 2, 3, 1)]})
    r = run("linearTransform", cc, "--bsgs-steps", "auto", dg)
    assert r.returncode == 0 and r.stdout.strip() == "[lintrans] bsgs n1=4 babies=3 giants=1 steps=1,2,3,-4", r.stdout + r.stderr
    r = run("linearTransform", cc, "--bsgs-steps", "2", dg)
    assert r.returncode == 0 and r.stdout.strip() == "[lintrans] bsgs n1=2 babies=1 giants=3 steps=1,-4,-2,2", r.stdout + r.stderr
    # refusals: exit 1 with the program's message
    for args, msg in [((cc, "--bsgs-steps", "x", dg), "[lintrans] ERROR: --bsgs: 'x' is neither a baby-step count nor auto"),
                      ((cc, "--bsgs-steps", "0", dg), "[lintrans] ERROR: --bsgs: '0' is neither"),
                      ((cc, "--bsgs-steps", "1", "--block", m128), "1 baby steps and 255 giant steps; at most 64"),
                      ((cc, "--bsgs-steps", "100", dg), "100 baby steps and 2 giant steps; at most 64"),
                      ((cc, "--bsgs-steps", "4", "--blocks", m8), "Usage:"),
                      ((cc, "--bsgs-steps", "4", tmp_path / "nofile.json"), "[lintrans] ERROR: diagonals: could not read"),
                      ((tmp_path / "nocc", "--bsgs-steps", "4", dg), "[lintrans] ERROR: Failed to load CryptoContext from")]:
        r = run("linearTransform", *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stdout + r.stderr)
    # --bsgs with a bad count is refused before anything is opened; without the option the usage is today's
    r = run("linearTransform", cc, "keys", dg, "in", tmp_path / "out", "--bsgs", "many")
    assert r.returncode == 1 and "--bsgs: 'many' is neither" in r.stderr and not os.path.exists(tmp_path / "out")
    r = run("linearTransform", cc, "keys", dg, "in", tmp_path / "out", "--bsgs")
    assert r.returncode == 1 and "Usage:" in r.stderr
