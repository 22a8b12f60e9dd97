"""Per-slot aggregation weights without a GPU: the C-ABI surface (declared, bound, exported; argument checks and
MKCKKS_E_NODEVICE on a host-only context), the --slot-weights host code -- the file-to-slot-vector mapping and the headroom
rule on boundary inputs -- as a stand-alone program under AddressSanitizer + UBSan, and the refusals of the two hosts that
are decided before anything is loaded.  (The refusals that need the round's ciphertexts -- an absent layer, another shape
or value count, no headroom -- are in tests/test_slot_weights_cli.py: the hosts cannot read a ciphertext without a device.)"""
import json
import os
import re
import subprocess

import pytest

from tests.test_cli_hosts import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppqsflhe_amd", "host")
SYMBOLS = ("mkckks_mult_plain_batch", "mkckks_mult_plain_rescale_batch")


def test_slot_weight_symbols_are_declared_bound_and_exported():
    from ppqsflhe_amd import Context, binding
    text = open(os.path.join(ROOT, "include", "mkckks.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert sym in binding.SYMBOLS
        assert hasattr(binding.load_library(), sym)
        # every entry point cites the lines it stands for, in the comment right above its declaration
        above = text[:text.index("int %s(" % sym)]
        assert "aggregateEncryptedWeights.cpp:82-83" in above[above.rindex("/*"):], sym
    for method in ("mult_plain", "mult_plain_rescale"):
        assert callable(getattr(Context, method, None)), method


def test_slot_weight_calls_on_a_host_only_context():
    from ppqsflhe_amd import Context
    from ppqsflhe_amd.binding import MkckksError
    c = Context(12, 2, 40, 60, dnum=2, device=-1)
    mul, resc = (getattr(c._L, s) for s in SYMBOLS)
    far = 1 << 40  # pointers are never dereferenced
    try:
        L = c.L
        # MKCKKS_E_INVALID: null pointers, n_pt outside {1, n_ct}, nl < 2 for the rescaling call, nl > L
        assert mul(c._h, None, 8, 2, 2, L) == -1
        assert mul(c._h, 8, None, 2, 2, L) == -1
        assert resc(c._h, None, 8, far, 2, 2, L) == -1
        assert resc(c._h, 8, None, far, 2, 2, L) == -1
        assert resc(c._h, 8, 8, None, 2, 2, L) == -1
        for n_ct, n_pt in ((2, 0), (2, 3), (3, 2), (1, 2)):
            assert mul(c._h, 8, far, n_ct, n_pt, L) == -1, (n_ct, n_pt)
            assert resc(c._h, 8, 8, far, n_ct, n_pt, L) == -1, (n_ct, n_pt)
        assert resc(c._h, 8, 8, far, 2, 2, 1) == -1
        assert resc(c._h, 8, 8, far, 2, 2, 0) == -1 and mul(c._h, 8, far, 2, 2, 0) == -1
        assert resc(c._h, 8, 8, far, 2, 2, L + 1) == -1 and mul(c._h, 8, far, 2, 2, L + 1) == -1
        assert mul(None, 8, far, 2, 2, L) == -1 and resc(None, 8, 8, far, 2, 2, L) == -1
        # MKCKKS_E_NODEVICE: well-formed calls
        for n_ct, n_pt in ((2, 2), (2, 1), (1, 1)):
            assert mul(c._h, 8, far, n_ct, n_pt, L) == -2
            assert mul(c._h, 8, far, n_ct, n_pt, 1) == -2
            assert resc(c._h, 8, 8, far, n_ct, n_pt, L) == -2
            assert resc(c._h, 8, 8, far, n_ct, n_pt, 2) == -2
        for call in (lambda: c.mult_plain(8, far, 2, 2, L), lambda: c.mult_plain_rescale(8, 8, far, 2, 1, L)):
            with pytest.raises(MkckksError) as ei:
                call()
            assert ei.value.code == -2
    finally:
        c.close()


def test_slot_weight_mapping_and_headroom_under_asan_ubsan():
    r = subprocess.run(["make", "-C", HOST, "-s", "slotweights-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    r = subprocess.run([os.path.join(HOST, "build", "asan", "slotweights_selftest")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for line in ("ok mapping", "ok parser", "ok headroom", "ok slotweights selftest"):
        assert line in r.stdout, r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


def _factor_file(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return p


LAYER = '{"layer": "dense", "shape": [2], "mean": 0.5, "std_dev": 0.5, "values": [0.5, %s]}'


def refusals(tmp_path):
    """(arguments after the positional ones, text in the ERROR line): all decided before the context file is read."""
    ok_file = _factor_file(tmp_path, "ok.json", '{"weights_summary": [%s]}' % (LAYER % "1"))
    return [(["--slot-weights", ok_file, "--weights", "1,1"], "cannot be combined with --weights"),
            (["--weights", "1,1", "--slot-weights", ok_file], "cannot be combined with --weights"),
            (["--slot-weights"], "--slot-weights needs a file"),
            (["--slot-weights", tmp_path / "missing.json"], "could not read"),
            (["--slot-weights", tmp_path], "could not read"),  # a directory
            (["--slot-weights", _factor_file(tmp_path, "trunc.json", '{"weights_summary": [')], "could not read"),
            (["--slot-weights", _factor_file(tmp_path, "other.json", '{"layers": []}')], "not a weights_summary"),
            (["--slot-weights", _factor_file(tmp_path, "text.json", '{"weights_summary": [%s]}' % (LAYER % '"x"'))], "not a weights_summary"),
            (["--slot-weights", _factor_file(tmp_path, "inf.json", '{"weights_summary": [%s]}' % (LAYER % "1e999"))], "is not finite"),
            (["--slot-weights", _factor_file(tmp_path, "ninf.json", '{"weights_summary": [%s]}' % (LAYER % "-1e999"))], "is not finite")]


def test_aggregate_refuses_bad_slot_weights_before_it_loads_anything(tmp_path):
    for extra, msg in refusals(tmp_path):
        r = run("aggregateEncryptedWeights", tmp_path / "nocc", tmp_path / "a", tmp_path / "b", tmp_path / "out", *extra)
        assert r.returncode == 1 and "[agg] ERROR" in r.stderr and msg in r.stderr, (extra, r.stderr)
        assert "CryptoContext" not in r.stderr  # refused before the context file is read
        assert not os.path.exists(tmp_path / "out")


def test_server_round_refuses_bad_slot_weights_before_it_loads_anything(tmp_path):
    for extra, msg in refusals(tmp_path):
        r = run("serverRound", tmp_path / "nocc", tmp_path / "out", "-", tmp_path / "a", "-", tmp_path / "b", *extra)
        assert r.returncode == 1 and "[round] ERROR" in r.stderr and msg in r.stderr, (extra, r.stderr)
        assert "CryptoContext" not in r.stderr
        assert not os.path.exists(tmp_path / "out")
    # a line of a --rounds file is judged the same way
    rounds = tmp_path / "rounds.txt"
    rounds.write_text(" ".join(map(str, [tmp_path / "out", "-", tmp_path / "a", "-", tmp_path / "b", "--slot-weights",
                                         tmp_path / "missing.json"])) + "\n")
    r = run("serverRound", tmp_path / "nocc", "--rounds", rounds)
    assert r.returncode == 1 and "[round] ERROR" in r.stderr and "could not read" in r.stderr and "CryptoContext" not in r.stderr


def test_a_well_formed_file_gets_as_far_as_the_context(tmp_path):
    """The same arguments with a readable file pass the early checks: the next error is the missing context file."""
    ok_file = _factor_file(tmp_path, "ok.json", json.dumps({"weights_summary": [
        {"layer": "dense", "shape": [2], "mean": 0.5, "std_dev": 0.5, "values": [0.5, 0.0]},
        {"layer": "optimizer/iter", "shape": [], "mean": 1e999, "std_dev": 0, "values": []}]}).replace("Infinity", "1e999"))
    r = run("aggregateEncryptedWeights", tmp_path / "nocc", tmp_path / "a", tmp_path / "b", tmp_path / "out", "--slot-weights", ok_file)
    assert r.returncode == 1 and "[agg] ERROR: Failed to load CryptoContext" in r.stderr
    r = run("serverRound", tmp_path / "nocc", tmp_path / "out", "-", tmp_path / "a", "-", tmp_path / "b", "--slot-weights", ok_file)
    assert r.returncode == 1 and "[round] ERROR: Failed to load CryptoContext" in r.stderr
