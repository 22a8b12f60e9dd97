"""Weighted aggregation without a GPU: the C-ABI surface (declared, bound, exported; a host-only context answers
MKCKKS_E_NODEVICE), and the host arithmetic -- the weight constants over the QP basis against 128-bit arithmetic and the
--weights parser on boundary inputs -- as a stand-alone program under AddressSanitizer + UBSan."""
import os
import re
import subprocess

import pytest

from tests.test_cli_hosts import run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppqsflhe_amd", "host")
SYMBOLS = ("mkckks_scale_evk_batch", "mkckks_reencrypt_wsum_batch", "mkckks_eval_wsum_batch")


def test_weighted_symbols_are_declared_bound_and_exported():
    from ppqsflhe_amd import Context, binding
    text = open(os.path.join(ROOT, "include", "mkckks.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert sym in binding.SYMBOLS
        assert hasattr(binding.load_library(), sym)
    for method in ("scale_evk", "reencrypt_wsum", "eval_wsum"):
        assert callable(getattr(Context, method, None)), method
    assert text.count("aggregateEncryptedWeights.cpp:82-83") >= 3  # every entry point cites the lines it stands for


def test_weighted_calls_on_a_host_only_context():
    import ctypes as C
    from ppqsflhe_amd import Context
    from ppqsflhe_amd.binding import MkckksError
    c = Context(12, 2, 40, 60, dnum=2, device=-1)
    scale, wsum, esum = (getattr(c._L, s) for s in SYMBOLS)
    w = (C.c_double * 2)(0.25, 0.75)
    wp = C.addressof(w)
    far = 1 << 40  # pointers are never dereferenced
    try:
        L = c.L
        assert scale(c._h, None, far, 2, wp, 1) == -1
        assert scale(c._h, 8, far, 2, None, 1) == -1
        assert wsum(c._h, 8, 8, None, 2, 1, L, wp, 1) == -1
        assert esum(c._h, None, far, 2, 1, L, wp, 1, 0) == -1
        assert scale(c._h, 8, far, 2, wp, 1) == -2
        assert wsum(c._h, 8, 8, far, 2, 1, L, wp, 1) == -2
        assert esum(c._h, 8, far, 2, 1, L, wp, 1, 0) == -2
        assert esum(c._h, 8, far, 2, 1, L, wp, 1, 1) == -2
        for call in (lambda: c.scale_evk(8, far, 2, [0.25, 0.75], 1),
                     lambda: c.reencrypt_wsum(8, 8, far, 2, 1, L, [0.25, 0.75], 1),
                     lambda: c.eval_wsum(8, far, 2, 1, L, [0.25, 0.75], 1, True)):
            with pytest.raises(MkckksError) as ei:
                call()
            assert ei.value.code == -2
    finally:
        c.close()


def test_weight_constants_and_parser_under_asan_ubsan():
    r = subprocess.run(["make", "-C", HOST, "-s", "weights-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    r = subprocess.run([os.path.join(HOST, "build", "asan", "weights_selftest")], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("ok constants log_n=") == 3 and "ok parser" in r.stdout and "ok weights selftest" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr


@pytest.mark.parametrize("value,msg", [("1,-2", "negative"), ("1,x", "non-negative numbers"), ("1,2,3", "3 value(s) for 2 client(s)"),
                                       ("0,0", "all be zero")])
def test_aggregate_refuses_bad_weights_before_it_loads_anything(tmp_path, value, msg):
    r = run("aggregateEncryptedWeights", tmp_path / "nocc", tmp_path / "a", tmp_path / "b", tmp_path / "out", "--weights", value)
    assert r.returncode == 1 and "[agg] ERROR" in r.stderr and msg in r.stderr, r.stderr
    assert not os.path.exists(tmp_path / "out")
