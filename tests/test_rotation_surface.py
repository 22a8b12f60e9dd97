"""Slot rotations and slot sums, the part that needs no GPU (include/mkckks.h: "slot rotations and slot sums"):
the symbols are declared, bound and exported; mkckks_galois_element on a host-only context; every refusal of the compute
calls, decided before a device is asked for; the index arithmetic of ppqsflhe_amd/csrc/galois.hpp as a stand-alone program
under -fsanitize=address,undefined (galois_selftest.cpp: permutation, defining congruence, block property, pair property,
sigma_g then sigma_{g^-1} on a ternary vector, 5^r 5^-r = 1)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ppqsflhe_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
SYMBOLS = ("mkckks_galois_element", "mkckks_automorphism_batch", "mkckks_automorphism_secret", "mkckks_galois_keygen",
           "mkckks_rotate_batch", "mkckks_slot_sum_batch")
METHODS = ("galois_element", "automorphism", "automorphism_secret", "galois_keygen", "rotate", "slot_sum")
INVALID, NODEVICE = -1, -2


def test_rotation_symbols_are_declared_bound_and_exported():
    from ppqsflhe_amd import Context, binding
    raw = open(os.path.join(ROOT, "include", "mkckks.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert sym in binding.SYMBOLS
        assert hasattr(binding.load_library(), sym)
    for m in METHODS:
        assert callable(getattr(Context, m, None)), m
    assert re.search(r"#define\s+MKCKKS_GALOIS_CONJ\b", hdr)
    # the declarations cite the upstream calls they stand for
    section = raw[raw.index("slot rotations and slot sums"):raw.index("mkckks_slot_sum_batch(")]
    assert "cc->EvalRotate" in section and "cc->EvalSum" in section and "never makes" in section


@pytest.fixture(scope="module")
def host_ctx():
    from ppqsflhe_amd import Context
    c = Context(12, 2, 40, 60, dnum=2, device=-1)
    yield c
    c.close()


@pytest.mark.parametrize("log_n", [9, 10, 12, 16, 17])
def test_galois_element_on_a_host_only_context(log_n):
    from ppqsflhe_amd import Context
    c = Context(log_n, 1, 40, 60, dnum=2, device=-1)
    try:
        N = c.N
        assert c.galois_element(0) == 1
        assert c.galois_element(1) == 5
        for r in (1, 2, 7, 100, N // 4 - 1, N // 4 - 7, N // 2 - 1):
            g, gi = c.galois_element(r), c.galois_element(-r)
            assert g == pow(5, r, 2 * N), r
            assert gi == pow(5, -r, 2 * N), r
            assert g * gi % (2 * N) == 1
            assert c.galois_element(r + N // 2) == g and c.galois_element(r - N // 2) == g
        assert c.galois_element(-2 ** 31) == 1 and c.galois_element(2 ** 31 - 1) == pow(5, -1, 2 * N)
        assert c.galois_conj == 2 * N - 1
        g = C.c_uint32()
        assert c._L.mkckks_galois_element(c._h, 1, None) == INVALID
        assert c._L.mkckks_galois_element(None, 1, C.byref(g)) == INVALID
    finally:
        c.close()


def test_rotation_refusals_on_a_host_only_context(host_ctx):
    """Pointers are never dereferenced: 8 stands for any input, `far` for an output away from it."""
    c = host_ctx
    auto, sec, kg, rot, ssum = (getattr(c._L, s) for s in SYMBOLS[1:])
    N, L, far = c.N, c.L, 1 << 40
    bad_g = (0, 2, 4, 2 * N, 2 * N + 1, 2 * N + 5, 0xFFFFFFFF)
    good_g = (1, 5, 2 * N - 1)
    # automorphism_batch(ctx, in, out, n_polys, nl, g)
    assert auto(c._h, None, far, 1, L, 5) == INVALID and auto(c._h, 8, None, 1, L, 5) == INVALID
    assert auto(None, 8, far, 1, L, 5) == INVALID
    for g in bad_g:
        assert auto(c._h, 8, far, 1, L, g) == INVALID, g
    for nl in (0, L + 1):
        assert auto(c._h, 8, far, 1, nl, 5) == INVALID, nl
    assert auto(c._h, 8, 8, 1, L, 5) == INVALID                           # in place
    assert auto(c._h, 8, 8 + 8 * N, 2, 1, 5) == INVALID                   # output starting inside the input
    assert auto(c._h, far + 8 * N, far, 2, 1, 5) == INVALID               # input starting inside the output
    assert auto(c._h, 8, far, 0, L, 5) == 0
    for g in good_g:
        assert auto(c._h, 8, far, 1, L, g) == NODEVICE, g
    assert auto(c._h, 8, 8 + 8 * N, 1, 1, 5) == NODEVICE                  # adjacent, not overlapping
    # automorphism_secret(ctx, s, out, g)
    assert sec(c._h, None, far, 5) == INVALID and sec(c._h, 8, None, 5) == INVALID
    for g in bad_g:
        assert sec(c._h, 8, far, g) == INVALID, g
    assert sec(c._h, 8, 8, 5) == INVALID and sec(c._h, 8, 8 + N - 1, 5) == INVALID
    assert sec(c._h, 8, 8 + N, 5) == NODEVICE
    # galois_keygen(ctx, s, pk, u, e0, e1, g, evk)
    for i in range(6):
        args = [8, 8, 8, 8, 8, 5, far]
        args[i if i < 5 else 6] = None
        assert kg(c._h, *args) == INVALID, i
    for g in bad_g:
        assert kg(c._h, 8, 8, 8, 8, 8, g, far) == INVALID, g
    assert kg(c._h, 8, 8, 8, 8, 8, 5, far) == NODEVICE
    # rotate_batch(ctx, ct, evk, out, n_ct, nl, g)
    for i in range(3):
        args = [8, 8, far]
        args[i] = None
        assert rot(c._h, *args, 1, L, 5) == INVALID, i
    for g in bad_g:
        assert rot(c._h, 8, 8, far, 1, L, g) == INVALID, g
    for nl in (0, L + 1):
        assert rot(c._h, 8, 8, far, 1, nl, 5) == INVALID, nl
    assert rot(c._h, 8, 8, 8, 1, L, 5) == INVALID
    assert rot(c._h, 8, 8, 8 + 8 * N, 1, L, 5) == INVALID
    assert rot(c._h, far + 8 * N, 8, far, 1, L, 5) == INVALID
    assert rot(c._h, 8, 8, far, 0, L, 5) == 0
    for nl in (1, L - 1, L):
        assert rot(c._h, 8, 8, far, 1, nl, 5) == NODEVICE, nl
    # slot_sum_batch(ctx, ct, evks, out, n_ct, nl, span)
    for i in range(3):
        args = [8, 8, far]
        args[i] = None
        assert ssum(c._h, *args, 1, L, 2) == INVALID, i
    for span in (0, 3, 6, N // 2 + 1, N, 2 * N, 0xFFFFFFFF, 0x80000000):
        assert ssum(c._h, 8, 8, far, 1, L, span) == INVALID, span
    for nl in (0, L + 1):
        assert ssum(c._h, 8, 8, far, 1, nl, 2) == INVALID, nl
    assert ssum(c._h, 8, 8, 8, 1, L, 2) == INVALID
    assert ssum(c._h, 8, 8, 8 + 8 * N, 1, L, 1) == INVALID
    assert ssum(c._h, 8, 8, far, 0, L, 2) == 0
    for span in (1, 2, N // 2):
        assert ssum(c._h, 8, 8, far, 1, L, span) == NODEVICE, span
    assert ssum(c._h, 8, None, far, 1, L, 1) == NODEVICE                   # span 1 reads no key


def test_rotation_methods_raise_on_a_host_only_context(host_ctx):
    from ppqsflhe_amd.binding import MkckksError
    c = host_ctx
    far = 1 << 40
    calls = [lambda: c.automorphism(8, far, 1, c.L, 5), lambda: c.automorphism_secret(8, far, 5),
             lambda: c.galois_keygen(8, 8, 8, 8, 8, 5, far), lambda: c.rotate(8, 8, far, 1, c.L, 5),
             lambda: c.slot_sum(8, 8, far, 1, c.L, 4)]
    for i, call in enumerate(calls):
        with pytest.raises(MkckksError) as ei:
            call()
        assert ei.value.code == NODEVICE, i
    with pytest.raises(MkckksError) as ei:
        c.rotate(8, 8, far, 1, c.L, 4)
    assert ei.value.code == INVALID and "Galois element" in str(ei.value)
    with pytest.raises(MkckksError) as ei:
        c.slot_sum(8, 8, far, 1, c.L, 3)
    assert ei.value.code == INVALID and "span" in str(ei.value)


def test_rotation_hosts_usage_and_exit_codes_without_a_device(tmp_path):
    """Everything rotKeyGen and slotSum decide before they open a device: exit 1 with the program's message, nothing
    written."""
    from tests.test_cli_hosts import BIN, _small_cc, run
    for prog in ("rotKeyGen", "slotSum"):
        assert os.access(os.path.join(BIN, prog), os.X_OK), f"{prog} not built (make -C ppqsflhe_amd/host)"
    cc = _small_cc(tmp_path)
    out = tmp_path / "out"
    rot_usage = "<cc.json> <privkey> <pubkey> <rotkeys_out> (--steps r1,r2,... | --sum <span>)"
    sum_usage = "<cc_path> <rotkeys> <input_encfile> <output_encfile> [--span <n>] [--slot-weights <factors.json>]"
    cases = [
        ("rotKeyGen", (), rot_usage),
        ("rotKeyGen", (cc, "sk", "pk", out), rot_usage),
        ("rotKeyGen", (cc, "sk", "pk", out, "--steps"), rot_usage),
        ("rotKeyGen", (cc, "sk", "pk", out, "--rot", "1"), rot_usage),
        ("rotKeyGen", (cc, "sk", "pk", out, "--steps", "1", "--sum", "2"), rot_usage),
        ("rotKeyGen", (cc, "sk", "pk", out, "--steps", "1,,2"), "[rotkeygen] ERROR: --steps needs a comma-separated list of integers"),
        ("rotKeyGen", (cc, "sk", "pk", out, "--steps", "1,x"), "[rotkeygen] ERROR: --steps needs a comma-separated list of integers"),
        ("rotKeyGen", (cc, "sk", "pk", out, "--steps", "1,"), "[rotkeygen] ERROR: --steps needs a comma-separated list of integers"),
        ("rotKeyGen", (cc, "sk", "pk", out, "--steps", "12345678901"), "[rotkeygen] ERROR: --steps needs a comma-separated list of integers"),
        ("rotKeyGen", (cc, "sk", "pk", out, "--sum", "6"), "[rotkeygen] ERROR: --sum needs a power of two of at least 1"),
        ("rotKeyGen", (cc, "sk", "pk", out, "--sum", "0"), "[rotkeygen] ERROR: --sum needs a power of two of at least 1"),
        ("rotKeyGen", (cc, "sk", "pk", out, "--sum", "-4"), "[rotkeygen] ERROR: --sum needs a power of two of at least 1"),
        ("rotKeyGen", (tmp_path / "nocc", "sk", "pk", out, "--sum", "4"), "[rotkeygen] ERROR: Failed to load CryptoContext from"),
        ("slotSum", (), sum_usage),
        ("slotSum", (cc, "keys", "in"), sum_usage),
        ("slotSum", (cc, "keys", "in", out, "--span"), sum_usage),
        ("slotSum", (cc, "keys", "in", out, "--span", "4", "--span", "8"), sum_usage),
        ("slotSum", (cc, "keys", "in", out, "--steps", "4"), sum_usage),
        ("slotSum", (cc, "keys", "in", out, "--slot-weights", ""), sum_usage),
        ("slotSum", (cc, "keys", "in", out, "--span", "3"), "[slotsum] ERROR: --span needs a power of two of at least 1"),
        ("slotSum", (cc, "keys", "in", out, "--span", "0"), "[slotsum] ERROR: --span needs a power of two of at least 1"),
        ("slotSum", (cc, "keys", "in", out, "--span", "x"), "[slotsum] ERROR: --span needs a power of two of at least 1"),
        ("slotSum", (cc, "keys", "in", out, "--slot-weights", tmp_path / "nofile.json"), "[slotsum] ERROR: "),
        ("slotSum", (tmp_path / "nocc", "keys", "in", out), "[slotsum] ERROR: Failed to load CryptoContext from"),
    ]
    for prog, args, msg in cases:
        r = run(prog, *args)
        assert r.returncode == 1 and msg in r.stderr, (prog, args, r.stdout + r.stderr)
        assert not os.path.exists(out), (prog, args)


def test_galois_index_arithmetic_under_sanitizers():
    r = subprocess.run(["make", "-C", CSRC, "-s", "../galois_selftest_asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(ROOT, "ppqsflhe_amd", "galois_selftest_asan")], capture_output=True, text=True, env=ENV,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "galois selftest ok" in r.stdout and "FAIL" not in r.stdout, r.stdout
