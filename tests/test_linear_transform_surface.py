"""Linear transforms, the part that needs no GPU (include/mkckks.h: "linear transforms by diagonals, double hoisted"): the
symbols are declared, bound and exported; every refusal of the compute calls, decided before a device is asked for; the
usage and exit codes of linearTransform without a device; the --block diagonals against a dense numpy product (the
construction restated here and the host's, through the stand-alone program); lintrans_selftest under
-fsanitize=address,undefined (the diagonals reader and the --block builder of ppqsflhe_amd/host/lintrans.hpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppqsflhe_amd", "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
SYMBOLS = ("mkckks_encode_ext_batch", "mkckks_linear_transform_batch")
METHODS = ("encode_ext", "linear_transform")
INVALID, NODEVICE = -1, -2


def test_linear_transform_symbols_are_declared_bound_and_exported():
    from ppqsflhe_amd import Context, binding
    raw = open(os.path.join(ROOT, "include", "mkckks.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert sym in binding.SYMBOLS
        assert hasattr(binding.load_library(), sym)
    for m in METHODS:
        assert callable(getattr(Context, m, None)), m
    # the declarations cite the upstream calls they stand for and state the headroom rule
    section = raw[raw.index("linear transforms by diagonals, double hoisted"):raw.index("mkckks_linear_transform_batch(")]
    for word in ("EvalLinearTransform", "EvalFastRotation", "never makes", "MakeCKKSPackedPlaintext", "Headroom"):
        assert word in section, word


@pytest.fixture(scope="module")
def host_ctx():
    from ppqsflhe_amd import Context
    c = Context(12, 2, 40, 60, dnum=2, device=-1)
    yield c
    c.close()


def gs(*vals):
    return (C.c_uint32 * len(vals))(*vals)


def test_linear_transform_refusals_on_a_host_only_context(host_ctx):
    """Device pointers are never dereferenced: 16 stands for any input, `far` for an output away from it.  h_g is a host
    array and is read."""
    c = host_ctx
    enc, lt = (getattr(c._L, s) for s in SYMBOLS)
    N, L, far = c.N, c.L, 1 << 40
    # encode_ext_batch(ctx, vals, pt, n, nl, scale)
    assert enc(c._h, None, far, 1, L, 2.0 ** 40) == INVALID and enc(c._h, 16, None, 1, L, 2.0 ** 40) == INVALID
    assert enc(None, 16, far, 1, L, 2.0 ** 40) == INVALID
    assert enc(c._h, 16, far, 1, L, 0.0) == INVALID and enc(c._h, 16, far, 1, L, -1.0) == INVALID
    for nl in (0, L + 1):
        assert enc(c._h, 16, far, 1, nl, 2.0 ** 40) == INVALID, nl
    assert enc(c._h, 16, far, 1, L, 2.0 ** 40) == NODEVICE
    # linear_transform_batch(ctx, ct, evks, pts, h_g, out, n_rot, n_ct, nl)
    good = gs(5, 1, 2 * N - 1)
    base = [16, 1 << 30, 1 << 35, good, far]
    for i in (0, 2, 3, 4):
        args = list(base)
        args[i] = None
        assert lt(c._h, *args, 3, 1, L) == INVALID, i
    assert lt(None, *base, 3, 1, L) == INVALID
    assert lt(c._h, 16, None, 1 << 35, good, far, 3, 1, L) == INVALID       # a keyed element and no keys
    assert lt(c._h, 16, None, 1 << 35, gs(1, 1), far, 2, 1, L) == NODEVICE  # unrotated terms alone read no key
    for nl in (0, L + 1):
        assert lt(c._h, *base, 3, 1, nl) == INVALID, nl
    for bad in (0, 2, 4, 2 * N, 2 * N + 1, 0xFFFFFFFF):
        assert lt(c._h, 16, 1 << 30, 1 << 35, gs(5, bad, 1), far, 3, 1, L) == INVALID, bad
        assert lt(c._h, 16, 1 << 30, 1 << 35, gs(5, 1, bad), far, 2, 1, L) == NODEVICE, bad  # past n_rot: not read
    ct_bytes = 2 * L * N * 8
    assert lt(c._h, 16, 1 << 30, 1 << 35, good, 16, 3, 1, L) == INVALID                  # in place
    assert lt(c._h, 16, 1 << 30, 1 << 35, good, 16 + ct_bytes, 3, 2, L) == INVALID       # output starting inside the input
    assert lt(c._h, far + ct_bytes, 1 << 30, 1 << 35, good, far, 3, 2, L) == INVALID     # input starting inside the output
    assert lt(c._h, 16, 1 << 30, far + 16, good, far, 3, 1, L) == INVALID                # output over the plaintexts
    assert lt(c._h, 16, far - 16, 1 << 35, good, far, 3, 1, L) == INVALID                # output over the keys
    assert lt(c._h, 16, 1 << 30, 1 << 35, good, 16 + ct_bytes, 3, 1, L) == NODEVICE      # adjacent, not overlapping
    for i in (0, 1, 2, 4):                                                                # 16-byte alignment
        args = list(base)
        args[i] += 8
        assert lt(c._h, *args, 3, 1, L) == INVALID, i
    assert lt(c._h, *base, 0, 1, L) == 0 and lt(c._h, *base, 3, 0, L) == 0                # no-ops
    for nl in (1, L - 1, L):
        assert lt(c._h, *base, 3, 1, nl) == NODEVICE, nl
    assert lt(c._h, 16, 1 << 30, 1 << 35, gs(5, 5, 1, 1), far, 4, 1, L) == NODEVICE      # duplicates are allowed


def test_more_than_six_digits_are_refused():
    from ppqsflhe_amd import Context
    c = Context(10, 6, 50, 60, dnum=8, device=-1)
    try:
        assert c.beta == 8
        lt = c._L.mkckks_linear_transform_batch
        assert lt(c._h, 16, 1 << 30, 1 << 35, gs(5), 1 << 40, 1, 1, c.L) == INVALID
        assert "more than 6 key-switch digits" in c._L.mkckks_last_error().decode()
        assert lt(c._h, 16, 1 << 30, 1 << 35, gs(5), 1 << 40, 1, 1, 6 * c.alpha) == NODEVICE
    finally:
        c.close()


def test_linear_transform_methods_raise_on_a_host_only_context(host_ctx):
    from ppqsflhe_amd.binding import MkckksError
    c = host_ctx
    far = 1 << 40
    for i, call in enumerate([lambda: c.encode_ext(16, far, 1, c.L, 2.0 ** 40),
                              lambda: c.linear_transform(16, 1 << 30, 1 << 35, [5, 1], far, 1, c.L)]):
        with pytest.raises(MkckksError) as ei:
            call()
        assert ei.value.code == NODEVICE, i
    with pytest.raises(MkckksError) as ei:
        c.linear_transform(16, 1 << 30, 1 << 35, [5, 4], far, 1, c.L)
    assert ei.value.code == INVALID and "Galois element" in str(ei.value)
    c.linear_transform(16, 1 << 30, 1 << 35, [], far, 1, c.L)  # no diagonals: a no-op


def test_linear_transform_host_usage_and_exit_codes_without_a_device(tmp_path):
    """Everything linearTransform decides before it opens a device: exit 1 with the program's message, nothing written."""
    import json
    from tests.test_cli_hosts import BIN, _small_cc, run
    assert os.access(os.path.join(BIN, "linearTransform"), os.X_OK), "linearTransform not built (make -C ppqsflhe_amd/host)"
    cc = _small_cc(tmp_path)
    out = tmp_path / "out"

    def doc(name, obj):
        p = tmp_path / name
        p.write_text(obj if isinstance(obj, str) else json.dumps(obj))
        return p

    usage = "<cc_path> <rotkeys> (<diagonals.json> | --block <matrix.json>) <input_encfile> <output_encfile>"
    good = doc("good.json", {"diagonals": [{"step": 0, "values": [1.0]}]})
    cases = [
        ((), usage),
        ((cc, "keys", good, "in"), usage),
        ((cc, "keys", good, "in", out, "extra", "more"), usage),
        ((cc, "keys", "--blocks", good, "in", out), usage),
        ((cc, "keys", good, "--block", "in", out), usage),
        ((cc, "keys", "--block", "in", out), usage),
        ((cc, "keys", "", "in", out), usage),
        ((tmp_path / "nocc", "keys", good, "in", out), "[lintrans] ERROR: Failed to load CryptoContext from"),
        ((cc, "keys", tmp_path / "nofile.json", "in", out), "[lintrans] ERROR: diagonals: could not read"),
        ((cc, "keys", "--block", tmp_path / "nofile.json", "in", out), "[lintrans] ERROR: --block: could not read"),
        ((cc, "keys", doc("e.json", {"diagonals": []}), "in", out), "[lintrans] ERROR: diagonals: not a non-empty array"),
        ((cc, "keys", doc("s.json", {"diagonals": [{"step": 0.5, "values": [1]}]}), "in", out), "[lintrans] ERROR: diagonals: not a list"),
        ((cc, "keys", doc("l.json", {"diagonals": [{"step": 1, "values": [0.0] * 8193}]}), "in", out), "has 8193 values, the ring has 8192 slots"),
        ((cc, "keys", doc("n.json", '{"diagonals": [{"step": 1, "values": [1e999]}]}'), "in", out), "[lintrans] ERROR: diagonals"),
        ((cc, "keys", "--block", doc("m3.json", {"matrix": [[1, 2, 3]] * 3}), "in", out), "[lintrans] ERROR: --block: the matrix has 3 rows"),
        ((cc, "keys", "--block", doc("mr.json", {"matrix": [[1, 2], [3]]}), "in", out), "[lintrans] ERROR: --block: row 1 does not have 2 entries"),
        ((cc, "keys", "--block", good, "in", out), "[lintrans] ERROR: --block: not a matrix"),
    ]
    for args, msg in cases:
        r = run("linearTransform", *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stdout + r.stderr)
        assert not os.path.exists(out), args


def block_diagonals(Mx, slots):
    """The --block construction: {step: diagonal}, diag_r[j] = M[j mod n][(j mod n) + r] where that column exists."""
    n = Mx.shape[0]
    j = np.arange(slots)
    out = {}
    for r in range(-(n - 1), n):
        col = j % n + r
        ok = (col >= 0) & (col < n)
        out[r] = np.where(ok, Mx[j % n, np.clip(col, 0, n - 1)], 0.0)
    return out


@pytest.mark.parametrize("n,slots", [(1, 8), (2, 8), (4, 32), (8, 8), (16, 64)])
def test_block_diagonals_apply_the_matrix_to_every_block(n, slots):
    """out[j] = sum_r diag_r[j] in[(j + r) mod slots] with the 2n - 1 masked diagonals is the dense product of every aligned
    n-slot block with M: no diagonal reaches across a block, the last block included (no wrap-around)."""
    rng = np.random.default_rng(n)
    Mx, x = rng.integers(-8, 9, (n, n)).astype(float), rng.integers(-8, 9, slots).astype(float)
    diags = block_diagonals(Mx, slots)
    assert sorted(diags) == list(range(-(n - 1), n))
    got = sum(d * np.roll(x, -r) for r, d in diags.items())
    assert np.array_equal(got, (x.reshape(-1, n) @ Mx.T).reshape(-1))


def test_diagonal_reader_and_block_builder_under_sanitizers():
    """The host's own builder does the same (lintrans_selftest compares it with a dense product at n = 1, 2, 4, 8 and on 64
    slots), plain and under ASan + UBSan."""
    r = subprocess.run(["make", "-C", HOST, "-s", "build/lintrans_selftest", "lintrans-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for exe in ("build/lintrans_selftest", "build/asan/lintrans_selftest"):
        r = subprocess.run([os.path.join(HOST, exe)], capture_output=True, text=True, env=ENV, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        assert "lintrans selftest ok" in r.stdout and "FAIL" not in r.stdout, r.stdout
