"""Collective evaluation keys, the part that needs no GPU (include/mkckks.h: "collective evaluation keys"): the two
symbols are declared, bound and exported; every refusal of the calls, decided before a device is asked for, with the text
mkckks_last_error keeps; the container kinds and matching rules of the hosts (evalkeys.hpp) as a stand-alone program,
plain and under -fsanitize=address,undefined; the hosts' usage lines and what they refuse before they open a device."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests.test_cli_hosts import BIN, _small_cc, run, write_key_container

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppqsflhe_amd", "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
SYMBOLS = ("mkckks_evk_sum", "mkckks_relin_share")
METHODS = ("evk_sum", "relin_share")
INVALID, NODEVICE = -1, -2
MAX_PARTIES = 64


def test_symbols_are_declared_bound_and_exported_and_the_header_states_the_rules():
    from ppqsflhe_amd import Context, binding
    raw = open(os.path.join(ROOT, "include", "mkckks.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert sym in binding.SYMBOLS
        assert hasattr(binding.load_library(), sym)
    for m in METHODS:
        assert callable(getattr(Context, m, None)), m
    assert "#define MKCKKS_MAX_PARTIES %d" % MAX_PARTIES in raw
    section = raw[raw.index("collective evaluation keys of a JOINT key"):raw.index("int mkckks_relin_share(")]
    for text in ("MultiEvalAtIndexKeyGen", "MultiEvalSumKeyGen", "MultiAddEvalAutomorphismKeys", "MultiKeySwitchGen", "MultiAddEvalKeys",
                 "MultiMultEvalKey", "MultiAddEvalMultKeys", "never makes", "sqrt(N * 2n/3)", "no secret under RLWE",
                 "FEWER than all n", "FRESH errors", "ALL n parties", "play no role", "16-byte aligned", "ALL D limbs"):
        assert text in section, text
    # the sentences that said a joint key's keys cannot be made are gone
    assert "which this library does not have" not in re.sub(r"\s+\*?\s*", " ", raw)
    for name in ("include/mkckks.h", "DESIGN.md", "ppqsflhe_amd/host/relinKeyGen.cpp", "ppqsflhe_amd/host/rotKeyGen.cpp"):
        text = re.sub(r"\s+(//|\*)?\s*", " ", open(os.path.join(ROOT, name)).read())
        assert "needs a collective protocol" not in text and "need a collective protocol" not in text, name


@pytest.fixture(scope="module")
def host_ctx():
    from ppqsflhe_amd import Context
    c = Context(12, 2, 40, 60, dnum=2, device=-1)
    yield c
    c.close()


def last_error(c):
    return c._L.mkckks_last_error().decode()


def refused(c, code, text):
    assert code == INVALID, code
    assert text in last_error(c), (text, last_error(c))
    return True


def test_refusals_on_a_host_only_context(host_ctx):
    """Pointers are never dereferenced: A stands for the shares or the round-1 key, `far` for an output away from them."""
    c = host_ctx
    es, rs = (getattr(c._L, s) for s in SYMBOLS)
    N, D, beta = c.N, c.D, c.beta
    key = 8 * beta * 2 * D * N  # bytes of one key
    A, S, E0, E1, far = 1 << 30, 1 << 20, 1 << 24, 1 << 26, 1 << 40
    # evk_sum(ctx, in, out, n_parties, n_keys)
    for i in range(2):
        args = [A, far]
        args[i] = None
        assert refused(c, es(c._h, *args, 3, 1), "null argument"), i
    assert es(None, A, far, 3, 1) == INVALID
    for n in (0, MAX_PARTIES + 1, 0xFFFFFFFF):
        assert refused(c, es(c._h, A, far, n, 1), "1 <= n_parties <= MKCKKS_MAX_PARTIES"), n
        assert refused(c, es(c._h, A, far, n, 0), "1 <= n_parties <= MKCKKS_MAX_PARTIES"), n
    assert refused(c, es(c._h, A + 8, far, 3, 1), "16-byte aligned")
    assert refused(c, es(c._h, A, far + 8, 3, 1), "16-byte aligned")
    assert refused(c, es(c._h, A, A + 16, 3, 1), "output overlaps the shares")               # cuts the first share
    assert refused(c, es(c._h, A, A + key, 3, 1), "output overlaps the shares")              # the second share
    assert refused(c, es(c._h, A, A + 3 * 2 * key - 16, 3, 2), "output overlaps the shares")  # the last words
    assert refused(c, es(c._h, A + key, A, 3, 2), "output overlaps the shares")              # shares start inside the output
    assert refused(c, es(c._h, A, far, MAX_PARTIES, 0xFFFFFFFF), "output overlaps the shares")  # spans everything
    assert es(c._h, A, far, 3, 0) == 0 and es(c._h, A, A, 1, 0) == 0                          # no keys: a no-op
    for args in ((A, far, 3, 1), (A, A, 3, 1), (A, A, 1, 1), (A, A + 3 * key, 3, 1), (A, far, MAX_PARTIES, 15)):
        assert es(c._h, *args) == NODEVICE, args
    # relin_share(ctx, key1, sk, e0, e1, share)
    for i in range(5):
        args = [A, S, E0, E1, far]
        args[i] = None
        assert refused(c, rs(c._h, *args), "null argument"), i
    assert rs(None, A, S, E0, E1, far) == INVALID
    for args in ((A + 8, S, E0, E1, far), (A, S + 8, E0, E1, far), (A, S, E0, E1, far + 8)):
        assert refused(c, rs(c._h, *args), "16-byte aligned"), args
    assert refused(c, rs(c._h, A, S, E0, E1, A + 16), "share partially overlaps the round-1 key")
    assert refused(c, rs(c._h, A, S, E0, E1, A + key - 16), "share partially overlaps the round-1 key")
    assert refused(c, rs(c._h, A + 16, S, E0, E1, A), "share partially overlaps the round-1 key")
    assert refused(c, rs(c._h, A, S, E0, E1, S), "share overlaps an input")                   # onto the secret
    assert refused(c, rs(c._h, A, far + key - 16, E0, E1, far), "share overlaps an input")    # the secret starts inside it
    assert refused(c, rs(c._h, A, S, far + 16, E1, far), "share overlaps an input")
    assert refused(c, rs(c._h, A, S, E0, far + key - 4, far), "share overlaps an input")
    for args in ((A, S, E0, E1, far), (A, S, E0, E1, A), (A, S, E0, E0, A), (A, S, E0 + 4, E1 + 4, far), (A, S, E0, E1, A + key)):
        assert rs(c._h, *args) == NODEVICE, args


def test_methods_raise_on_a_host_only_context(host_ctx):
    from ppqsflhe_amd.binding import MkckksError
    c = host_ctx
    A, S, E0, E1, far = 1 << 30, 1 << 20, 1 << 24, 1 << 26, 1 << 40
    for i, call in enumerate((lambda: c.evk_sum(A, far, 3, 1), lambda: c.relin_share(A, S, E0, E1, A))):
        with pytest.raises(MkckksError) as ei:
            call()
        assert ei.value.code == NODEVICE, i
    with pytest.raises(MkckksError) as ei:
        c.evk_sum(A, far, 65, 1)
    assert ei.value.code == INVALID and "n_parties" in str(ei.value)
    with pytest.raises(MkckksError) as ei:
        c.relin_share(A, S, E0, E1, A + 16)
    assert ei.value.code == INVALID and "overlaps" in str(ei.value)


def test_kinds_and_matching_rules_plain_and_under_sanitizers():
    for target, exe in (("build/evalkeys_selftest", ("build", "evalkeys_selftest")),
                        ("build/asan/evalkeys_selftest", ("build", "asan", "evalkeys_selftest"))):
        r = subprocess.run(["make", "-C", HOST, "-s", target], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        r = subprocess.run([os.path.join(HOST, *exe)], capture_output=True, text=True, env=ENV, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
        assert "evalkeys selftest ok" in r.stdout and "FAIL" not in r.stdout, r.stdout


USAGE = {"fuseEvalKeys": "<cc.json> <out> <share_1> ... <share_n>",
         "relinKeyGen": "<cc.json> <privkey> <key1> <share_out> --share",
         "rotKeyGen": "<cc.json> <privkey> <pubkey> <rotkeys_out> (--steps r1,r2,... | --sum <span>)"}


def test_hosts_are_built_and_state_their_usage():
    for prog, usage in USAGE.items():
        assert os.access(os.path.join(BIN, prog), os.X_OK), f"{prog} not built (make -C ppqsflhe_amd/host)"
        for args in ((), ("a",), ("a", "b")):
            r = run(prog, *args)
            assert r.returncode == 1 and "Usage:" in r.stderr and usage in r.stderr, (prog, args, r.stderr)
    # a trailing word that is not --share, and words after it
    for prog, args in (("relinKeyGen", ("a", "b", "c", "d", "--shares")), ("relinKeyGen", ("a", "b", "c", "d", "--share", "x")),
                       ("rotKeyGen", ("a", "b", "c", "d", "--sum", "4", "share")), ("rotKeyGen", ("a", "b", "c", "d", "--sum", "4", "--share", "x"))):
        r = run(prog, *args)
        assert r.returncode == 1 and "Usage:" in r.stderr, (prog, args, r.stderr)
    # --share changes no refusal of rotKeyGen's own arguments
    r = run("rotKeyGen", "a", "b", "c", "d", "--sum", "6", "--share")
    assert r.returncode == 1 and "[rotkeygen] ERROR: --sum needs a power of two of at least 1" in r.stderr
    r = run("rotKeyGen", "nocc", "b", "c", "d", "--sum", "4", "--share")
    assert r.returncode == 1 and "[rotkeygen] ERROR: Failed to load CryptoContext from nocc" in r.stderr


def rot_container(path, kind, ring_dim, limbs, parts, elements):
    """The rotation-key layout (rotkeys.hpp): header with slots = entries, then (g, key) per entry; zero keys."""
    hdr = struct.pack("<4sIIIIIIIdII", b"MKCK", 1, kind, ring_dim, limbs, parts, 0, 0, 0.0, len(elements), 0)
    with open(path, "wb") as f:
        f.write(hdr)
        for g in elements:
            f.write(struct.pack("<Q", g))
            f.write(bytes(8 * ring_dim * limbs * parts))


def test_refusals_decided_before_a_device_is_opened(tmp_path):
    cc = _small_cc(tmp_path)
    out = tmp_path / "out.key"
    n, D, parts = 16, 2, 4
    zeros = np.zeros(n * D * parts, dtype=np.uint64)
    mk = lambda name, kind, ring=n, limbs=D, pp=parts: (write_key_container(tmp_path / name, kind, ring, limbs, pp,
                                                                            np.zeros(ring * limbs * pp, dtype=np.uint64)), tmp_path / name)[1]
    rk, rk2, sh = mk("rk", 4), mk("rk2", 4), mk("sh", 12)

    def refused(prog, args, msg):
        r = run(prog, *args)
        assert r.returncode == 1 and msg in r.stderr, (args, r.stdout + r.stderr)
        assert not os.path.exists(out), args

    refused("fuseEvalKeys", (tmp_path / "nocc", out, rk, rk2), "[fuseevalkeys] ERROR: Failed to load CryptoContext from")
    refused("fuseEvalKeys", (cc, out, rk, tmp_path / "absent"), f"[fuseevalkeys] ERROR: Failed to load a key share from {tmp_path / 'absent'}")
    (tmp_path / "junk").write_text("not a key container, but longer than one header: " + "x" * 64)
    refused("fuseEvalKeys", (cc, out, tmp_path / "junk", rk), f"Failed to load a key share from {tmp_path / 'junk'}")
    # mixed kinds, by file and by name
    refused("fuseEvalKeys", (cc, out, rk, sh), f"{sh}: kind differs from {rk} (a relinearisation-key share beside a re-encryption key)")
    refused("fuseEvalKeys", (cc, out, sh, rk2, sh), f"{rk2}: kind differs from {sh}")
    # finished keys and foreign containers are no shares
    refused("fuseEvalKeys", (cc, out, mk("fin10", 10), sh), f"{tmp_path / 'fin10'} is a relinearisation key, a finished key, not a share")
    rot_container(tmp_path / "fin9", 9, n, D, parts, [5])
    refused("fuseEvalKeys", (cc, out, sh, tmp_path / "fin9"), f"{tmp_path / 'fin9'} is a rotation-key file, a finished key, not a share")
    refused("fuseEvalKeys", (cc, out, mk("pk", 2), rk), "is a public key, not a share of an evaluation key")
    refused("fuseEvalKeys", (cc, out, rk, mk("sk", 3)), "is a secret key, not a share of an evaluation key")
    # differing N / D / beta, by field
    refused("fuseEvalKeys", (cc, out, sh, mk("sh_n", 12, ring=32)), f"{tmp_path / 'sh_n'}: ring dimension N differs from {sh} (32 beside 16)")
    refused("fuseEvalKeys", (cc, out, sh, mk("sh_d", 12, limbs=3)), f"{tmp_path / 'sh_d'}: limb count D differs from {sh} (3 beside 2)")
    refused("fuseEvalKeys", (cc, out, sh, mk("sh_b", 12, pp=6)), f"{tmp_path / 'sh_b'}: digit count beta differs from {sh} (3 beside 2)")
    # a payload that is not what the header says
    with open(tmp_path / "short", "wb") as f:
        f.write(open(sh, "rb").read()[:-8])
    refused("fuseEvalKeys", (cc, out, sh, tmp_path / "short"), f"{tmp_path / 'short'}: size does not match its header")
    # rotation-key shares: the sets of Galois elements
    for name, el in (("ra", [5, 25, 31]), ("rb", [31, 5, 25]), ("rc", [5, 25]), ("rd", [5, 25, 29]), ("re", [5, 25, 25]), ("rf", [5, 6, 25])):
        rot_container(tmp_path / name, 11, n, D, parts, el)
    ra, rb, rc, rd = (tmp_path / x for x in ("ra", "rb", "rc", "rd"))
    refused("fuseEvalKeys", (cc, out, ra, rb, rc), f"{rc}: Galois element 31 of {ra} is missing")
    refused("fuseEvalKeys", (cc, out, rc, ra), f"{ra}: Galois element 31 is not in {rc}")
    refused("fuseEvalKeys", (cc, out, ra, rd), f"{rd}: Galois element 31 of {ra} is missing")
    refused("fuseEvalKeys", (cc, out, ra, tmp_path / "re"), f"{tmp_path / 're'}: holds Galois element 25 twice")
    refused("fuseEvalKeys", (cc, out, tmp_path / "rf", ra), f"{tmp_path / 'rf'}: holds the invalid Galois element 6")
    refused("fuseEvalKeys", (cc, out, ra, sh), f"{sh}: kind differs from {ra} (a relinearisation-key share beside a rotation-key share)")
    # more shares than parties
    refused("fuseEvalKeys", (cc, out, *([sh] * (MAX_PARTIES + 1))), "65 shares (at most 64 parties)")
    # relinKeyGen --share: the round-1 key by kind
    refused("relinKeyGen", (tmp_path / "nocc", "sk", rk, out, "--share"), "[relinkeygen] ERROR: Failed to load CryptoContext from")
    refused("relinKeyGen", (cc, "sk", tmp_path / "absent", out, "--share"), "[relinkeygen] ERROR: Failed to load the round-1 key from")
    refused("relinKeyGen", (cc, "sk", sh, out, "--share"), f"{sh} is a relinearisation-key share, not the round-1 key")
    refused("relinKeyGen", (cc, "sk", tmp_path / "fin10", out, "--share"), "is a relinearisation key, not the round-1 key")
    # cipherProduct: a share offered as the key is refused by name
    refused("cipherProduct", (cc, sh, "a", "b", out), f"{sh} is a relinearisation-key share, not a relinearisation key")
    refused("cipherProduct", (cc, ra, "a", "b", out), f"{ra} is a rotation-key share, not a relinearisation key")
