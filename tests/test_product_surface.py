"""Ciphertext products, the part that needs no GPU (include/mkckks.h: "ciphertext products"): the four symbols are
declared, bound and exported; every refusal of the calls, decided before a device is asked for, with the text
mkckks_last_error keeps; zero counts; the hosts' header bookkeeping (product.hpp) as a stand-alone program under
-fsanitize=address,undefined."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppqsflhe_amd", "host")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
SYMBOLS = ("mkckks_relin_keygen", "mkckks_tensor_sum_batch", "mkckks_relinearize_batch", "mkckks_mult_relin_batch")
METHODS = ("relin_keygen", "tensor_sum", "relinearize", "mult_relin")
INVALID, NODEVICE = -1, -2


def test_product_symbols_are_declared_bound_and_exported():
    from ppqsflhe_amd import Context, binding
    raw = open(os.path.join(ROOT, "include", "mkckks.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for sym in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert sym in binding.SYMBOLS
        assert hasattr(binding.load_library(), sym)
    for m in METHODS:
        assert callable(getattr(Context, m, None)), m
    # the declarations cite the upstream calls they stand for and state the scale, headroom, noise and alignment rules
    section = raw[raw.index("ciphertext products: cc->EvalMultKeyGen"):raw.index("mkckks_mult_relin_batch(")]
    for text in ("cc->EvalMultKeyGen", "cc->EvalMult(ct, ct)", "cc->Relinearize", "cc->EvalInnerProduct(ct, ct)", "never makes",
                 "S_a * S_b", "noiseScaleDeg", "mkckks_rescale_batch", "cannot check", "one re-encryption", "16-byte aligned",
                 "JOINT key"):
        assert text in section, text


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


def test_product_refusals_on_a_host_only_context(host_ctx):
    """Pointers are never dereferenced: A and B stand for any inputs, `far` for an output away from them."""
    c = host_ctx
    kg, ts, rl, mr = (getattr(c._L, s) for s in SYMBOLS)
    N, L = c.N, c.L
    A, B, K, far = 1 << 20, 1 << 30, 1 << 36, 1 << 40
    ct = lambda n, nl, comps=2: 8 * n * comps * nl * N  # bytes of n ciphertexts
    # relin_keygen(ctx, s, pk, u, e0, e1, evk)
    for i in range(6):
        args = [8, 8, 8, 8, 8, far]
        args[i] = None
        assert refused(c, kg(c._h, *args), "null argument"), i
    assert kg(None, 8, 8, 8, 8, 8, far) == INVALID
    assert kg(c._h, 8, 8, 8, 8, 8, far) == NODEVICE
    # tensor_sum_batch(ctx, a, b, out3, n_terms, n_ct, nl)
    for i in range(3):
        args = [A, B, far]
        args[i] = None
        assert refused(c, ts(c._h, *args, 1, 1, L), "null argument"), i
    assert ts(None, A, B, far, 1, 1, L) == INVALID
    for nl in (0, L + 1, 0xFFFFFFFF):
        assert refused(c, ts(c._h, A, B, far, 1, 1, nl), "nl out of range"), nl
    assert refused(c, ts(c._h, A, B, far, 0, 1, L), "n_terms must be at least 1")
    assert refused(c, ts(c._h, A, B, far, 0, 0, L), "n_terms must be at least 1")
    for args in ((A + 8, B, far), (A, B + 8, far), (A, B, far + 8)):
        assert refused(c, ts(c._h, *args, 1, 1, L), "16-byte aligned"), args
    assert refused(c, ts(c._h, A, B, A, 1, 1, L), "output overlaps input")                          # out3 is a
    assert refused(c, ts(c._h, A, B, B, 1, 1, L), "output overlaps input")                          # out3 is b
    assert refused(c, ts(c._h, A, B, A + ct(2, L) - 16, 1, 2, L), "output overlaps input")          # starts inside a
    assert refused(c, ts(c._h, A, B, A + ct(3, 1) * 2 - 16, 3, 2, 1), "output overlaps input")      # inside a's last term
    assert refused(c, ts(c._h, A, far + ct(1, L, 3) - 16, far, 1, 1, L), "output overlaps input")   # b starts inside out3
    assert refused(c, ts(c._h, A, B, far, 0xFFFFFFFF, 0xFFFFFFFF, L), "output overlaps input")      # spans everything
    assert ts(c._h, A, B, far, 1, 0, L) == 0 and ts(c._h, A, B, far, 7, 0, 1) == 0                  # zero count: a no-op
    assert ts(c._h, A, B, A + ct(2, L), 1, 2, L) == NODEVICE                                        # adjacent to a
    assert ts(c._h, A, A, far, 1, 1, L) == NODEVICE                                                 # the square
    for nl, terms in ((1, 1), (L - 1, 2), (L, 5)):
        assert ts(c._h, A, B, far, terms, 1, nl) == NODEVICE, (nl, terms)
    # relinearize_batch(ctx, in3, rlk, out, n_ct, nl)
    for i in range(3):
        args = [A, K, far]
        args[i] = None
        assert refused(c, rl(c._h, *args, 1, L), "null argument"), i
    for nl in (0, L + 1):
        assert refused(c, rl(c._h, A, K, far, 1, nl), "nl out of range"), nl
    assert refused(c, rl(c._h, A + 8, K, far, 1, L), "16-byte aligned")
    assert refused(c, rl(c._h, A, K, far + 8, 1, L), "16-byte aligned")
    assert refused(c, rl(c._h, A, K, A, 1, L), "output overlaps input")                             # in place
    assert refused(c, rl(c._h, A, K, A + ct(1, L, 3) - 16, 1, L), "output overlaps input")          # out starts inside in3
    assert refused(c, rl(c._h, far + ct(1, L) - 16, K, far, 1, L), "output overlaps input")         # in3 starts inside out
    assert rl(c._h, A, K, far, 0, L) == 0
    assert rl(c._h, A, K, A + ct(1, L, 3), 1, L) == NODEVICE
    for nl in (1, L - 1, L):
        assert rl(c._h, A, K, far, 1, nl) == NODEVICE, nl
    # mult_relin_batch(ctx, a, b, rlk, out, n_ct, nl)
    for i in range(4):
        args = [A, B, K, far]
        args[i] = None
        assert refused(c, mr(c._h, *args, 1, L), "null argument"), i
    for nl in (0, L + 1):
        assert refused(c, mr(c._h, A, B, K, far, 1, nl), "nl out of range"), nl
    for args in ((A + 8, B, K, far), (A, B + 8, K, far), (A, B, K, far + 8)):
        assert refused(c, mr(c._h, *args, 1, L), "16-byte aligned"), args
    assert refused(c, mr(c._h, A, B, K, A + 16, 1, L), "output partially overlaps an input")
    assert refused(c, mr(c._h, A, B, K, B + ct(1, L) - 16, 1, L), "output partially overlaps an input")
    assert refused(c, mr(c._h, A + ct(1, L), B, K, A, 2, L), "output partially overlaps an input")  # a starts inside out
    assert refused(c, mr(c._h, A, A + 16, K, A, 1, L), "output partially overlaps an input")        # out is a, but cuts b
    assert mr(c._h, A, B, K, far, 0, L) == 0
    for args in ((A, B, K, far), (A, B, K, A), (A, B, K, B), (A, A, K, far), (A, A, K, A), (A, B, K, A + ct(1, L))):
        assert mr(c._h, *args, 1, L) == NODEVICE, args
    for nl in (1, L - 1):
        assert mr(c._h, A, B, K, far, 1, nl) == NODEVICE, nl


def test_product_methods_raise_on_a_host_only_context(host_ctx):
    from ppqsflhe_amd.binding import MkckksError
    c = host_ctx
    A, B, K, far = 1 << 20, 1 << 30, 1 << 36, 1 << 40
    calls = [lambda: c.relin_keygen(8, 8, 8, 8, 8, far), lambda: c.tensor_sum(A, B, far, 1, 1, c.L),
             lambda: c.relinearize(A, K, far, 1, c.L), lambda: c.mult_relin(A, B, K, A, 1, c.L)]
    for i, call in enumerate(calls):
        with pytest.raises(MkckksError) as ei:
            call()
        assert ei.value.code == NODEVICE, i
    with pytest.raises(MkckksError) as ei:
        c.tensor_sum(A, B, far, 0, 1, c.L)
    assert ei.value.code == INVALID and "n_terms" in str(ei.value)
    with pytest.raises(MkckksError) as ei:
        c.relinearize(A, K, A, 1, c.L)
    assert ei.value.code == INVALID and "overlaps" in str(ei.value)


def test_product_bookkeeping_under_sanitizers():
    r = subprocess.run(["make", "-C", HOST, "-s", "build/asan/product_selftest"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(HOST, "build", "asan", "product_selftest")], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "product selftest ok" in r.stdout and "FAIL" not in r.stdout, r.stdout
