"""The baby-step giant-step linear transform, the part that needs no GPU (include/mkckks.h:
mkckks_linear_transform_bsgs_batch): the symbol is declared, bound and exported; every refusal, decided before a device is
asked for, on a device = -1 context; MKCKKS_E_NODEVICE for every accepted call."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "mkckks_linear_transform_bsgs_batch"
INVALID, NODEVICE = -1, -2
BSGS_MAX = 64


def test_the_symbol_is_declared_bound_and_exported():
    from ppqsflhe_amd import Context, binding
    raw = open(os.path.join(ROOT, "include", "mkckks.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, hdr)
    assert re.search(r"#define\s+MKCKKS_BSGS_MAX\s+%d\b" % BSGS_MAX, hdr)
    assert SYMBOL in binding.SYMBOLS and hasattr(binding.load_library(), SYMBOL)
    assert callable(getattr(Context, "linear_transform_bsgs", None))
    section = raw[raw.index("baby-step giant-step form of the same transform"):raw.index(SYMBOL + "(")]
    for word in ("rolled RIGHT", "h_present", "MKCKKS_BSGS_WS_MIB", "ModDown(Ua_t)", "Refusals"):
        assert word in section, word


@pytest.fixture(scope="module")
def host_ctx():
    from ppqsflhe_amd import Context
    c = Context(12, 2, 40, 60, dnum=2, device=-1)
    yield c
    c.close()


def u32(*vals):
    return (C.c_uint32 * len(vals))(*vals)


def u8(*vals):
    return (C.c_uint8 * len(vals))(*vals)


def call(c, ct=16, bkeys=1 << 30, gb=None, n1=2, gkeys=1 << 32, gg=None, n2=3, pts=1 << 35, present=None, out=1 << 40, n_ct=1,
         nl=None):
    """Device pointers are never dereferenced: plain integers stand for them.  The three h_ arrays are host arrays."""
    N = c.N
    gb = u32(1, 5) if gb is None else gb
    gg = u32(1, 25, 2 * N - 1) if gg is None else gg
    present = u8(*([1] * (n1 * n2))) if present is None else present
    return getattr(c._L, SYMBOL)(c._h, ct, bkeys, gb, n1, gkeys, gg, n2, pts, present, out, n_ct, c.L if nl is None else nl)


def test_refusals_on_a_host_only_context(host_ctx):
    c = host_ctx
    N, L, far = c.N, c.L, 1 << 40
    assert call(c) == NODEVICE
    # null pointers
    for name in ("ct", "pts", "out"):
        assert call(c, **{name: None}) == INVALID, name
    fn = getattr(c._L, SYMBOL)
    good_gb, good_gg, pres = u32(1, 5), u32(1, 25, 2 * N - 1), u8(1, 1, 1, 1, 1, 1)
    assert fn(c._h, 16, 1 << 30, None, 2, 1 << 32, good_gg, 3, 1 << 35, pres, far, 1, L) == INVALID
    assert fn(c._h, 16, 1 << 30, good_gb, 2, 1 << 32, None, 3, 1 << 35, pres, far, 1, L) == INVALID
    assert fn(c._h, 16, 1 << 30, good_gb, 2, 1 << 32, good_gg, 3, 1 << 35, None, far, 1, L) == INVALID
    assert fn(None, 16, 1 << 30, good_gb, 2, 1 << 32, good_gg, 3, 1 << 35, pres, far, 1, L) == INVALID
    # keys: a keyed element needs its array; a list of ones needs none
    assert call(c, bkeys=None) == INVALID and call(c, gkeys=None) == INVALID
    assert call(c, bkeys=None, gb=u32(1, 1)) == NODEVICE
    assert call(c, gkeys=None, gg=u32(1, 1, 1)) == NODEVICE
    # Galois elements: even, or not below 2N, in either list; past the count: not read
    for bad in (0, 2, 4, 2 * N, 2 * N + 1, 0xFFFFFFFF):
        assert call(c, gb=u32(bad, 5)) == INVALID and call(c, gg=u32(1, bad, 5)) == INVALID, bad
        assert call(c, gb=u32(1, 5, bad)) == NODEVICE and call(c, gg=u32(1, 25, 5, bad)) == NODEVICE, bad
    # the counts
    many = u32(*([5] * (BSGS_MAX + 1)))
    for n in (0, BSGS_MAX + 1):
        assert call(c, n1=n, gb=many, present=u8(*([1] * 3 * (BSGS_MAX + 1)))) == INVALID, n
        assert call(c, n2=n, gg=many, present=u8(*([1] * 2 * (BSGS_MAX + 1)))) == INVALID, n
    assert "MKCKKS_BSGS_MAX" in c._L.mkckks_last_error().decode()
    assert call(c, n1=BSGS_MAX, gb=many, n2=BSGS_MAX, gg=many, present=u8(*([1] * BSGS_MAX * BSGS_MAX))) == NODEVICE
    # nl
    for nl in (0, L + 1):
        assert call(c, nl=nl) == INVALID, nl
    for nl in (1, L - 1, L):
        assert call(c, nl=nl) == NODEVICE, nl
    # overlaps
    ct_bytes = 2 * L * N * 8
    assert call(c, out=16) == INVALID                                   # in place
    assert call(c, out=16 + ct_bytes, n_ct=2) == INVALID                # output starting inside the input
    assert call(c, ct=far + ct_bytes, n_ct=2) == INVALID                # input starting inside the output
    assert call(c, pts=far + 16) == INVALID                             # output over the plaintexts
    assert call(c, pts=far - 16) == INVALID                             # the plaintexts reach into the output
    assert call(c, bkeys=far - 16) == INVALID and call(c, gkeys=far - 16) == INVALID  # output over the keys
    assert call(c, out=16 + ct_bytes) == NODEVICE                       # adjacent, not overlapping
    # 16-byte alignment
    for name, base in (("ct", 16), ("bkeys", 1 << 30), ("gkeys", 1 << 32), ("pts", 1 << 35), ("out", far)):
        assert call(c, **{name: base + 8}) == INVALID, name
    # no-ops: no ciphertext, no present entry
    assert call(c, n_ct=0) == 0
    assert call(c, present=u8(0, 0, 0, 0, 0, 0)) == 0
    assert call(c, present=u8(0, 0, 0, 0, 0, 1)) == NODEVICE
    # duplicate elements are allowed
    assert call(c, gb=u32(5, 5), gg=u32(25, 25, 1)) == NODEVICE


def test_more_than_six_digits_are_refused():
    from ppqsflhe_amd import Context
    c = Context(10, 6, 50, 60, dnum=8, device=-1)
    try:
        assert c.beta == 8
        assert call(c) == INVALID
        assert "more than 6 key-switch digits" in c._L.mkckks_last_error().decode()
        assert call(c, nl=6 * c.alpha) == NODEVICE
    finally:
        c.close()


def test_the_method_raises_on_a_host_only_context(host_ctx):
    from ppqsflhe_amd.binding import MkckksError
    c = host_ctx
    far = 1 << 40
    with pytest.raises(MkckksError) as ei:
        c.linear_transform_bsgs(16, 1 << 30, [1, 5], None, [1], 1 << 35, [[1, 1]], far, 1, c.L)
    assert ei.value.code == NODEVICE
    with pytest.raises(MkckksError) as ei:
        c.linear_transform_bsgs(16, 1 << 30, [1, 4], None, [1], 1 << 35, [[1, 1]], far, 1, c.L)
    assert ei.value.code == INVALID and "Galois element" in str(ei.value)
    with pytest.raises(ValueError):
        c.linear_transform_bsgs(16, 1 << 30, [1, 5], None, [1], 1 << 35, [[1]], far, 1, c.L)
    c.linear_transform_bsgs(16, 1 << 30, [1, 5], None, [1], 1 << 35, [[0, 0]], far, 1, c.L)  # nothing present: a no-op
