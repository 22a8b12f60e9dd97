"""The walk of k_row3_inner_int: a workgroup owns (client, limb slot, row tile) and walks MK_INNER_WALK consecutive
ciphertext indices of that client (ntt_radix.hpp).  Every case is bit-exact against the oracle chain reencrypt x C +
eval_add, at the smallest shapes at which the walk can go wrong: an index count below the walk length, counts that
are no multiple of it (a last, shorter walk), walks that end at a client boundary, a workspace chunk shorter than
the walk, the running sum across client groups, the one-client default of the single re-encryption, a partial last
digit, and the 512-point-row instance.

Runs on a real MI355X (`-m gpu`).
"""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.oracle import OracleContext  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CONFIGS = {
    # name: (log_n, depth, scaling_bits, first_bits, dnum)
    "ref": (14, 2, 40, 60, 2),   # 256-point rows, merged n-client flow
    "c3": (16, 10, 50, 60, 3),   # the flagship ring: L = 12, dnum = 3
    "n17": (17, 2, 50, 60, 2),   # 512-point rows
}


def walk_length():
    """The library's compile-time walk length, read from the source that defines it."""
    with open(os.path.join(ROOT, "ppqsflhe_amd", "csrc", "ntt_radix.hpp")) as f:
        m = re.search(r"^#define MK_INNER_WALK (\d+)", f.read(), re.M)
    assert m, "MK_INNER_WALK is not defined in ntt_radix.hpp"
    return int(m.group(1))


W = walk_length()


@pytest.fixture(scope="module")
def ctxs():
    from ppqsflhe_amd import Context
    cache = {}

    def get(name):
        if name not in cache:
            a = CONFIGS[name]
            cache[name] = (Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0),
                           OracleContext(a[0], a[1], a[2], a[3], dnum=a[4]))
        return cache[name]

    yield get
    for g, _ in cache.values():
        g.close()


def rand_polys(rng, ctx, limb_ids, count):
    out = np.empty((count, len(limb_ids), ctx.N), dtype=np.uint64)
    for j, l in enumerate(limb_ids):
        out[:, j, :] = rng.integers(0, int(ctx.moduli[l]), size=(count, ctx.N), dtype=np.uint64)
    return out


def oracle_chain(o, cts, evks):
    """The clients' individual re-encryptions [C][B][2][nl][N] and, per index, their EvalAdd chain [B][2][nl][N]."""
    C, B = cts.shape[:2]
    per = np.stack([np.stack([o.reencrypt(cts[c, b], evks[c]) for b in range(B)]) for c in range(C)])
    out = []
    for b in range(B):
        acc = per[0, b]
        for c in range(1, C):
            acc = o.eval_add(acc, per[c, b])
        out.append(acc)
    return per, np.stack(out)


_cases = {}


def case(ctxs, name, nl, C, B):
    """Seeded inputs and their oracle result, computed once per shape and shared (read-only) by the tests."""
    key = (name, nl, C, B)
    if key not in _cases:
        g, o = ctxs(name)
        rng = np.random.default_rng(4100 + 97 * nl + 13 * C + B)
        cts = rand_polys(rng, g, list(range(nl)) * 2, C * B).reshape(C, B, 2, nl, g.N)
        evks = rand_polys(rng, g, list(range(g.D)) * (2 * g.beta), C).reshape(C, g.beta, 2, g.D, g.N)
        per, want = oracle_chain(o, cts, evks)
        for a in (cts, evks, per, want):
            a.setflags(write=False)
        _cases[key] = (cts, evks, per, want)
    return _cases[key]


def gpu_sum(g, cts, evks, nl):
    C, B = cts.shape[:2]
    d_out = g.empty((B, 2, nl, g.N))
    g.reencrypt_sum(g.to_device(cts), g.to_device(evks), d_out, C, B, nl)
    return d_out.to_host()


SHAPES = [(1, 1), (2, 3), (3, 5), (2, 2 * W + 1)]


@pytest.mark.parametrize("C,B", SHAPES)
@pytest.mark.parametrize("nl", [4, 3])
def test_walk_reencrypt_sum_ref(ctxs, nl, C, B):
    """Index counts below the walk length, no multiple of it, and walks that end at a client boundary."""
    g, _ = ctxs("ref")
    cts, evks, _, want = case(ctxs, "ref", nl, C, B)
    assert np.array_equal(gpu_sum(g, cts, evks, nl), want)


@pytest.mark.parametrize("env", [{"MKCKKS_CHUNK": "2"},         # a workspace chunk shorter than the walk
                                 {"MKCKKS_QSUM_GROUP": "2"}])   # the running sum across client groups (2 + 1 clients)
def test_walk_under_chunk_and_client_groups(ctxs, monkeypatch, env):
    from ppqsflhe_amd import Context
    nl, C, B = 4, 3, 5
    cts, evks, _, want = case(ctxs, "ref", nl, C, B)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a = CONFIGS["ref"]
    g2 = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)  # switches are read once, when a context is created
    try:
        assert np.array_equal(gpu_sum(g2, cts, evks, nl), want)
    finally:
        g2.close()


def test_walk_extreme_residues(ctxs):
    """Maximal operands through every item of a walk: every residue q - 1 (client 0), alternating 0 / q - 1 (client 1)."""
    g, o = ctxs("ref")
    nl, C, B = 4, 2, 5
    cts = np.zeros((C, B, 2, nl, g.N), dtype=np.uint64)
    evks = np.zeros((C, g.beta, 2, g.D, g.N), dtype=np.uint64)
    idx = np.arange(g.N)
    for c in range(C):
        m = np.ones(g.N, dtype=bool) if c == 0 else ((idx // (1 << (3 * c))) % 2 == 0)
        for l in range(nl):
            cts[c, :, :, l, m] = int(g.moduli[l]) - 1
        for l in range(g.D):
            evks[c, :, :, l, m] = int(g.moduli[l]) - 1
    # the B ciphertexts of a client are equal here, so one oracle chain serves every index
    want = oracle_chain(o, cts[:, :1], evks)[1][0]
    got = gpu_sum(g, cts, evks, nl)
    for b in range(B):
        assert np.array_equal(got[b], want), b


def test_walk_single_reencrypt_and_accumulate(ctxs):
    """The one-client default of the single re-encryption (every index belongs to one client): B = 5 is no multiple
    of the walk length."""
    g, _ = ctxs("ref")
    nl, C, B = 4, 2, 5
    cts, evks, per, want = case(ctxs, "ref", nl, C, B)
    d_acc = g.empty((B, 2, nl, g.N))
    g.reencrypt(g.to_device(cts[0]), g.to_device(evks[0]), d_acc, B, nl)
    assert np.array_equal(d_acc.to_host(), per[0])
    g.reencrypt_accumulate(g.to_device(cts[1]), g.to_device(evks[1]), d_acc, B, nl)
    assert np.array_equal(d_acc.to_host(), want)


@pytest.mark.parametrize("nl", [12, 9])  # nl = 9: the last digit is partial
def test_walk_flagship_ring(ctxs, nl):
    g, _ = ctxs("c3")
    cts, evks, _, want = case(ctxs, "c3", nl, 2, 5)
    assert np.array_equal(gpu_sum(g, cts, evks, nl), want)


def test_walk_512_point_rows(ctxs):
    g, _ = ctxs("n17")
    cts, evks, _, want = case(ctxs, "n17", 4, 2, 3)
    assert np.array_equal(gpu_sum(g, cts, evks, 4), want)
