"""Fan-out re-encryption (include/mkckks.h: mkckks_reencrypt_fanout_batch): one ciphertext batch into many key domains,
out[k][b] = ReEncrypt(ct[b], evks[k]), with the key-independent half of the key switch computed once per ciphertext.

CPU: the C-ABI surface and the argument checks on a host-only context.  GPU: every word against the oracle's
`reencrypt` (and against the single-key device entry point where the oracle is too slow), the library's switches, and the
distribution leg of `serverRound --back`, which now goes through this entry point."""
import json
import os
import re

import numpy as np
import pytest

from tests.test_cli_hosts import _small_cc, _weights, run
from tests.test_gpu_parity import CONFIGS, rand_ct, rand_polys
from tests.test_seeded_ciphertexts import read_mkws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "mkckks_reencrypt_fanout_batch"


# ---- CPU: surface and argument checks -------------------------------------------------------------------------------

def test_fanout_symbol_is_declared_bound_and_exported():
    from ppqsflhe_amd import Context, binding
    hdr = open(os.path.join(ROOT, "include", "mkckks.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert "server_fns.sh:76-80" in hdr and "changeCipherDomain.cpp:74" in hdr  # the call sites it replaces
    assert SYMBOL in binding.SYMBOLS
    assert hasattr(binding.load_library(), SYMBOL)
    assert callable(getattr(Context, "reencrypt_fanout", None))


def test_fanout_argument_checks_on_a_host_only_context():
    from ppqsflhe_amd import Context
    from ppqsflhe_amd.binding import MkckksError
    c = Context(12, 1, 40, 60, dnum=2, device=-1)
    f = getattr(c._L, SYMBOL)
    try:
        # pointers are never dereferenced: argument checks, then the host-only check
        assert f(c._h, None, 8, 8, 1, 1, 1) == -1
        assert f(c._h, 8, None, 8, 1, 1, 1) == -1
        assert f(c._h, 8, 8, None, 1, 1, 1) == -1
        assert f(c._h, 8, 8, 1 << 30, 1, 1, 0) == -1
        assert f(c._h, 8, 8, 1 << 30, 1, 1, c.L + 1) == -1
        assert f(c._h, 8, 8, 1 << 30, 1, 1, c.L) == -2
        assert f(c._h, 8, 8, 1 << 30, 0, 1, c.L) == 0
        with pytest.raises(MkckksError) as ei:
            c.reencrypt_fanout(8, 8, 1 << 30, 1, 1, c.L)
        assert ei.value.code == -2
    finally:
        c.close()


# ---- GPU ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctxs():
    from oracle.oracle import OracleContext
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


def rand_evks(rng, g, n_keys):
    return np.stack([rand_polys(rng, g, list(range(g.D)) * (2 * g.beta), 1).reshape(g.beta, 2, g.D, g.N)
                     for _ in range(n_keys)])


def fanout(g, ct, evks, nl):
    n_keys, B = evks.shape[0], ct.shape[0]
    d_out = g.empty((n_keys, B, 2, nl, g.N))
    g.reencrypt_fanout(g.to_device(ct), g.to_device(evks), d_out, n_keys, B, nl)
    return d_out.to_host()


def check_against_oracle(g, o, ct, evks, nl, tag):
    got = fanout(g, ct, evks, nl)
    for k in range(evks.shape[0]):
        for b in range(ct.shape[0]):
            assert np.array_equal(got[k, b], o.reencrypt(ct[b], evks[k])), (tag, nl, k, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl,n_keys,B", [
    ("tiny", 5, 3, 2), ("tiny", 1, 2, 1), ("c1", 3, 2, 2), ("ref", 4, 3, 3),
    ("ref", 3, 2, 2),    # partial last digit
    ("ref", 2, 2, 2),    # single digit
    ("c3", 12, 3, 2),
    ("c3", 11, 7, 2),    # the shape of the real back leg
    ("c3", 9, 2, 1), ("c3", 4, 2, 1), ("c3", 2, 2, 1), ("c5s", 20, 2, 1), ("c5s", 15, 2, 1),
    ("n17", 4, 3, 2), ("n17", 3, 2, 1), ("n11", 4, 2, 2)])
def test_fanout_matches_the_oracle(ctxs, name, nl, n_keys, B):
    g, o = ctxs(name)
    rng = np.random.default_rng(1000 + 31 * nl + n_keys)
    check_against_oracle(g, o, rand_ct(rng, g, nl, B), rand_evks(rng, g, n_keys), nl, name)


@pytest.mark.gpu
@pytest.mark.parametrize("nl", [20, 15])
def test_fanout_n17_at_its_real_limb_structure(nl):
    """N = 2^17, L = 20, dnum = 3 (alpha = K = 7): the <3, 3, .> instances of the fused kernels, all words vs the oracle."""
    from oracle.oracle import OracleContext
    from ppqsflhe_amd import Context
    g, o = Context(17, 18, 50, 60, dnum=3, device=0), OracleContext(17, 18, 50, 60, dnum=3)
    try:
        rng = np.random.default_rng(170 + nl)
        check_against_oracle(g, o, rand_ct(rng, g, nl, 1), rand_evks(rng, g, 2), nl, "n17-real")
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl,n_keys,B", [("ref", 4, 9, 19),   # more keys than one group, more ciphertexts than one chunk
                                              ("c3", 11, 7, 16)])  # the real back leg at its real batch
def test_fanout_equals_the_loop_of_single_key_calls(ctxs, name, nl, n_keys, B):
    g, _ = ctxs(name)
    rng = np.random.default_rng(7 * n_keys + B)
    ct, evks = rand_ct(rng, g, nl, B), rand_evks(rng, g, n_keys)
    d_ct, d_evks = g.to_device(ct), g.to_device(evks)
    d_out, d_one = g.empty((n_keys, B, 2, nl, g.N)), g.empty((B, 2, nl, g.N))
    g.reencrypt_fanout(d_ct, d_evks, d_out, n_keys, B, nl)
    got = d_out.to_host()
    evk_words = g.beta * 2 * g.D * g.N
    for k in range(n_keys):
        g.reencrypt(d_ct, d_evks.view(k * evk_words, (g.beta, 2, g.D, g.N)), d_one, B, nl)
        assert np.array_equal(got[k], d_one.to_host()), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl", [("c3", 12), ("ref", 4), ("n17", 4)])
def test_fanout_extreme_residues(ctxs, name, nl):
    """Maximal operands (the pattern of test_reencrypt_sum_extreme_residues): ciphertexts with every residue q - 1, all 0
    and alternating 0 / q - 1, against keys with every residue q - 1 and alternating ones."""
    g, o = ctxs(name)
    B, n_keys = 3, 2
    idx = np.arange(g.N)
    ct = np.zeros((B, 2, nl, g.N), dtype=np.uint64)
    evks = np.zeros((n_keys, g.beta, 2, g.D, g.N), dtype=np.uint64)
    for b, m in ((0, np.ones(g.N, dtype=bool)), (2, (idx // 8) % 2 == 0)):  # ciphertext 1 stays all 0
        for l in range(nl):
            ct[b, :, l, m] = int(g.moduli[l]) - 1
    for k in range(n_keys):
        m = np.ones(g.N, dtype=bool) if k == 0 else ((idx // (1 << (3 * k))) % 2 == 0)
        for l in range(g.D):
            evks[k, :, :, l, m] = int(g.moduli[l]) - 1
    check_against_oracle(g, o, ct, evks, nl, name + "-extreme")


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl", [("c3", 12), ("ref", 4)])
@pytest.mark.parametrize("env", [{"MKCKKS_FANOUT_GROUP": "1"}, {"MKCKKS_FANOUT_GROUP": "2"}, {"MKCKKS_FANOUT_GROUP": "3"},
                                 {"MKCKKS_CHUNK": "1"}, {"MKCKKS_GENERIC_NTT": "1"}, {"MKCKKS_NO_PM": "1"},
                                 {"MKCKKS_NO_FP64": "1"}, {"MKCKKS_CU_AFFINE": "0"}])
def test_fanout_under_the_library_switches(ctxs, monkeypatch, env, name, nl):
    """Switches are read once, when a context is created: a fresh context under each must give the oracle's bits."""
    from ppqsflhe_amd import Context
    _, o = ctxs(name)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a = CONFIGS[name]
    g = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)
    try:
        rng = np.random.default_rng(55 + nl)
        check_against_oracle(g, o, rand_ct(rng, g, nl, 2), rand_evks(rng, g, 4), nl, (name, env))
    finally:
        g.close()


@pytest.mark.gpu
def test_fanout_call_properties(ctxs):
    """Two calls give the same bits; the input is not written; overlapping output is refused; empty calls write nothing;
    a call on another stream agrees."""
    import torch
    from ppqsflhe_amd.binding import MkckksError
    g, _ = ctxs("c3")
    nl, n_keys, B = 11, 3, 2
    rng = np.random.default_rng(4242)
    ct, evks = rand_ct(rng, g, nl, B), rand_evks(rng, g, n_keys)
    d_ct, d_evks = g.to_device(ct), g.to_device(evks)
    d_out = g.empty((n_keys, B, 2, nl, g.N))
    g.reencrypt_fanout(d_ct, d_evks, d_out, n_keys, B, nl)
    first = d_out.to_host()
    g.reencrypt_fanout(d_ct, d_evks, d_out, n_keys, B, nl)
    assert np.array_equal(d_out.to_host(), first)
    assert np.array_equal(d_ct.to_host(), ct)
    # overlap: output starting inside the input, and input starting inside the output
    ct_words = 2 * nl * g.N
    d_big = g.empty((n_keys * B + B, 2, nl, g.N))
    with pytest.raises(MkckksError) as ei:
        g.reencrypt_fanout(d_ct, d_evks, d_ct, 1, B, nl)
    assert ei.value.code == -1
    with pytest.raises(MkckksError):
        g.reencrypt_fanout(d_big.view((B - 1) * ct_words, (B, 2, nl, g.N)), d_evks, d_big, n_keys, B, nl)
    with pytest.raises(MkckksError):
        g.reencrypt_fanout(d_big, d_evks, d_big.view(ct_words, (n_keys * B, 2, nl, g.N)), n_keys, B, nl)
    # adjacent, not overlapping: accepted
    g.reencrypt_fanout(d_big.upload(np.concatenate([ct, np.zeros((n_keys * B, 2, nl, g.N), dtype=np.uint64)])), d_evks,
                       d_big.view(B * ct_words, (n_keys, B, 2, nl, g.N)), n_keys, B, nl)
    assert np.array_equal(d_big.to_host()[B:].reshape(first.shape), first)
    # empty calls leave the output alone
    poison = np.full((n_keys, B, 2, nl, g.N), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    d_out.upload(poison)
    g.reencrypt_fanout(d_ct, d_evks, d_out, 0, B, nl)
    g.reencrypt_fanout(d_ct, d_evks, d_out, n_keys, 0, nl)
    assert np.array_equal(d_out.to_host(), poison)
    # a non-default stream
    s = torch.cuda.Stream()
    g.set_stream(s.cuda_stream)
    try:
        g.reencrypt_fanout(d_ct, d_evks, d_out, n_keys, B, nl)
        g.sync()
    finally:
        g.set_stream(None)
    assert np.array_equal(d_out.to_host(), first)


# ---- GPU: the distribution leg of serverRound -----------------------------------------------------------------------

def _ok(r):
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def _round_inputs(tmp_path, n, ext, seed):
    """n clients with keys, encrypted weights (envelope form by extension), inbound keys towards client n-1 and one back
    key per other client; returns (cc, plaintext values, inbound arguments, back key paths)."""
    cc = _small_cc(tmp_path)
    rng = np.random.default_rng(seed)
    vals = [[("dense", rng.uniform(-0.3, 0.3, 2 * 8192 + 300)), ("bias", rng.uniform(-0.3, 0.3, 4))] for _ in range(n)]
    for c in range(n):
        _ok(run("keyGen", cc, tmp_path / f"pk{c}", tmp_path / f"sk{c}"))
        _ok(run("encryptModelWeights", cc, tmp_path / f"pk{c}", _weights(tmp_path, f"w{c}.json", vals[c]),
                tmp_path / f"enc{c}.{ext}"))
    target = n - 1
    args, back_keys = ["-", tmp_path / f"enc{target}.{ext}"], []
    for c in range(n - 1):
        _ok(run("REkeyGen", cc, tmp_path / f"sk{c}", tmp_path / f"pk{target}", tmp_path / f"rk{c}"))
        _ok(run("REkeyGen", cc, tmp_path / f"sk{target}", tmp_path / f"pk{c}", tmp_path / f"rkback{c}"))
        args += [tmp_path / f"rk{c}", tmp_path / f"enc{c}.{ext}"]
        back_keys.append(tmp_path / f"rkback{c}")
    return cc, vals, args, back_keys


def _same_bytes(a, b):
    return open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.gpu
@pytest.mark.parametrize("ext", ["json", "mkws"])
def test_server_round_back_leg_is_one_fanout(tmp_path, ext):
    """A 4-client round with 3 --back keys: every back file equals changeCipherDomain run on the aggregate file and the
    file the per-key loop (MKCKKS_BACK_LOOP=1) writes; every client decrypts the mean with its own key."""
    n = 4
    cc, vals, args, back_keys = _round_inputs(tmp_path, n, ext, 300 + len(ext))
    back = [x for c in range(n - 1) for x in (back_keys[c], tmp_path / f"for{c}.{ext}")]
    loop = [x for c in range(n - 1) for x in (back_keys[c], tmp_path / f"loop{c}.{ext}")]
    r = _ok(run("serverRound", cc, tmp_path / f"agg.{ext}", *args, "--back", *back))
    assert r.stdout.count("[round] aggregate re-encrypted with") == n - 1
    rl = _ok(run("serverRound", cc, tmp_path / f"aggL.{ext}", *args, "--back", *loop, env={"MKCKKS_BACK_LOOP": "1"}))
    assert rl.stdout.count("[round] aggregate re-encrypted with") == n - 1
    assert _same_bytes(tmp_path / f"agg.{ext}", tmp_path / f"aggL.{ext}")
    mean = [np.mean([np.asarray(vals[c][li][1]) for c in range(n)], axis=0) for li in range(2)]
    for c in range(n - 1):
        assert _same_bytes(tmp_path / f"for{c}.{ext}", tmp_path / f"loop{c}.{ext}"), c
        _ok(run("changeCipherDomain", cc, back_keys[c], tmp_path / f"agg.{ext}", tmp_path / f"ref{c}.{ext}"))
        if ext == "json":
            assert json.load(open(tmp_path / f"for{c}.json")) == json.load(open(tmp_path / f"ref{c}.json"))
        else:
            assert read_mkws(tmp_path / f"for{c}.mkws")[1]  # a well-formed container with blobs
            assert _same_bytes(tmp_path / f"for{c}.mkws", tmp_path / f"ref{c}.mkws"), c
        _ok(run("decryptModelWeights", cc, tmp_path / f"sk{c}", tmp_path / f"for{c}.{ext}", tmp_path / f"dec{c}.json"))
        dec = json.load(open(tmp_path / f"dec{c}.json"))["weights_summary"]
        for li in range(2):
            assert np.abs(np.array(dec[li]["values"]) - mean[li]).max() < 2.0 ** -24, (c, li)


@pytest.mark.gpu
def test_server_rounds_keep_the_back_keys_by_name(tmp_path):
    """--rounds: two rounds naming the same back keys and a third naming them in another order write the one-shot files
    (resident keys are matched by file name, not by position)."""
    n = 4
    cc, _, args, back_keys = _round_inputs(tmp_path, n, "mkws", 909)
    one = [x for c in range(n - 1) for x in (back_keys[c], tmp_path / f"one{c}.mkws")]
    _ok(run("serverRound", cc, tmp_path / "agg.mkws", *args, "--back", *one))
    lines = []
    for rd, order in enumerate([(0, 1, 2), (0, 1, 2), (2, 0, 1)]):
        back = [x for c in order for x in (back_keys[c], tmp_path / f"r{rd}_for{c}.mkws")]
        lines.append(" ".join(map(str, [tmp_path / f"r{rd}.mkws", *args, "--back", *back])))
    rounds = tmp_path / "rounds.txt"
    rounds.write_text("\n".join(lines) + "\n")
    r = _ok(run("serverRound", cc, "--rounds", rounds))
    for rd in range(3):
        assert _same_bytes(tmp_path / f"r{rd}.mkws", tmp_path / "agg.mkws")
        for c in range(n - 1):
            assert _same_bytes(tmp_path / f"r{rd}_for{c}.mkws", tmp_path / f"one{c}.mkws"), (rd, c)


@pytest.mark.gpu
def test_server_round_reports_the_back_leg_and_keeps_its_keys_resident(tmp_path):
    """The `[round] back leg:` line follows the per-key lines; under --rounds a second round naming the same back keys
    uploads none of them."""
    n = 3
    cc, _, args, back_keys = _round_inputs(tmp_path, n, "mkws", 77)
    line = r"\[round\] back leg: 2 keys x (\d+) ciphertexts in \S+ ms -> \S+ ciphertexts/s, (\d+) key\(s\) uploaded"
    lines = []
    for rd in range(2):
        back = [x for c in range(n - 1) for x in (back_keys[c], tmp_path / f"r{rd}_for{c}.mkws")]
        lines.append(" ".join(map(str, [tmp_path / f"r{rd}.mkws", *args, "--back", *back])))
    rounds = tmp_path / "rounds.txt"
    rounds.write_text("\n".join(lines) + "\n")
    r = _ok(run("serverRound", cc, "--rounds", rounds))
    legs = re.findall(line, r.stdout)
    assert [u for _, u in legs] == ["2", "0"] and legs[0][0] == legs[1][0] and int(legs[0][0]) > 0
    out = r.stdout
    assert out.index("[round] back leg:") > out.index("[round] aggregate re-encrypted with")
    back = [x for c in range(n - 1) for x in (back_keys[c], tmp_path / f"loop{c}.mkws")]
    rl = _ok(run("serverRound", cc, tmp_path / "aggL.mkws", *args, "--back", *back, env={"MKCKKS_BACK_LOOP": "1"}))
    assert [u for _, u in re.findall(line, rl.stdout)] == ["2"]
    for c in range(n - 1):
        assert _same_bytes(tmp_path / f"loop{c}.mkws", tmp_path / f"r1_for{c}.mkws")
