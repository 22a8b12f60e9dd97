"""Seeded secret-key ciphertexts (include/mkckks.h: mkckks_encrypt_seeded_batch / mkckks_expand_seeded_batch;
KIND_CT_SEEDED containers in ppqsflhe_amd/host).  A client sends c0 and a 40-byte seed instead of (c0, c1); the server
rebuilds c1 = a on the GPU as word i*N + j of the ChaCha20 uniform stream that mkckks_sample_uniform already defines.

CPU: the C-ABI surface, the usage text, hostile seeded containers under ASan/UBSan.  GPU: the expansion against the
existing sampler and a numpy restatement, the encryption against Python integers, and whole rounds through the CLIs."""
import base64
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.test_cli_hosts import _small_cc, _weights, run
from tests.test_decode_flood import chacha20_blocks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppqsflhe_amd", "host")
HDR_FMT = "<4sIIIIIIIdII"  # BlobHeader: magic, version, kind, ring_dim, limbs, parts, level, noise_deg, scale, slots, reserved
KIND_CT, KIND_CT_SEEDED = 1, 5


# ---- containers (Python side of hostlib.hpp)

def read_mkws(path):
    raw = open(path, "rb").read()
    assert raw[:4] == b"MKWS"
    _, skel_len = struct.unpack_from("<IQ", raw, 4)
    skel, pos = raw[16:16 + skel_len], 16 + skel_len
    (n,) = struct.unpack_from("<Q", raw, pos)
    pos += 8
    blobs = []
    for _ in range(n):
        (sz,) = struct.unpack_from("<Q", raw, pos)
        blobs.append(raw[pos + 8:pos + 8 + sz])
        pos += 8 + sz
    assert pos == len(raw)
    return skel, blobs


def write_mkws(path, skel, blobs):
    with open(path, "wb") as f:
        f.write(b"MKWS" + struct.pack("<IQ", 1, len(skel)) + skel + struct.pack("<Q", len(blobs)))
        for b in blobs:
            f.write(struct.pack("<Q", len(b)) + b)


def mkws_to_json(src, dst):
    """the same document as a JSON envelope (base64 blobs in place of the "@<index>" references)"""
    skel, blobs = read_mkws(src)
    doc = json.loads(skel)
    for lay in doc["weights_summary"]:
        for k in ("mean", "std_dev"):
            lay[k] = base64.b64encode(blobs[int(lay[k][1:])]).decode()
        lay["values"] = [base64.b64encode(blobs[int(v[1:])]).decode() for v in lay["values"]]
    with open(dst, "w") as f:
        json.dump(doc, f)


def seeded_parts(blob, N):
    h = struct.unpack_from(HDR_FMT, blob, 0)
    assert h[0] == b"MKCK" and h[2] == KIND_CT_SEEDED and h[5] == 1
    nl = h[4]
    key, sid, pad = blob[48:80], *struct.unpack_from("<II", blob, 80)
    assert pad == 0 and len(blob) == 48 + 40 + 8 * nl * N
    return h, key, sid, np.frombuffer(blob, dtype=np.uint64, offset=88).reshape(nl, N)


def expand_file(g, src, dst):
    """every seeded blob of an MKWS file -> a full container, c1 from Context.sample_uniform (not the new kernel)"""
    skel, blobs = read_mkws(src)
    out = []
    for b in blobs:
        h, key, sid, c0 = seeded_parts(b, g.N)
        nl = h[4]
        d_a = g.empty((1, nl, g.N))
        g.sample_uniform(d_a, 1, nl, 0, key, sid)
        hdr = struct.pack(HDR_FMT, h[0], h[1], KIND_CT, h[3], nl, 2, *h[6:])
        out.append(hdr + c0.tobytes() + d_a.to_host().tobytes())
    write_mkws(dst, skel, out)


# ---- numpy restatement of the stream (sampler_kernels.hpp: k_sample_uniform with n_polys = 1)

def uniform_stream(key, sid, moduli, N):
    """words i*N + j of stream sid reduced mod q_i, and how many of them were rejected at attempt 0"""
    nl = len(moduli)
    b = np.arange(nl * N // 8, dtype=np.uint64)
    blk = chacha20_blocks(key, (b & np.uint64(0xFFFFFFFF)).astype(np.uint32), (b >> np.uint64(32)).astype(np.uint32),
                          sid, 0).astype(np.uint64)
    words = (blk[:, 0::2] | (blk[:, 1::2] << np.uint64(32))).reshape(nl, N)
    out, rejected = np.empty((nl, N), dtype=np.uint64), 0
    for i, q in enumerate(int(m) for m in moduli):
        limit = 2 ** 64 - 2 ** 64 % q
        row = words[i].copy()
        for j in np.nonzero(row >= np.uint64(limit))[0]:
            rejected += 1
            pos = i * N + int(j)
            for att in range(1, 64):
                o = chacha20_blocks(key, [(pos >> 3) & 0xFFFFFFFF], [pos >> 35], sid, att)[0]
                r = int(o[2 * (pos & 7)]) | int(o[2 * (pos & 7) + 1]) << 32
                if r < limit:
                    break
            row[j] = r
        out[i] = row % np.uint64(q)
    return out, rejected


# ---- CPU

def test_entry_points_are_declared_and_bound():
    from ppqsflhe_amd import binding
    hdr = open(os.path.join(ROOT, "include", "mkckks.h")).read()
    for name in ("mkckks_encrypt_seeded_batch", "mkckks_expand_seeded_batch"):
        assert name + "(" in hdr and name in binding.SYMBOLS
    from ppqsflhe_amd import Context
    assert hasattr(Context, "encrypt_seeded") and hasattr(Context, "expand_seeded")


def test_argument_checks_without_a_device():
    import ctypes as C
    from ppqsflhe_amd import Context
    c = Context(12, 1, 40, 60, dnum=2, device=-1)
    L = c._L
    keys, sids = b"\0" * 32, (C.c_uint32 * 1)(0)
    assert L.mkckks_expand_seeded_batch(c._h, None, 1, 1, keys, sids) == -1          # null ciphertext
    assert L.mkckks_expand_seeded_batch(c._h, 8, 1, 1, None, sids) == -1             # null seed array
    assert L.mkckks_encrypt_seeded_batch(c._h, 8, 8, 8, 8, 1, 1, None, 0) == -1      # null seed
    assert L.mkckks_expand_seeded_batch(c._h, 8, 1, 1, keys, sids) == -2             # host-only context
    c.close()


def test_usage_names_both_forms():
    r = run("encryptModelWeights")
    assert r.returncode == 1
    assert "<cc_path> <pubkey_path> <input_weights> <output_encfile>" in r.stderr
    assert "<cc_path> <privkey_path> <input_weights> <output_encfile> --seeded" in r.stderr
    for args in (("a", "b", "c", "d", "--seed"), ("a", "b", "c", "d", "--seeded", "x"), ("a", "b", "c", "d", "e", "--seeded")):
        r = run("encryptModelWeights", *args)
        assert r.returncode == 1 and "Usage:" in r.stderr, args


def seeded_blob(N=64, nl=3, parts=1, pad=0, extra=b"", cut=0):
    hdr = struct.pack(HDR_FMT, b"MKCK", 1, KIND_CT_SEEDED, N, nl, parts, 1, 2, 2.0 ** 40, 32, 0)
    body = hdr + bytes(range(32)) + struct.pack("<II", 7, pad) + np.arange(nl * N, dtype=np.uint64).tobytes() + extra
    return body[:len(body) - cut]


def test_hostile_seeded_containers_under_asan(tmp_path):
    r = subprocess.run(["make", "-C", HOST, "-s", "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    exe = os.path.join(HOST, "build", "asan", "hostlib_selftest")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99",
               UBSAN_OPTIONS="halt_on_error=1:exitcode=98")

    def envelope(name, blob, binary):
        p = tmp_path / name
        if binary:
            skel = b'{"weights_summary": [{"layer": "l", "shape": [1], "mean": "@0", "std_dev": "@1", "values": []}]}'
            write_mkws(p, skel, [blob, blob])
        else:
            b64 = base64.b64encode(blob).decode()
            p.write_text(json.dumps({"weights_summary": [{"layer": "l", "shape": [1], "mean": b64, "std_dev": b64,
                                                          "values": []}]}))
        return subprocess.run([exe, "envelope", str(p)], capture_output=True, text=True, env=env, timeout=300)

    for binary in (False, True):
        r = envelope("good", seeded_blob(), binary)
        assert r.returncode == 0 and f"2 ciphertexts {2 * 3 * 64 * 8} bytes" in r.stdout, r.stderr
        for name, blob in {"truncated": seeded_blob(cut=8), "oversized": seeded_blob(extra=b"\0" * 8),
                           "parts": seeded_blob(parts=2), "pad": seeded_blob(pad=1), "trailer": seeded_blob()[:60],
                           "limbs": seeded_blob(nl=3)[:16] + struct.pack("<I", 0xFFFFFFFF) + seeded_blob()[20:]}.items():
            r = envelope(name, blob, binary)
            assert r.returncode == 1 and "ERROR" in r.stderr, (name, binary, r.stderr[-300:])
            assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (name, r.stderr[-500:])


# ---- GPU

@pytest.fixture(scope="module")
def ctxs():
    from ppqsflhe_amd import Context
    cache = {}

    def get(*args):
        if args not in cache:
            cache[args] = Context(*args[:4], dnum=args[4], device=0)
        return cache[args]

    yield get
    for g in cache.values():
        g.close()


def keys_of(rng, n):
    return [bytes(rng.integers(0, 256, 32, dtype=np.uint8)) for _ in range(n)]


@pytest.mark.gpu
def test_expansion_equals_the_existing_sampler(ctxs):
    rng = np.random.default_rng(11)
    g = ctxs(12, 10, 50, 60, 3)
    N = g.N
    restated = rejected = 0
    for nl in (1, 5, g.L):
        n = 6
        keys, sids = keys_of(rng, n), [int(x) for x in rng.integers(0, 2 ** 32, n)]
        ct = np.stack([rng.integers(0, 2 ** 62, (2, nl, N), dtype=np.uint64) for _ in range(n)])
        d_ct = g.to_device(ct)
        g.expand_seeded(d_ct, n, nl, keys, sids)
        got = d_ct.to_host()
        assert np.array_equal(got[:, 0], ct[:, 0])  # component 0 untouched
        for t in range(n):
            d_a = g.empty((1, nl, N))
            g.sample_uniform(d_a, 1, nl, 0, keys[t], sids[t])
            assert np.array_equal(got[t, 1], d_a.to_host()[0]), (nl, t)
            if nl == g.L and (restated < 2 or rejected == 0):  # numpy restatement until the retry branch has been hit
                exp, rej = uniform_stream(keys[t], sids[t], g.moduli[:nl], N)
                assert np.array_equal(got[t, 1], exp), t
                restated, rejected = restated + 1, rejected + rej
    assert rejected > 0, "no first-attempt rejection among the restated words: the retry branch went untested"
    # prefix property: a lower level is the first nl limbs of the same stream
    d_lo, d_hi = g.empty((1, 2, 3, N)), g.empty((1, 2, g.L, N))
    g.expand_seeded(d_lo, 1, 3, [keys[0]], [sids[0]])
    g.expand_seeded(d_hi, 1, g.L, [keys[0]], [sids[0]])
    assert np.array_equal(d_lo.to_host()[0, 1], d_hi.to_host()[0, 1, :3])
    # C3: 16 items, distinct keys and stream ids (more than one launch's worth is covered by 70 items at N = 2^12)
    g3 = ctxs(16, 10, 50, 60, 3)
    n, nl = 16, 12
    keys, sids = keys_of(rng, n), [int(x) for x in rng.choice(2 ** 32, n, replace=False)]
    d_ct = g3.empty((n, 2, nl, g3.N))
    g3.expand_seeded(d_ct, n, nl, keys, sids)
    got = d_ct.to_host()
    d_a = g3.empty((1, nl, g3.N))
    for t in range(n):
        g3.sample_uniform(d_a, 1, nl, 0, keys[t], sids[t])
        assert np.array_equal(got[t, 1], d_a.to_host()[0]), t
    n = 70
    keys, sids = keys_of(rng, n), list(range(1000, 1000 + n))
    d_ct = g.empty((n, 2, 2, N))
    g.expand_seeded(d_ct, n, 2, keys, sids)
    got = d_ct.to_host()
    d_a = g.empty((1, 2, N))
    for t in (0, 63, 64, 69):
        g.sample_uniform(d_a, 1, 2, 0, keys[t], sids[t])
        assert np.array_equal(got[t, 1], d_a.to_host()[0]), t


@pytest.mark.gpu
def test_encryption_is_bit_exact(ctxs):
    from oracle.oracle import OracleContext, sample_gauss, sample_ternary, sample_uniform
    rng = np.random.default_rng(12)
    g = ctxs(12, 10, 50, 60, 3)
    o = OracleContext(12, 10, 50, 60, dnum=3)
    N, nl, n = g.N, g.L, 3
    assert len(set(int(a) for a in g.arith[:nl])) >= 2  # limbs of both arithmetic classes
    _, sk = o.keygen(sample_ternary(rng, N), sample_uniform(rng, o.moduli, N), sample_gauss(rng, N))
    pt = np.stack([sample_uniform(rng, o.moduli[:nl], N) for _ in range(n)])
    e = np.stack([sample_gauss(rng, N) for _ in range(n)])
    seed, base = keys_of(rng, 1)[0], 5
    d_c0 = g.empty((n, nl, N))
    g.encrypt_seeded(g.to_device(sk), g.to_device(pt), g.to_device(e), d_c0, n, nl, seed, base)
    c0 = d_c0.to_host()
    d_a = g.empty((1, nl, N))
    for t in range(n):
        g.sample_uniform(d_a, 1, nl, 0, seed, base + t)
        a = d_a.to_host()[0]
        for i in range(nl):
            q = int(o.moduli[i])
            ee = o.ntt_fwd(i, np.array([int(x) % q for x in e[t]], dtype=np.uint64))
            exp = [(int(p) + int(x) - int(y) * int(s)) % q for p, x, y, s in zip(pt[t, i], ee, a[i], sk[i])]
            assert np.array_equal(c0[t, i], np.array(exp, dtype=np.uint64)), (t, i)
    # expanded and decrypted at the reference shape: the values within 2^-25
    g = ctxs(14, 2, 40, 60, 2)
    o = OracleContext(14, 2, 40, 60, dnum=2)
    N, nl = g.N, g.L
    _, sk = o.keygen(sample_ternary(rng, N), sample_uniform(rng, o.moduli, N), sample_gauss(rng, N))
    vals = rng.uniform(-0.5, 0.5, N // 2)
    scale = o.sf_big(0)
    pt = o.encode(vals, scale, nl)[None]
    d_c0 = g.empty((1, nl, N))
    g.encrypt_seeded(g.to_device(sk), g.to_device(pt), g.to_device(sample_gauss(rng, N)[None]), d_c0, 1, nl, seed, 9)
    d_ct = g.to_device(np.stack([d_c0.to_host()[0], np.zeros((nl, N), np.uint64)])[None])
    g.expand_seeded(d_ct, 1, nl, [seed], [9])
    dec = o.decrypt_decode(d_ct.to_host()[0], sk, scale)
    assert np.abs(dec - vals).max() < 2.0 ** -25


@pytest.fixture(scope="module")
def seeded_round(tmp_path_factory, ctxs):
    """4 clients at the reference shape (N = 2^14, L = 4): 0 and 2 seeded, 1 full, target 3 both ways; every seeded file
    also expanded in Python into full containers."""
    d = tmp_path_factory.mktemp("seeded")
    cc = _small_cc(d)
    rng = np.random.default_rng(13)
    g = ctxs(14, 2, 40, 60, 2)

    def ok(r):
        assert r.returncode == 0, r.stdout + r.stderr
        return r

    vals = [[("dense", rng.uniform(-0.3, 0.3, 2 * 8192 + 11)), ("bias", rng.uniform(-0.3, 0.3, 5)), ("empty", [])]
            for _ in range(4)]
    for c in range(4):
        ok(run("keyGen", cc, d / f"pk{c}", d / f"sk{c}"))
        w = _weights(d, f"w{c}.json", vals[c])
        ok(run("encryptModelWeights", cc, d / f"pk{c}", w, d / f"encF{c}.mkws"))
        ok(run("encryptModelWeights", cc, d / f"sk{c}", w, d / f"encS{c}.mkws", "--seeded"))
        expand_file(g, d / f"encS{c}.mkws", d / f"encX{c}.mkws")
        for tag in "FSX":
            mkws_to_json(d / f"enc{tag}{c}.mkws", d / f"enc{tag}{c}.json")
    for c in range(3):
        ok(run("REkeyGen", cc, d / f"sk{c}", d / "pk3", d / f"rk{c}"))
    ok(run("REkeyGen", cc, d / "sk3", d / "pk0", d / "rkback0"))
    return d, cc, vals, g


@pytest.mark.gpu
def test_seeded_files_have_the_documented_format(seeded_round):
    d, cc, vals, g = seeded_round
    N, L = g.N, g.L
    skel_s, blobs_s = read_mkws(d / "encS0.mkws")
    skel_f, blobs_f = read_mkws(d / "encF0.mkws")
    assert skel_s == skel_f and len(blobs_s) == len(blobs_f) == 2 + 3 + 2 + 1 + 2  # mean, std_dev, values per layer
    keys = set()
    for t, b in enumerate(blobs_s):
        assert len(b) == 48 + 40 + 8 * L * N
        h, key, sid, c0 = seeded_parts(b, N)
        hf = struct.unpack_from(HDR_FMT, blobs_f[t], 0)
        assert h[3:5] == hf[3:5] and h[6:] == hf[6:]  # ring_dim, limbs, level, noise_deg, scale, slots as a full ct
        assert sid == t and (c0 < g.moduli[:L, None]).all()
        keys.add(key)
    assert len(keys) == 1  # one key per file ...
    other = {seeded_parts(b, N)[1] for b in read_mkws(d / "encS1.mkws")[1]}
    assert other.isdisjoint(keys)  # ... drawn afresh for every file
    ok = run("encryptModelWeights", cc, d / "sk0", d / "w0.json", d / "again.mkws", "--seeded")
    assert ok.returncode == 0
    assert seeded_parts(read_mkws(d / "again.mkws")[1][0], N)[1] not in keys
    # decrypts to the weights
    r = run("decryptModelWeights", cc, d / "sk0", d / "encS0.mkws", d / "dec.json")
    assert r.returncode == 0, r.stderr
    dec = json.load(open(d / "dec.json"))["weights_summary"]
    for li in range(2):
        assert np.abs(np.array(dec[li]["values"]) - vals[0][li][1]).max() < 2.0 ** -25
    assert dec[2]["values"] == []
    # the JSON envelope of a seeded file decrypts to the same values
    r = run("decryptModelWeights", cc, d / "sk0", d / "encS0.json", d / "dec2.json")
    assert r.returncode == 0 and json.load(open(d / "dec2.json")) == json.load(open(d / "dec.json"))


@pytest.mark.gpu
def test_server_round_on_seeded_files_writes_the_bytes_of_the_expanded_ones(seeded_round):
    d, cc, vals, g = seeded_round

    def same(a, b):
        return open(d / a, "rb").read() == open(d / b, "rb").read()

    def round_args(out, back, tag3, tags=("S", "F", "S")):
        args = [d / out, "-", d / f"enc{tag3}3.mkws"]
        for c, t in enumerate(tags):
            args += [d / f"rk{c}", d / f"enc{t}{c}.mkws"]
        return args + ["--back", d / "rkback0", d / back]

    # reference: every input a full container (the seeded ones expanded in Python), synchronous path
    for tag3 in "SF":
        ref = round_args(f"aggX{tag3}.mkws", f"backX{tag3}.mkws", "X" if tag3 == "S" else "F", ("X", "F", "X"))
        r = run("serverRound", cc, *ref, env={"MKCKKS_SYNC_IO": "1"})
        assert r.returncode == 0, r.stdout + r.stderr
        for name, env in (("t1", {"MKCKKS_IO_THREADS": "1"}), ("t3", {"MKCKKS_IO_THREADS": "3"}),
                          ("sync", {"MKCKKS_SYNC_IO": "1"})):
            r = run("serverRound", cc, *round_args(f"agg{name}{tag3}.mkws", f"back{name}{tag3}.mkws", tag3), env=env)
            assert r.returncode == 0, r.stdout + r.stderr
            assert same(f"agg{name}{tag3}.mkws", f"aggX{tag3}.mkws"), (name, tag3)
            assert same(f"back{name}{tag3}.mkws", f"backX{tag3}.mkws"), (name, tag3)
            if name != "sync":
                line = [ln for ln in r.stdout.splitlines() if "[round] timing:" in ln][0]
                n_seeded = 30 if tag3 == "S" else 20  # 10 ciphertexts per client
                assert f"({n_seeded} seeded ciphertexts)" in line and " MiB " in line, line
    # several rounds in one process, seeded and full in turn
    rounds = d / "rounds.txt"
    rounds.write_text("\n".join(" ".join(map(str, round_args(f"r{k}{t}.mkws", f"r{k}{t}back.mkws", t)))
                                for k, t in enumerate("SFS")) + "\n")
    r = run("serverRound", cc, "--rounds", rounds, env={"MKCKKS_IO_THREADS": "3"})
    assert r.returncode == 0 and "[round] 3 rounds, " in r.stdout, r.stdout + r.stderr
    for k, t in enumerate("SFS"):
        assert same(f"r{k}{t}.mkws", f"aggX{t}.mkws") and same(f"r{k}{t}back.mkws", f"backX{t}.mkws"), k
    # the aggregate decrypts to the mean
    r = run("decryptModelWeights", cc, d / "sk3", d / "aggt3S.mkws", d / "dec.json")
    assert r.returncode == 0, r.stderr
    dec = json.load(open(d / "dec.json"))["weights_summary"]
    mean = np.mean([np.asarray(vals[c][0][1]) for c in range(4)], axis=0)
    assert np.abs(np.array(dec[0]["values"]) - mean).max() < 2.0 ** -25
    # every output is a full (kind 1) ciphertext
    for name in ("aggt3S.mkws", "backt3S.mkws"):
        assert all(struct.unpack_from(HDR_FMT, b, 0)[2] == KIND_CT for b in read_mkws(d / name)[1])


@pytest.mark.gpu
def test_per_client_programs_on_seeded_json_envelopes(seeded_round):
    d, cc, vals, g = seeded_round
    for tag in "SX":
        r = run("changeCipherDomain", cc, d / "rk0", d / f"enc{tag}0.json", d / f"pre{tag}0.json")
        assert r.returncode == 0, r.stderr
        r = run("aggregateEncryptedWeights", cc, d / f"enc{tag}3.json", d / f"pre{tag}0.json", d / f"agg{tag}.json",
                d / "encF1.json")
        assert r.returncode == 0, r.stderr
    assert open(d / "preS0.json").read() == open(d / "preX0.json").read()
    assert open(d / "aggS.json").read() == open(d / "aggX.json").read()
    blob = base64.b64decode(json.load(open(d / "preS0.json"))["weights_summary"][0]["mean"])
    assert struct.unpack_from(HDR_FMT, blob, 0)[2] == KIND_CT


@pytest.mark.gpu
def test_malformed_seeded_blobs_are_refused(seeded_round):
    d, cc, vals, g = seeded_round
    skel, blobs = read_mkws(d / "encS0.mkws")

    def tampered(name, fn):
        b = bytearray(blobs[0])
        b = fn(b)
        write_mkws(d / name, skel, [bytes(b)] + blobs[1:])
        return d / name

    def parts(b):
        b[20:24] = struct.pack("<I", 2)
        return b

    def pad(b):
        b[84:88] = struct.pack("<I", 1)
        return b

    def residue(b):
        b[88 + 8 * 5:88 + 8 * 6] = struct.pack("<Q", int(g.moduli[0]))
        return b

    cases = {"trunc.mkws": lambda b: b[:-8], "over.mkws": lambda b: b + b"\0" * 8, "parts.mkws": parts, "pad.mkws": pad,
             "residue.mkws": residue}
    for name, fn in cases.items():
        bad = tampered(name, fn)
        for env in ({"MKCKKS_SYNC_IO": "1"}, {"MKCKKS_IO_THREADS": "2"}):
            r = run("serverRound", cc, d / "x.mkws", d / "rk0", bad, "-", d / "encS3.mkws", env=env)
            assert r.returncode == 1 and "ERROR" in r.stderr, (name, env, r.stdout + r.stderr)
