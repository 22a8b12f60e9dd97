"""Collective key switching of the joint-key aggregate to a recipient's public key: mkckks_switch_share_batch, the fused
k_lift_col + k_kswitch_row pair, switchShare and fuseSwitchShares.

The reference is exact integer arithmetic built from the oracle as it stands: a party's share is exact_rerandomize applied to
the ciphertext (x, 0) with x = NTT(decrypt_core(prefix, c0 zeroed unless lead)) -- the composition the header names.

Noise rule (include/mkckks.h): n shares put n (sigma0^2 + h sigma1^2 + (2N/3) sigma_pk^2) of variance on every coefficient;
the decoded values carry sqrt(that N / 2) / scale.  The two tolerances on it are those of tests/test_threshold_decrypt.py,
same reasoning: the measured standard deviation over N/2 slots has a relative sampling error of 1 / sqrt(N) (1.6 % at
N = 2^12), so +-10 % is six of those; the largest of N/2 Gaussian values stays below 6 sd except with probability
N/2 * 2e-9.
"""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests.test_cli_hosts import BIN, _small_cc, run
from tests.test_compact_downlink import BOUND, PARAMS, _ok, _same_bytes, prefix
from tests.test_gpu_parity import CONFIGS, make_keys, rand_ct, rand_polys
from tests.test_rerandomize import exact_rerandomize, rand_pk, wide_errors
from tests.test_threshold_decrypt import key_chain, noise_sd, sum_mod, threshold_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "ppqsflhe_amd", "host")
SYMBOL = "mkckks_switch_share_batch"
EMAX = (1 << 62) - 1
SIGMA_STD = 3.19  # the scheme's error deviation (oracle.sample_gauss, the hosts' keyGen / encrypt)
N_PARTIES = 3
HDR = "<4sIIIIIIIdII"  # hostlib.hpp BlobHeader: magic, version, kind, ring, limbs, parts, level, noise_deg, scale, slots, reserved
KIND_CT, KIND_PK, KIND_KEYSHARE, KIND_SWITCH_SHARE = 1, 2, 7, 8


# ---- the exact reference ------------------------------------------------------------------------------------------------

def exact_switch_share(o, ct, sk, pk, v, e0, e1, nl, lead):
    """One party's key-switch share of ct [2][nl_in][N] at its first nl limbs: exact_rerandomize of (x, 0),
    x[i] = NTT_i(decrypt_core(prefix with c0 zeroed unless lead, sk)[i])."""
    pre = np.array(ct[:, :nl], dtype=np.uint64)
    if not lead:
        pre[0] = 0
    m = o.decrypt_core(pre, sk)
    x0 = np.zeros((2, nl, o.N), dtype=np.uint64)
    for i in range(nl):
        x0[0, i] = o.ntt_fwd(i, m[i])
    return exact_rerandomize(o, x0, pk, v, e0, e1, nl)


def rule_sd(n, N, scale, sigma0, h, sigma1=SIGMA_STD, sigma_pk=SIGMA_STD):
    """the header's noise rule, decoded"""
    return np.sqrt(n * (sigma0 ** 2 + h * sigma1 ** 2 + (2.0 * N / 3.0) * sigma_pk ** 2) * N / 2.0) / scale


# ---- CPU: surface and argument checks -----------------------------------------------------------------------------------

def test_switch_share_symbol_is_declared_bound_and_exported():
    from ppqsflhe_amd import Context, binding
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mkckks.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, hdr)
    assert SYMBOL in binding.SYMBOLS
    assert hasattr(binding.load_library(), SYMBOL)
    assert callable(getattr(Context, "switch_share", None))
    for prog in ("switchShare", "fuseSwitchShares"):
        assert os.access(os.path.join(BIN, prog), os.X_OK), prog


def test_switch_share_argument_checks_on_a_host_only_context():
    from ppqsflhe_amd import Context
    c = Context(12, 2, 40, 60, dnum=2, device=-1)
    f = getattr(c._L, SYMBOL)
    far = 1 << 40  # an output address far from the input's: pointers are never dereferenced
    W = 8 * c.N    # bytes of one limb polynomial
    try:
        L = c.L
        assert L >= 3
        # switch_share(ctx, ct, sk, pk, v, e0, e1, share, n_ct, nl_in, nl, lead)
        good = [8, 8, 8, 8, 8, 8, far]
        for lead in (0, 1):
            for i in range(7):
                args = list(good)
                args[i] = None
                assert f(c._h, *args, 1, L, L, lead) == -1, i
            assert f(None, *good, 1, L, L, lead) == -1
            assert f(c._h, *good, 1, L, 0, lead) == -1           # nl == 0
            assert f(c._h, *good, 1, 2, 3, lead) == -1           # nl > nl_in
            assert f(c._h, *good, 1, L + 1, 1, lead) == -1       # nl_in > L
            assert f(c._h, *good, 1, L + 1, L + 1, lead) == -1
            over = list(good)
            over[6] = 8
            assert f(c._h, *over, 1, L, L, lead) == -1                         # share over the ciphertext
            over[6] = 8 + (2 * L - 1) * W
            assert f(c._h, *over, 1, L, 1, lead) == -1                         # share starting inside its last limb
            assert f(c._h, far + W, 8, 8, 8, 8, 8, far, 2, L, 1, lead) == -1   # ciphertext starting inside the share
            over[6] = 8 + 2 * L * W
            assert f(c._h, *over, 1, L, L, lead) == -2                         # share right behind the ciphertext
            assert f(c._h, *good, 1, L, L, lead) == -2
            assert f(c._h, *good, 1, L, 1, lead) == -2
            assert f(c._h, *good, 0, L, L, lead) == 0
    finally:
        c.close()


# ---- CPU: the hosts' argument and file checks (no device is reached) ----------------------------------------------------

def blob(N, L, nl, lead, kind=KIND_SWITCH_SHARE, parts=2, fill=1, scale=2.0 ** 40, deg=2):
    """`lead`: the flags word of a share (1 lead, 2 rescale at the fusion)"""
    hdr = struct.pack(HDR, b"MKCK", 1, kind, N, nl, parts, L - nl, deg, scale, N // 2, int(lead))
    return hdr + np.full(parts * nl * N, fill, dtype=np.uint64).tobytes()


def envelope(path, b, layer="l"):
    """a JSON envelope with one layer: mean, std_dev and one values position, all holding `b`."""
    import base64
    b64 = base64.b64encode(b).decode()
    path.write_text(json.dumps({"weights_summary": [{"layer": layer, "shape": [3], "mean": b64, "std_dev": b64, "values": [b64]}]}))
    return path


def test_key_switch_command_line_errors(tmp_path):
    """Every misuse of switchShare and fuseSwitchShares: exit 1 with its [tag] ERROR line (or the usage line), nothing written."""
    from tests.test_cli_hosts import write_key_container
    cc = _small_cc(tmp_path)
    moduli = json.load(open(cc))["mkckks_cc"]["moduli"]
    N, L = 1 << 14, len(moduli)
    out = tmp_path / "out.json"
    sk, pk, agg = tmp_path / "sk", tmp_path / "pk", envelope(tmp_path / "agg.json", blob(N, L, L - 1, 0, kind=KIND_CT))
    sk.write_bytes(b"not read before the device\n")
    write_key_container(pk, KIND_PK, N, 1, 2, np.zeros(2 * N, dtype=np.uint64))
    sigma = tmp_path / "sigma1"  # a combined key share of party 1, 2-of-3
    sigma.write_bytes(struct.pack(HDR + "4I", b"MKCK", 1, KIND_KEYSHARE, N, L, 1, 0, 0, 0.0, 0, 0, 3, 2, 0, 1) +
                      np.ones(L * N, dtype=np.uint64).tobytes())
    dealt = tmp_path / "ks2.1"   # one dealer's share, not a combined one
    dealt.write_bytes(struct.pack(HDR + "4I", b"MKCK", 1, KIND_KEYSHARE, N, L, 1, 0, 0, 0.0, 0, 0, 3, 2, 2, 1) +
                      np.ones(L * N, dtype=np.uint64).tobytes())

    def refused(prog, args, *msgs):
        r = run(prog, *args)
        assert r.returncode == 1 and all(m in r.stderr for m in msgs), (prog, args, r.stdout + r.stderr)
        assert not os.path.exists(out), (prog, args)
        return r

    # wrong argc and malformed options: the usage line
    usage = "<cc_path> <privkey_path> <recipient_pubkey> <agg_encfile> <share_out> [--lead] [--smudge-bits <s>] [--parties i,j,...] [--limbs <m>]"
    for argv in ((), (cc,), (cc, sk, pk, agg), (cc, sk, pk, agg, out, "--limbs"), (cc, sk, pk, agg, out, "--lead", "--lead"),
                 (cc, sk, pk, agg, out, "--limbs", "1", "--limbs", "1"), (cc, sk, pk, agg, out, "--led"),
                 (cc, sk, pk, agg, out, "--parties"), (cc, sk, pk, agg, out, "--smudge-bits")):
        refused("switchShare", argv, "Usage:", usage)
    for bits in ("5", "57", "x"):
        refused("switchShare", (cc, sk, pk, agg, out, "--smudge-bits", bits), "[kswitch] ERROR: --smudge-bits needs an integer in [6, 56]")
    # --limbs 0, malformed, and above the aggregate's limbs
    for m in ("0", "x", "-1", "100"):
        refused("switchShare", (cc, sk, pk, agg, out, "--limbs", m), "[kswitch] ERROR: --limbs needs an integer in [1, the aggregate's limbs]")
    for m in (L, L + 1, 64):
        refused("switchShare", (cc, sk, pk, agg, out, "--limbs", m),
                f"[kswitch] ERROR: --limbs {m} exceeds the aggregate's {L - 1} limb(s)")
    agg1 = envelope(tmp_path / "agg1.json", blob(N, L, L - 1, 0, kind=KIND_CT, deg=1))  # nothing left to rescale
    refused("switchShare", (cc, sk, pk, agg1, out, "--limbs", 1), "[kswitch] ERROR: --limbs 1 needs input at noiseScaleDeg 2")
    # missing files and files of another kind
    refused("switchShare", (tmp_path / "nocc", sk, pk, agg, out), "[kswitch] ERROR: Failed to load CryptoContext from")
    refused("switchShare", (cc, tmp_path / "nosk", pk, agg, out), "[kswitch] ERROR: Failed to load private key from")
    for bad in (tmp_path / "nopk", sk, cc, sigma):
        refused("switchShare", (cc, sk, bad, agg, out), f"[kswitch] ERROR: Failed to load public key from {bad}")
    refused("switchShare", (cc, sk, pk, tmp_path / "noagg", out), "[kswitch] ERROR: Could not open input file:")
    share = envelope(tmp_path / "share.json", blob(N, L, L - 1, 1))
    refused("switchShare", (cc, sk, pk, share, out), "[kswitch] ERROR: not a mkckks ciphertext blob")
    # --parties misuse: partialDecrypt's usage errors
    for args, msg in (((sigma, pk, agg, out), "a key share needs --parties"),
                      ((sigma, pk, agg, out, "--lead"), "a key share needs --parties"),
                      ((sk, pk, agg, out, "--parties", "1,3"), "--parties needs a combined key share"),
                      ((sigma, pk, agg, out, "--parties", "1"), "fewer parties than the threshold"),
                      ((sigma, pk, agg, out, "--parties", "2,3"), "does not name the key share's own party"),
                      ((sigma, pk, agg, out, "--parties", "1,4"), "above the share's n_parties"),
                      ((sigma, pk, agg, out, "--parties", "1,1"), "--parties needs distinct party indices"),
                      ((sigma, pk, agg, out, "--parties", "1,x"), "--parties needs distinct party indices"),
                      ((dealt, pk, agg, out, "--parties", "1,2"), "the key share is one dealer's")):
        refused("switchShare", (cc,) + args, "[kswitch] ERROR: ", msg)
    # fuseSwitchShares
    files = {
        "lead": envelope(tmp_path / "lead.json", blob(N, L, L - 1, True)),
        "lead2": envelope(tmp_path / "lead2.json", blob(N, L, L - 1, True)),
        "main": envelope(tmp_path / "main.json", blob(N, L, L - 1, False)),
        "main2": envelope(tmp_path / "main2.json", blob(N, L, L - 1, False)),
        "low": envelope(tmp_path / "low.json", blob(N, L, L - 2, False)),
        "resc": envelope(tmp_path / "resc.json", blob(N, L, L - 1, 2)),
        "flags": envelope(tmp_path / "flags.json", blob(N, L, L - 1, 4)),
        "resc1": envelope(tmp_path / "resc1.json", blob(N, L, L - 1, 2, deg=1)),
        "scale": envelope(tmp_path / "scale.json", blob(N, L, L - 1, False, scale=2.0 ** 41)),
        "layer": envelope(tmp_path / "layer.json", blob(N, L, L - 1, False), layer="other"),
        "ct": envelope(tmp_path / "ct.json", blob(N, L, L - 1, 0, kind=KIND_CT)),
        "dshare": envelope(tmp_path / "dshare.json", blob(N, L, L - 1, 0, kind=6, parts=1)),
        "cut": envelope(tmp_path / "cut.json", blob(N, L, L - 1, False)[:-8]),
        "level": envelope(tmp_path / "level.json", blob(N, L + 1, L - 1, False)),
    }
    for names, msg in ((("main", "main2"), "[fuse] ERROR: need exactly one lead share per ciphertext (position 0 has 0)"),
                       (("main",), "[fuse] ERROR: need exactly one lead share per ciphertext (position 0 has 0)"),
                       (("lead", "main", "lead2"), "[fuse] ERROR: need exactly one lead share per ciphertext (position 0 has 2)"),
                       (("lead", "low"), "shares differ in layers, shapes, limbs, levels or scales"),
                       (("low", "lead"), "shares differ in layers, shapes, limbs, levels or scales"),
                       (("lead", "scale"), "shares differ in layers, shapes, limbs, levels or scales"),
                       (("lead", "resc"), "shares differ in layers, shapes, limbs, levels or scales"),
                       (("lead", "flags"), "key-switch share: unknown flag bits"),
                       (("lead", "resc1"), "the rescale flag needs noiseScaleDeg 2"),
                       (("lead", "layer"), "shares differ in layers, shapes, limbs, levels or scales"),
                       (("lead", "ct"), "not a mkckks key-switch share blob"),
                       (("ct", "main"), "not a mkckks key-switch share blob"),
                       (("lead", "dshare"), "not a mkckks key-switch share blob"),
                       (("lead", "cut"), "key-switch share blob has the wrong size"),
                       (("lead", "level"), "level does not match its limb count")):
        refused("fuseSwitchShares", (cc, *(files[n] for n in names), out), "[fuse] ERROR: ", msg)
    refused("fuseSwitchShares", (cc, files["lead"], tmp_path / "nofile.json", out), "[fuse] ERROR: Could not open share file")
    refused("fuseSwitchShares", (tmp_path / "nocc", files["lead"], out), "[fuse] ERROR: Failed to load CryptoContext from")
    for argv in ((), (cc,), (cc, out)):
        refused("fuseSwitchShares", argv, "Usage:")
    assert not [p for p in os.listdir(tmp_path) if p.startswith("out")]


def test_switchshare_selftest_plain_and_under_asan_ubsan():
    """The key-switch share parser on truncated, oversized, wrong-kind, wrong-ring and non-canonical blobs: a stand-alone
    program, plain and under AddressSanitizer + UBSan.  A sanitizer report aborts the process (non-zero exit)."""
    r = subprocess.run(["make", "-C", HOST, "-s", "build/switchshare_selftest", "switchshare-asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
    for exe in (os.path.join(BIN, "switchshare_selftest"), os.path.join(BIN, "asan", "switchshare_selftest")):
        r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, (exe, r.stdout[-2000:] + r.stderr[-2000:])
        assert "ok switchshare selftest" in r.stdout and "FAIL" not in r.stderr, exe
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, exe
        for case in ("truncated payload", "oversized by one byte", "ciphertext blob", "decryption share blob", "wrong ring",
                     "2^32 - 1 limbs", "non-canonical word", "parse_limbs", "rescale flag round trip", "flag bits 4",
                     "rescale at degree 1", "rescale of one limb"):
            assert f"ok {case}" in r.stdout, (exe, case)


# ---- CPU: the protocol on the oracle alone ------------------------------------------------------------------------------

_RECIPIENTS = {}


def recipient(name):
    """a stand-alone key pair outside the chain: (ternary s, pk, sk); computed once per parameter set."""
    if name not in _RECIPIENTS:
        o = threshold_chain(name)["o"]
        s, a, e = make_keys(o, np.random.default_rng(61))
        _RECIPIENTS[name] = (s,) + tuple(o.keygen(s, a, e))
    return _RECIPIENTS[name]


def oracle_masks(rng, N, sigma0, n=N_PARTIES):
    from oracle.oracle import sample_gauss, sample_ternary
    return [(sample_ternary(rng, N), np.zeros(N, dtype=np.int64) if sigma0 == 0 else wide_errors(rng, N, sigma0),
             sample_gauss(rng, N).astype(np.int64)) for _ in range(n)]


@pytest.mark.parametrize("name", ["p12", "p14"])
def test_oracle_key_switch_protocol(name):
    ch = threshold_chain(name)
    o, agg, scale, sks, mean = ch["o"], ch["agg"], ch["scale"], ch["sks"], ch["mean"]
    s_r, pk_r, sk_r = recipient(name)
    N, nl = o.N, agg.shape[1]
    h = int(np.count_nonzero(s_r))
    # zero smudging: three shares sum to a ciphertext under the recipient's key that decodes to the mean
    masks = oracle_masks(np.random.default_rng(600), N, 0)
    shares = [exact_switch_share(o, agg, sks[p], pk_r, *masks[p], nl, p == 0) for p in range(N_PARTIES)]
    fused = sum_mod(o, shares)
    err0 = np.abs(o.decrypt_decode(fused, sk_r, scale) - mean).max()
    print(f"{name}: zero-smudging error 2^{np.log2(err0):.2f}")
    assert err0 < BOUND[name], (name, err0)
    # component 1 carries no trace of the aggregate: it is the encryption of zero's own
    zero_ct = np.zeros_like(agg)
    for p in range(N_PARTIES):
        assert np.array_equal(shares[p][1], exact_switch_share(o, zero_ct, sks[p], pk_r, *masks[p], nl, p == 0)[1])
    # no party's key, nor the joint secret, opens the delivered ciphertext; any two shares are garbage
    for key in sks + [ch["sk_sum"]]:
        assert np.abs(o.decrypt_decode(fused, key, scale) - mean).max() > 1
    for pair in ((0, 1), (0, 2), (1, 2)):
        assert np.abs(o.decrypt_decode(sum_mod(o, [shares[p] for p in pair]), sk_r, scale) - mean).max() > 1, pair
    # sigma0 = 2^20 on a degree-1 cut of the aggregate (Rescale: one limb fewer, scale / q_last ~ sf of that level), where
    # the smudging is visible in the decoded values
    cut, scale1 = o.rescale(agg), scale / float(o.moduli[nl - 1])
    nl1 = nl - 1
    rng = np.random.default_rng(601)
    clean = oracle_masks(rng, N, 0)
    sigma0 = 2.0 ** 20
    smudge = [wide_errors(rng, N, sigma0) for _ in range(N_PARTIES)]
    dec = []
    for with_smudge in (False, True):
        sh = [exact_switch_share(o, cut, sks[p], pk_r, clean[p][0], smudge[p] if with_smudge else clean[p][1], clean[p][2],
                                 nl1, p == 0) for p in range(N_PARTIES)]
        dec.append(o.decrypt_decode(sum_mod(o, sh), sk_r, scale1))
    err1 = np.abs(dec[0] - mean).max()
    noise = dec[1] - dec[0]
    sd = rule_sd(N_PARTIES, N, scale1, sigma0, h)
    ratio = noise.std() / sd
    err = np.abs(dec[1] - mean).max()
    print(f"{name} sigma0 2^20 at scale 2^{np.log2(scale1):.2f}: sd 2^{np.log2(sd):.2f}, measured / rule {ratio:.4f}, largest / sd "
          f"{np.abs(noise).max() / sd:.2f}, error 2^{np.log2(err):.2f}, zero-smudging error 2^{np.log2(err1):.2f}")
    assert abs(sd / noise_sd(sigma0, N_PARTIES, N, scale1) - 1) < 1e-3  # partial_decrypt's rule to within 10^-3
    assert 0.9 < ratio < 1.1, (name, ratio)
    assert err < err1 + 6 * sd, (name, err, err1, sd)


@pytest.mark.parametrize("name,m", [("p14", 1), ("p14", 2), ("p12", 1)])
def test_oracle_key_switch_compaction(name, m):
    """switchShare --limbs m on the oracle: shares at the m + 1-limb prefix with sigma0 = 2^20, summed, THEN rescaled to m limbs
    -- within the compact bound under the recipient's key.  The other order is what must not be built: a share rescaled by
    its party loses its smudging (2^20 / q_m rounds to nothing)."""
    ch = threshold_chain(name)
    o, agg, scale, sks, mean = ch["o"], ch["agg"], ch["scale"], ch["sks"], ch["mean"]
    _, pk_r, sk_r = recipient(name)
    masks = oracle_masks(np.random.default_rng(602 + m), o.N, 2.0 ** 20)
    shares = [exact_switch_share(o, agg, sks[p], pk_r, *masks[p], m + 1, p == 0) for p in range(N_PARTIES)]
    small = o.rescale(sum_mod(o, shares))
    assert small.shape == (2, m, o.N)
    err = np.abs(o.decrypt_decode(small, sk_r, scale / float(o.moduli[m])) - mean).max()
    print(f"{name} --limbs {m}: error 2^{np.log2(err):.2f}, bound 2^{np.log2(16 * BOUND[name]):.2f}")
    assert err < 16 * BOUND[name], (name, m, err)
    q = int(o.moduli[m])
    assert np.abs(masks[0][1]).max() * 2 < q  # every smudging word is below q_m / 2: Rescale of a single share rounds it to 0


def test_oracle_key_share_linearity():
    """n = 5, t = 3, identical (v, e0, e1) per party POSITION: the shares made with lambda_j sigma_j over any set T of three
    sum, word for word, to the sum made with three keys whose sum is sum s_i."""
    from tests.test_key_sharing import lagrange, scale_ref, shamir_ref, wsum_ref
    ch = threshold_chain("p14")
    o, agg, pk_r = ch["o"], ch["agg"], recipient("p14")[1]
    N, L, nl, n, t = o.N, o.L, agg.shape[1], 5, 3
    moduli = [int(q) for q in o.moduli[:L]]
    rng = np.random.default_rng(92)
    sks = [k[2] for k in key_chain(o, rng, n)]
    dealt = [shamir_ref(sks[i][:L], [np.stack([rng.integers(0, q, size=N, dtype=np.uint64) for q in moduli]) for _ in range(t - 1)],
                        moduli, n) for i in range(n)]
    sigma = []
    for j in range(n):
        s = np.zeros((o.D, N), dtype=np.uint64)
        s[:L] = wsum_ref(np.stack([dealt[i][j] for i in range(n)]), np.ones((n, L), dtype=np.uint64), moduli)
        sigma.append(s)
    masks = oracle_masks(rng, N, 2.0 ** 20, t)

    def fused(keys):
        return sum_mod(o, [exact_switch_share(o, agg, keys[a], pk_r, *masks[a], nl, a == 0) for a in range(t)])

    # three keys that sum to sum s_i: (s_1 + s_2, s_3 + s_4, s_5)
    want = fused([sum_mod(o, [sks[0][None], sks[1][None]])[0], sum_mod(o, [sks[2][None], sks[3][None]])[0], sks[4]])
    for T in ((1, 2, 3), (1, 3, 5), (2, 4, 5), (3, 4, 5)):
        keys = [scale_ref(sigma[j - 1], [lagrange(T, j, q) for q in moduli], moduli) for j in T]
        assert np.array_equal(fused(keys), want), T
    keys = [scale_ref(sigma[j - 1], [lagrange((1, 2), j, q) for q in moduli], moduli) for j in (1, 2)] + [np.zeros_like(sigma[0])]
    assert not np.array_equal(fused(keys), want)  # below the threshold


# ---- GPU ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctxs():
    from oracle.oracle import OracleContext
    from ppqsflhe_amd import Context
    cache = {}

    def get(name):
        if name not in cache:
            a = CONFIGS[name] if name in CONFIGS else PARAMS[name]
            cache[name] = (Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0),
                           OracleContext(a[0], a[1], a[2], a[3], dnum=a[4]))
        return cache[name]

    yield get
    for g, _ in cache.values():
        g.close()


def rand_sk(rng, g):
    return rand_polys(rng, g, list(range(g.D)), 1)[0]


def switch_share(g, ct, sk, pk, v, e0, e1, nl, lead):
    d = g.switch_share(g.to_device(ct), g.to_device(sk), g.to_device(pk), g.to_device(v, np.int8), g.to_device(e0, np.int64),
                       g.to_device(e1, np.int64), nl, lead)
    assert d.shape == (ct.shape[0], 2, nl, g.N)
    return d.to_host()


def wide_inputs(rng, g, nl_in, B, signs=(1, -1)):
    """e uniform in +-2^59 with +-(2^62 - 1), 0 and +-1 planted; v all +1 (item 0), all -1 (item 1), ternary after that."""
    from oracle.oracle import sample_ternary
    v = np.stack([np.full(g.N, signs[b], dtype=np.int8) if b < len(signs) else sample_ternary(rng, g.N) for b in range(B)])
    e0 = rng.integers(-2 ** 59, 2 ** 59, size=(B, g.N), dtype=np.int64)
    e1 = rng.integers(-2 ** 59, 2 ** 59, size=(B, g.N), dtype=np.int64)
    plant = np.array([EMAX, -EMAX, 0, 1, -1], dtype=np.int64)
    e0[:, :5], e1[:, -5:] = plant, plant[::-1]
    e0[:, g.N // 2 + 3], e1[:, g.N // 2 - 3] = -EMAX, EMAX
    return rand_ct(rng, g, nl_in, B), rand_sk(rng, g), rand_pk(rng, g), v, e0, e1


def check_exact(g, o, ct, sk, pk, v, e0, e1, nl, lead, tag):
    got = switch_share(g, ct, sk, pk, v, e0, e1, nl, lead)
    for b in range(ct.shape[0]):
        assert np.array_equal(got[b], exact_switch_share(o, ct[b], sk, pk, v[b], e0[b], e1[b], nl, lead)), (tag, lead, b)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("lead", [0, 1])
@pytest.mark.parametrize("name,nl_in,nl,B", [("c1", 2, 2, 3), ("ref", 4, 3, 3), ("ref", 4, 1, 2), ("c3", 12, 11, 1), ("n11", 4, 3, 2)])
def test_switch_share_matches_the_exact_reference(ctxs, name, nl_in, nl, B, lead):
    """The smallest shapes that reach every instance: ROW_H 2 (c1), ROW_H 3 and a prefix (ref), one limb, 256-point rows with
    fp64 and pseudo-Mersenne limbs (c3), the generic path (n11)."""
    from oracle.oracle import sample_ternary
    g, o = ctxs(name)
    rng = np.random.default_rng(800 + 17 * nl_in + nl + B)
    v = np.stack([sample_ternary(rng, g.N) for _ in range(B)])
    e0 = rng.integers(-2 ** 40, 2 ** 40, size=(B, g.N), dtype=np.int64)
    e1 = rng.integers(-20, 21, size=(B, g.N), dtype=np.int64)
    check_exact(g, o, rand_ct(rng, g, nl_in, B), rand_sk(rng, g), rand_pk(rng, g), v, e0, e1, nl, lead, (name, nl_in, nl))


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl,B", [("c1", 2, 3), ("ref", 4, 3), ("n11", 4, 3), ("c3", 12, 1)])
def test_switch_share_wide_errors_are_exact(ctxs, name, nl, B):
    """62-bit errors against exact integers (the fp64-class limbs hold 53 bits: the lift must not go through them)."""
    g, o = ctxs(name)
    rng = np.random.default_rng(950 + nl)
    for signs in ((1, -1),) if B > 1 else ((1,), (-1,)):
        ct, sk, pk, v, e0, e1 = wide_inputs(rng, g, nl, B, signs)
        for lead in (0, 1):
            check_exact(g, o, ct, sk, pk, v, e0, e1, nl, lead, (name, signs))


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl", [("c3", 12), ("ref", 4)])
def test_switch_share_extreme_residues(ctxs, name, nl):
    """ct, sk and pk with every word at q_i - 1 (item 0) and alternating 0 / q_i - 1 (item 1, the key and the public key
    alternate in both items' second run), every |e| at 2^62 - 1: the largest c1 s + c0 + b V + E0."""
    g, o = ctxs(name)
    B, N = 2, g.N
    alt = (np.arange(N) % 2).astype(np.uint64)
    v = np.stack([np.full(N, 1, dtype=np.int8), np.full(N, -1, dtype=np.int8)])
    e0 = np.stack([np.full(N, EMAX, dtype=np.int64), np.full(N, -EMAX, dtype=np.int64)])
    e1 = -e0
    for keys_alternate in (False, True):
        ct = np.empty((B, 2, nl, N), dtype=np.uint64)
        sk = np.empty((g.D, N), dtype=np.uint64)
        pk = np.empty((2, g.D, N), dtype=np.uint64)
        for l in range(nl):
            q1 = np.uint64(int(g.moduli[l]) - 1)
            ct[0, :, l] = q1
            ct[1, :, l] = q1 * alt
        for l in range(g.D):
            q1 = np.uint64(int(g.moduli[l]) - 1)
            sk[l] = q1 * (alt if keys_alternate else np.uint64(1))
            pk[:, l] = q1 * ((np.uint64(1) - alt) if keys_alternate else np.uint64(1))
        for lead in (0, 1):
            check_exact(g, o, ct, sk, pk, v, e0, e1, nl, lead, (name, keys_alternate))


def composition(g, ct, sk, pk, v, e0, e1, nl, lead):
    """the header's three calls: partial_decrypt(e = 0) -> ntt_forward -> rerandomize on (that, 0)."""
    B, nl_in, N = ct.shape[0], ct.shape[2], g.N
    d_x = g.empty((B, nl, N))
    g.partial_decrypt(g.to_device(ct), g.to_device(sk), g.to_device(np.zeros((B, N), dtype=np.int64)), d_x, B, nl_in, nl, lead)
    g.ntt_forward(d_x, B, nl)
    x0 = np.zeros((B, 2, nl, N), dtype=np.uint64)
    x0[:, 0] = d_x.to_host().reshape(B, nl, N)
    d_ct = g.to_device(x0)
    g.rerandomize(d_ct, g.to_device(pk), g.to_device(v, np.int8), g.to_device(e0, np.int64), g.to_device(e1, np.int64), d_ct,
                  B, nl, nl)
    return d_ct.to_host()


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl_in,nl,B", [("ref", 4, 3, 3), ("c3", 12, 11, 2)])
def test_switch_share_equals_the_composition_of_the_entry_points(ctxs, name, nl_in, nl, B):
    g, _ = ctxs(name)
    rng = np.random.default_rng(33 + nl)
    ct, sk, pk, v, e0, e1 = wide_inputs(rng, g, nl_in, B)
    for lead in (0, 1):
        assert np.array_equal(switch_share(g, ct, sk, pk, v, e0, e1, nl, lead), composition(g, ct, sk, pk, v, e0, e1, nl, lead)), lead


@pytest.mark.gpu
@pytest.mark.parametrize("name,nl", [("c3", 12), ("ref", 4)])
@pytest.mark.parametrize("env", [{"MKCKKS_GENERIC_NTT": "1"}, {"MKCKKS_NO_FP64": "1"}, {"MKCKKS_NO_PM": "1"}, {"MKCKKS_CHUNK": "1"}])
def test_switch_share_under_the_library_switches(ctxs, monkeypatch, env, name, nl):
    """Switches are read once, when a context is created: a fresh context under each must give the same bits."""
    from ppqsflhe_amd import Context
    _, o = ctxs(name)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    a = CONFIGS[name]
    g = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)
    try:
        rng = np.random.default_rng(45 + nl)
        ct, sk, pk, v, e0, e1 = wide_inputs(rng, g, nl, 2)
        for lead in (0, 1):
            check_exact(g, o, ct, sk, pk, v, e0, e1, nl, lead, (name, env))
    finally:
        g.close()


@pytest.mark.gpu
def test_switch_share_call_properties(ctxs):
    """A share over the ciphertexts is refused; inputs are not written; a poisoned tail after the output stays intact; an
    empty call writes nothing; a batch larger than one workspace chunk (MKCKKS_CHUNK = 16) equals per-chunk calls; rerandomize
    and partial_decrypt give what they gave before the call."""
    from ppqsflhe_amd.binding import MkckksError
    from tests.test_rerandomize import rerandomize
    from tests.test_threshold_decrypt import partial_decrypt
    g, o = ctxs("c3")
    rng = np.random.default_rng(79)
    nl_in, B, N = 11, 2, g.N
    ct, sk, pk, v, e0, e1 = wide_inputs(rng, g, nl_in, B)
    rr_before, pd_before = rerandomize(g, ct, pk, v, e0, e1, nl_in), partial_decrypt(g, ct, sk, e0, nl_in, 1)
    full = switch_share(g, ct, sk, pk, v, e0, e1, nl_in, 1)
    d_ct, d_sk, d_pk = g.to_device(ct), g.to_device(sk), g.to_device(pk)
    d_v, d_e0, d_e1 = g.to_device(v, np.int8), g.to_device(e0, np.int64), g.to_device(e1, np.int64)
    POISON = 0xA5A5A5A5A5A5A5A5
    for nl in (2, 5):
        words, pad = B * 2 * nl * N, 2 * N
        d_big = g.to_device(np.full(words + pad, POISON, dtype=np.uint64))
        d_out = d_big.view(0, (B, 2, nl, N))
        assert g.switch_share(d_ct, d_sk, d_pk, d_v, d_e0, d_e1, nl, True, out=d_out) is d_out
        strided = d_out.to_host()
        assert np.all(d_big.to_host()[words:] == POISON)
        assert np.array_equal(strided, switch_share(g, prefix(ct, nl), sk, pk, v, e0, e1, nl, 1)), nl
        assert np.array_equal(strided, full[:, :, :nl]), nl  # limb by limb the same arithmetic
        d_out.upload(np.full(strided.shape, POISON, dtype=np.uint64))
        g.switch_share(d_ct.view(0, (0, 2, nl_in, N)), d_sk, d_pk, d_v, d_e0, d_e1, nl, True, out=d_out)
        assert np.all(d_out.to_host() == POISON)
    for call in (lambda: g.switch_share(d_ct, d_sk, d_pk, d_v, d_e0, d_e1, 2, True, out=d_ct),
                 lambda: g.switch_share(d_ct, d_sk, d_pk, d_v, d_e0, d_e1, nl_in, False, out=d_ct),
                 lambda: g.switch_share(d_ct, d_sk, d_pk, d_v, d_e0, d_e1, nl_in, False, out=d_ct.view(N, (N,)))):
        with pytest.raises(MkckksError) as ei:
            call()
        assert ei.value.code == -1
    assert np.array_equal(d_ct.to_host(), ct) and np.array_equal(d_sk.to_host(), sk) and np.array_equal(d_pk.to_host(), pk)
    assert np.array_equal(d_v.to_host(), v) and np.array_equal(d_e0.to_host(), e0) and np.array_equal(d_e1.to_host(), e1)
    assert np.array_equal(rerandomize(g, ct, pk, v, e0, e1, nl_in), rr_before)
    assert np.array_equal(partial_decrypt(g, ct, sk, e0, nl_in, 1), pd_before)
    # more ciphertexts than one chunk, on the small ring: one call = the calls chunk by chunk = the exact reference
    g2, o2 = ctxs("ref")
    B2, nl2 = 19, 3
    ct, sk, pk, v, e0, e1 = wide_inputs(rng, g2, nl2, B2)
    for lead in (0, 1):
        got = check_exact(g2, o2, ct, sk, pk, v, e0, e1, nl2, lead, "19")
        parts = [switch_share(g2, ct[a:b], sk, pk, v[a:b], e0[a:b], e1[a:b], nl2, lead) for a, b in ((0, 16), (16, 19))]
        assert np.array_equal(got, np.concatenate(parts)), lead


def device_masks(g, key, base, sigma0):
    """(v, e0, e1) of one ciphertext from streams base .. base + 2: e1 at the wide sampler's smallest sigma, 2^6."""
    N = g.N
    d_v, d_e0, d_e1 = g.empty((1, N), np.int8), g.empty((1, N), np.int64), g.empty((1, N), np.int64)
    g.sample_ternary(d_v, N, key, base)
    g.sample_gauss_wide(d_e0, N, sigma0, key, base + 1)
    g.sample_gauss_wide(d_e1, N, 2.0 ** 6, key, base + 2)
    return d_v, d_e0, d_e1


def deliver(g, d_shares, n, d_sk_r, nl, scale):
    """eval_sum -> decrypt under the recipient's key -> decode"""
    N = g.N
    d_ct, d_m, d_vals = g.empty((1, 2, nl, N)), g.empty((1, nl, N)), g.empty((1, N // 2), dtype=np.float64)
    g.eval_sum(d_shares, d_ct, n, 1, nl)
    g.decrypt(d_ct, d_sk_r, d_m, 1, nl)
    g.decode(d_m, d_vals, 1, nl, scale)
    return d_ct.to_host(), d_vals.to_host().reshape(N // 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["p14", "p12"])
def test_key_switch_on_the_device(ctxs, name):
    """The chain of the CPU test, three parties, device-drawn randomness (sigma0 = 2^20): switch_share x 3 -> eval_sum ->
    decrypt under the recipient's key -> decode, within BOUND (at the aggregate's scale ~ 2^(2p) the smudging is far
    below it); every share equals the exact reference on the drawn randomness."""
    g, o = ctxs(name)
    ch = threshold_chain(name)
    agg, scale, sks, mean = ch["agg"], ch["scale"], ch["sks"], ch["mean"]
    _, pk_r, sk_r = recipient(name)
    nl, N = agg.shape[1], g.N
    d_agg, d_pk, d_sk_r = g.to_device(agg[None]), g.to_device(pk_r), g.to_device(sk_r)
    key = np.random.default_rng(5).bytes(32)
    d_shares = g.empty((N_PARTIES, 1, 2, nl, N))
    for p in range(N_PARTIES):
        d_v, d_e0, d_e1 = device_masks(g, key, 3 * p, 2.0 ** 20)
        out = d_shares.view(p * 2 * nl * N, (1, 2, nl, N))
        g.switch_share(d_agg, g.to_device(sks[p]), d_pk, d_v, d_e0, d_e1, nl, p == 0, out=out)
        exp = exact_switch_share(o, agg, sks[p], pk_r, d_v.to_host()[0], d_e0.to_host()[0], d_e1.to_host()[0], nl, p == 0)
        assert np.array_equal(out.to_host()[0], exp), (name, p)
    fused, vals = deliver(g, d_shares, N_PARTIES, d_sk_r, nl, scale)
    assert np.array_equal(fused[0], sum_mod(o, list(d_shares.to_host()[:, 0])))
    err = np.abs(vals - mean).max()
    print(f"{name}: error 2^{np.log2(err):.2f}, bound 2^{np.log2(BOUND[name]):.2f}")
    assert err < BOUND[name], (name, err)
    assert g.count_noncanonical(d_shares, N_PARTIES, nl) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["p14", "p12"])
def test_key_switch_with_key_shares_on_the_device(ctxs, name):
    """n = 5, t = 3 on the device: keygen / keygen_join, share_key, combine_key_shares; an aggregate-like ciphertext under the
    joint key.  With identical randomness per party position the fused ciphertext is the same words for every 3-subset,
    and decodes within BOUND under the recipient's key; 2 of 5 do not decode."""
    import itertools
    from oracle.oracle import sample_gauss, sample_ternary
    g, o = ctxs(name)
    rng = np.random.default_rng(405)
    N, L, D, n, t = g.N, g.L, g.D, 5, 3
    d_pk, sks = None, []
    for p in range(n):
        d_new, d_sk = g.empty((2, D, N)), g.empty((D, N))
        d_s, d_e = g.to_device(sample_ternary(rng, N)), g.to_device(sample_gauss(rng, N))
        if p == 0:
            g.keygen(d_s, g.to_device(rand_sk(rng, g)), d_e, d_new, d_sk)
        else:
            g.keygen_join(d_pk, d_s, d_e, d_new, d_sk)
        d_pk = d_new
        sks.append(d_sk)
    d_dealt = g.empty((n, n, L, N))
    for i in range(n):
        g.share_key(sks[i], d_dealt.view(i * n * L * N, (n, L, N)), L, n, t, rng.bytes(32), 0)
    dealt = d_dealt.to_host()
    sigma = []
    for j in range(n):
        d_in = g.to_device(np.ascontiguousarray(dealt[:, j]))
        g.combine_key_shares(d_in, np.ones((n, L), dtype=np.uint64), d_in, n, L)
        sigma.append(d_in.view(0, (L, N)))
    _, pk_r, sk_r = recipient(name)
    d_pk_r, d_sk_r = g.to_device(pk_r), g.to_device(sk_r)
    vals = rng.uniform(-0.3, 0.3, size=(1, N // 2))
    scale = g.sf_big(0)
    d_pt, d_ct = g.empty((1, L, N)), g.empty((1, 2, L, N))
    g.encode(g.to_device(vals), d_pt, 1, L, scale)
    g.encrypt(d_pk, d_pt, g.to_device(sample_ternary(rng, N)[None]), g.to_device(sample_gauss(rng, N)[None]),
              g.to_device(sample_gauss(rng, N)[None]), d_ct, 1, L)
    key = rng.bytes(32)
    masks = [device_masks(g, key, 3 * a, 2.0 ** 20) for a in range(t)]

    def round_of(T):
        lam = g.lagrange_at_zero(T)
        d_shares = g.empty((len(T), 1, 2, L, N))
        for a, j in enumerate(T):
            d_key = g.empty((L, N))
            g.combine_key_shares(sigma[j - 1], lam[a:a + 1], d_key, 1, L)  # lambda_j sigma_j, u64[L][N]
            g.switch_share(d_ct, d_key, d_pk_r, *masks[a], L, a == 0, out=d_shares.view(a * 2 * L * N, (1, 2, L, N)))
        return deliver(g, d_shares, len(T), d_sk_r, L, scale)

    first = None
    for T in itertools.combinations(range(1, n + 1), t):
        fused, dec = round_of(T)
        if first is None:
            first = fused
            err = np.abs(dec - vals[0]).max()
            print(f"{name}: error 2^{np.log2(err):.2f}")
            assert err < BOUND[name], (name, err)
        assert np.array_equal(fused, first), (name, T)
    _, dec2 = round_of((1, 2))
    assert np.abs(dec2 - vals[0]).max() > 1, name


# ---- GPU: through the binaries ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cli_round(tmp_path_factory):
    """N = 2^14, MKWS: a key chain of 3 and a stand-alone recipient; three uploads under the joint key; serverRound."""
    from tests.test_cli_hosts import _weights
    tmp, ext = tmp_path_factory.mktemp("kswitch"), "mkws"
    cc = _small_cc(tmp)
    rng = np.random.default_rng(810)
    vals = [[("dense", rng.uniform(-0.3, 0.3, 8192 + 300)), ("bias", rng.uniform(-0.3, 0.3, 4))] for _ in range(3)]
    mean = [np.mean([np.asarray(vals[c][li][1]) for c in range(3)], axis=0) for li in range(2)]
    _ok(run("keyGen", cc, tmp / "pk1", tmp / "sk1"))
    for p in (2, 3):
        _ok(run("keyGen", cc, tmp / f"pk{p}", tmp / f"sk{p}", "--join", tmp / f"pk{p - 1}"))
    _ok(run("keyGen", cc, tmp / "pkr", tmp / "skr"))  # the recipient: not a party of the chain
    for c in range(3):
        _ok(run("encryptModelWeights", cc, tmp / "pk3", _weights(tmp, f"w{c}.json", vals[c]), tmp / f"enc{c}.{ext}"))
    agg = tmp / f"agg.{ext}"
    _ok(run("serverRound", cc, agg, "-", tmp / f"enc0.{ext}", "-", tmp / f"enc1.{ext}", "-", tmp / f"enc2.{ext}"))
    return dict(tmp=tmp, ext=ext, cc=cc, mean=mean, agg=agg, N=1 << 14)


def decoded_error(cc, sk, enc, out, mean):
    _ok(run("decryptModelWeights", cc, sk, enc, out))
    dec = json.load(open(out))["weights_summary"]
    return max(np.abs(np.array(dec[li]["values"]) - mean[li]).max() for li in range(2))


def switch_round(r, tag, keys, extra=(), lead=0):
    """switchShare per key (keys: [(path, per-key options)]), fuseSwitchShares; the fused file"""
    tmp, ext, cc = r["tmp"], r["ext"], r["cc"]
    files = []
    for a, (key, opts) in enumerate(keys):
        f = tmp / f"{tag}{a}.{ext}"
        _ok(run("switchShare", cc, key, tmp / "pkr", r["agg"], f, *(["--lead"] if a == lead else []), *opts, *extra))
        files.append(f)
    fused = tmp / f"{tag}.{ext}"
    _ok(run("fuseSwitchShares", cc, *files, fused))
    return files, fused


@pytest.mark.gpu
def test_key_switch_round_through_the_binaries(cli_round):
    from tests.test_seeded_ciphertexts import read_mkws
    r = cli_round
    tmp, ext, cc, mean, agg, N = r["tmp"], r["ext"], r["cc"], r["mean"], r["agg"], r["N"]
    files, fused = switch_round(r, "sh", [(tmp / f"sk{p}", o) for p, o in ((1, []), (2, ["--smudge-bits", "10"]), (3, []))])
    agg_heads = [struct.unpack(HDR, b[:48]) for b in read_mkws(agg)[1]]
    for a, f in enumerate(files):
        blobs = read_mkws(f)[1]
        assert len(blobs) == len(agg_heads)
        for b, ah in zip(blobs, agg_heads):
            h = struct.unpack(HDR, b[:48])
            assert h[2] == KIND_SWITCH_SHARE and h[5] == 2 and h[10] == (1 if a == 0 else 0) and len(b) == 48 + 16 * h[4] * N
            assert h[3:5] + h[6:10] == ah[3:5] + ah[6:10]
    # the fused file: a kind-1 envelope with the aggregate's header fields, which the recipient's key opens
    fused_blobs = read_mkws(fused)[1]
    assert [struct.unpack(HDR, b[:48]) for b in fused_blobs] == agg_heads
    assert [len(b) for b in fused_blobs] == [len(b) for b in read_mkws(agg)[1]]
    err = decoded_error(cc, tmp / "skr", fused, tmp / "dec.json", mean)
    print(f"delivered: error 2^{np.log2(err):.2f}, bound 2^{np.log2(BOUND['p14']):.2f}")
    assert err < BOUND["p14"], err
    dec = json.load(open(tmp / "dec.json"))["weights_summary"]
    assert [d["layer"] for d in dec] == ["dense", "bias"] and [d["shape"] for d in dec] == [[len(m)] for m in mean]
    # the order of the share files does not matter; a second share of the same file is drawn afresh
    _ok(run("fuseSwitchShares", cc, files[2], files[0], files[1], tmp / f"fused_b.{ext}"))
    assert _same_bytes(fused, tmp / f"fused_b.{ext}")
    _ok(run("switchShare", cc, tmp / "sk3", tmp / "pkr", agg, tmp / f"again.{ext}"))
    assert not _same_bytes(files[2], tmp / f"again.{ext}")
    # nobody else opens it: a party's key, two of the three shares, shares for another recipient mixed in (exit 0, noise)
    assert decoded_error(cc, tmp / "sk1", fused, tmp / "one.json", mean) > 1
    _ok(run("fuseSwitchShares", cc, files[0], files[1], tmp / f"two.{ext}"))
    assert decoded_error(cc, tmp / "skr", tmp / f"two.{ext}", tmp / "two.json", mean) > 1
    _ok(run("switchShare", cc, tmp / "sk3", tmp / "pk1", agg, tmp / f"other.{ext}"))
    _ok(run("fuseSwitchShares", cc, files[0], files[1], tmp / f"other.{ext}", tmp / f"mixed.{ext}"))
    assert decoded_error(cc, tmp / "skr", tmp / f"mixed.{ext}", tmp / "mixed.json", mean) > 1
    # a word at its modulus is refused on the device's count
    raw = bytearray(open(files[1], "rb").read())
    at = raw.find(fused_blobs[0][:4], 16) + 48  # first word of the first blob
    q0 = json.load(open(cc))["mkckks_cc"]["moduli"][0]
    raw[at:at + 8] = struct.pack("<Q", int(q0))
    (tmp / f"bad.{ext}").write_bytes(bytes(raw))
    bad = run("fuseSwitchShares", cc, files[0], tmp / f"bad.{ext}", files[2], tmp / f"badout.{ext}")
    assert bad.returncode == 1 and "[fuse] ERROR: 1 residue(s) not below their modulus" in bad.stderr, bad.stdout + bad.stderr
    assert not os.path.exists(tmp / f"badout.{ext}")
    # a share file is no ciphertext file, and the other way round
    for prog, args, msg in (("switchShare", (tmp / "sk1", tmp / "pkr", files[0], tmp / "x.mkws"), "not a mkckks ciphertext blob"),
                            ("decryptModelWeights", (tmp / "skr", files[0], tmp / "x.mkws"), "not a mkckks ciphertext blob"),
                            ("fuseSwitchShares", (files[0], agg, tmp / "x.mkws"), "not a mkckks key-switch share blob"),
                            ("fuseDecryptions", (files[0], files[1], tmp / "x.mkws"), "not a mkckks share blob")):
        x = run(prog, cc, *args)
        assert x.returncode == 1 and msg in x.stderr and not os.path.exists(tmp / "x.mkws"), (prog, x.stdout + x.stderr)
    # partialDecrypt + fuseDecryptions on the same aggregate still give what they gave
    for p in (1, 2, 3):
        _ok(run("partialDecrypt", cc, tmp / f"sk{p}", agg, tmp / f"pd{p}.{ext}", *(["--lead"] if p == 1 else [])))
    _ok(run("fuseDecryptions", cc, *(tmp / f"pd{p}.{ext}" for p in (1, 2, 3)), tmp / "opened.json"))
    opened = json.load(open(tmp / "opened.json"))["weights_summary"]
    for li in range(2):
        assert np.abs(np.array(opened[li]["values"]) - mean[li]).max() < BOUND["p14"], li


@pytest.mark.gpu
def test_key_switch_round_with_key_shares_through_the_binaries(cli_round):
    """(3, 2): shareKey x 3, combineKeyShares x 3; parties 1 and 3 deliver with --parties 1,3."""
    r = cli_round
    tmp, cc, mean = r["tmp"], r["cc"], r["mean"]
    for i in (1, 2, 3):
        _ok(run("shareKey", cc, tmp / f"sk{i}", 3, 2, i, tmp / f"ks{i}"))
    for j in (1, 2, 3):
        _ok(run("combineKeyShares", cc, tmp / f"sigma{j}", *(tmp / f"ks{i}.{j}" for i in (1, 2, 3))))
    files, fused = switch_round(r, "tn", [(tmp / "sigma1", ["--parties", "1,3"]), (tmp / "sigma3", ["--parties", "1,3"])])
    out = run("switchShare", cc, tmp / "sigma1", tmp / "pkr", r["agg"], tmp / "log.mkws", "--parties", "1,3").stdout
    assert "[kswitch] Key share of party 1 loaded (2-of-3, 2 parties this round)\n" in out and "Private key" not in out
    err = decoded_error(cc, tmp / "skr", fused, tmp / "tn.json", mean)
    print(f"parties 1,3: error 2^{np.log2(err):.2f}")
    assert err < BOUND["p14"], err
    # shares made with different --parties sets fuse to noise, exit 0
    _ok(run("switchShare", cc, tmp / "sigma3", tmp / "pkr", r["agg"], tmp / "tn_23.mkws", "--parties", "2,3"))
    _ok(run("fuseSwitchShares", cc, files[0], tmp / "tn_23.mkws", tmp / "tn_mixed.mkws"))
    assert decoded_error(cc, tmp / "skr", tmp / "tn_mixed.mkws", tmp / "tn_mixed.json", mean) > 1


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 2])
def test_key_switch_limbs_through_the_binaries(cli_round, m):
    """--limbs m below the aggregate's 3 limbs, at the default smudging: the shares are made at m + 1 limbs and flagged, the
    fusion rescales, and the delivered file is an m-limb ciphertext at noiseScaleDeg 1 and scale / q_m that decrypts within
    the compact bound, 16 x the full one (tests/test_compact_downlink.py: "compaction costs about two bits").  --limbs 3
    is the aggregate as it stands."""
    from tests.test_seeded_ciphertexts import read_mkws
    r = cli_round
    tmp, cc, mean, N = r["tmp"], r["cc"], r["mean"], r["N"]
    moduli = json.load(open(cc))["mkckks_cc"]["moduli"]
    L = len(moduli)
    agg_head = struct.unpack(HDR, read_mkws(r["agg"])[1][0][:48])
    assert agg_head[4] == 3 and agg_head[7] == 2
    files, fused = switch_round(r, f"l{m}", [(tmp / f"sk{p}", []) for p in (1, 2, 3)], extra=["--limbs", str(m)])
    for a, f in enumerate(files):
        for b in read_mkws(f)[1]:
            h = struct.unpack(HDR, b[:48])
            assert (h[2], h[4], h[5], h[6], h[7], h[8], h[10]) == (KIND_SWITCH_SHARE, m + 1, 2, L - m - 1, 2, agg_head[8],
                                                                   2 | (1 if a == 0 else 0)), h
            assert len(b) == 48 + 16 * (m + 1) * N
    for b in read_mkws(fused)[1]:
        h = struct.unpack(HDR, b[:48])
        assert (h[2], h[4], h[5], h[6], h[7]) == (KIND_CT, m, 2, L - m, 1) and len(b) == 48 + 16 * m * N, h
        assert h[8] == agg_head[8] / float(int(moduli[m]))
    err = decoded_error(cc, tmp / "skr", fused, tmp / f"l{m}.json", mean)
    print(f"--limbs {m}: error 2^{np.log2(err):.2f}, bound 2^{np.log2(16 * BOUND['p14']):.2f}")
    assert err < 16 * BOUND["p14"], (m, err)
    if m == 1:
        # flagged and unflagged shares do not fuse; --limbs 3 writes what no flag writes (sizes and headers)
        _ok(run("switchShare", cc, tmp / "sk3", tmp / "pkr", r["agg"], tmp / "l3.mkws", "--limbs", "3"))
        assert all(struct.unpack(HDR, b[:48])[4:11] == agg_head[4:10] + (0,) for b in read_mkws(tmp / "l3.mkws")[1])
        bad = run("fuseSwitchShares", cc, files[0], files[1], tmp / "l3.mkws", tmp / "badmix.mkws")
        assert bad.returncode == 1 and "shares differ in layers, shapes, limbs, levels or scales" in bad.stderr
        assert not os.path.exists(tmp / "badmix.mkws")
