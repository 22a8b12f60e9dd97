"""The integer-class Q limb (q_0) of the merged n-client flow in its two forms: k_qsum3_int, whose workgroup walks the
clients of a group and keeps one pair of 128-bit accumulator sets over digits and clients (MKCKKS_Q0_WALK=1), and the
two kernels k_row3_inner_int + k_row3_tail_once with a compact til between them (MKCKKS_Q0_WALK=0).  `auto` chooses per
call by grid size (mkckks_q0_walk_choice).

Every device result is compared bit for bit with the oracle's per-client chain, FastCpuContext.reencrypt + eval_add,
and the two forms with each other.  Shapes are the smallest at which the walk can go wrong: N = 2^14 (256-point rows)
with 2, 3 and 6 digits and a single-digit level, 1 / 2 / 8 clients, 1 / 3 ciphertext indices, a second client group
(the running sum taken over from `out`), maximal operands through a whole run of the deferred reduction and across the
end of a run, the 512-point-row instance, the weighted instance and the Shoup instances.

The accumulator runs (qsum_kernels.hpp): 31 products per run on a pseudo-Mersenne limb, 15 on a Shoup limb; a client
adds beta products.  beta = 3: runs of 10 (5) clients, beta = 6: runs of 5 (2) -- 8 clients at beta = 6 and 12 clients
at beta = 3 cross the end of a run in both arithmetics.

What the maximal-residue inputs reach: a build whose pseudo-Mersenne runs were 63 products long (8 clients x 6 digits
in one run) still passed test_accumulator_bound on an MI355X -- the lazy transform outputs of these inputs stay far
enough below 8U that 48 products do not wrap 2^128.  These cases therefore check the run boundaries (carry-over of the
reduced value, the last partial run, both arithmetics), not the bound itself; the bound -- 31 products of (8U - 1) x
(q - 1) on top of a carried q - 1 through mac128 and pm_reduce128_wide -- is checked on the host by
ppqsflhe_amd/csrc/pm_glue_selftest.cpp (tests/test_pm_glue.py) and derived in qsum_kernels.hpp.

Runs on a real MI355X (`-m gpu`), except the path-choice test, which needs only the library.
"""
import os

import numpy as np
import pytest

from oracle.oracle import FastCpuContext  # noqa: E402

gpu = pytest.mark.gpu

PARAMS = {
    # name: (log_n, depth, scaling_bits, first_bits, dnum); L = depth + 2
    "l4d2": (14, 2, 40, 60, 2),
    "l6d3": (14, 4, 40, 60, 3),
    "l6d6": (14, 4, 40, 60, 6),   # six digits: the largest instance of the kernel
    "n17": (17, 2, 50, 60, 2),    # 512-point rows
}
FORMS = ("0", "1")  # MKCKKS_Q0_WALK: two kernels, one kernel


class _Env:
    """Library switches are read once, when a context is created: set them around the constructor only."""

    def __init__(self, env):
        self.env, self.old = env, {}

    def __enter__(self):
        for k, v in self.env.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ctxs():
    """Device contexts by (parameter set, switches) and one oracle per parameter set, created on first use."""
    from ppqsflhe_amd import Context
    dev, ora = {}, {}

    def device(name, **env):
        key = (name, tuple(sorted(env.items())))
        if key not in dev:
            a = PARAMS[name]
            with _Env(env):
                dev[key] = Context(a[0], a[1], a[2], a[3], dnum=a[4], device=0)
        return dev[key]

    def oracle(name):
        if name not in ora:
            a = PARAMS[name]
            ora[name] = FastCpuContext(a[0], a[1], a[2], a[3], dnum=a[4])
        return ora[name]

    device.oracle = oracle
    yield device
    for g in dev.values():
        g.close()


def rand_polys(rng, ctx, limb_ids, count):
    out = np.empty((count, len(limb_ids), ctx.N), dtype=np.uint64)
    for j, l in enumerate(limb_ids):
        out[:, j, :] = rng.integers(0, int(ctx.moduli[l]), size=(count, ctx.N), dtype=np.uint64)
    return out


def oracle_chain(o, cts, evks):
    """Per index, the EvalAdd chain over the clients of their re-encryptions: [B][2][nl][N]."""
    C, B = cts.shape[:2]
    out = []
    for b in range(B):
        acc = o.reencrypt(cts[0, b], evks[0])
        for c in range(1, C):
            acc = o.eval_add(acc, o.reencrypt(cts[c, b], evks[c]))
        out.append(acc)
    return np.stack(out)


_cases = {}


def case(o, name, nl, C, B):
    """Seeded inputs and their oracle result, computed once per shape and shared (read-only) by the tests."""
    key = (name, nl, C, B)
    if key not in _cases:
        rng = np.random.default_rng(7300 + 101 * nl + 17 * C + B)
        cts = rand_polys(rng, o, list(range(nl)) * 2, C * B).reshape(C, B, 2, nl, o.N)
        evks = rand_polys(rng, o, list(range(o.D)) * (2 * o.beta), C).reshape(C, o.beta, 2, o.D, o.N)
        want = oracle_chain(o, cts, evks)
        for a in (cts, evks, want):
            a.setflags(write=False)
        _cases[key] = (cts, evks, want)
    return _cases[key]


def gpu_sum(g, cts, evks, nl):
    C, B = cts.shape[:2]
    d_out = g.empty((B, 2, nl, g.N))
    g.reencrypt_sum(g.to_device(cts), g.to_device(evks), d_out, C, B, nl)
    return d_out.to_host()


def check_both_forms(ctxs, name, nl, C, B, **env):
    cts, evks, want = case(ctxs.oracle(name), name, nl, C, B)
    got = [gpu_sum(ctxs(name, MKCKKS_Q0_WALK=form, **env), cts, evks, nl) for form in FORMS]
    assert np.array_equal(got[0], want), "two-kernel form differs from the oracle chain"
    assert np.array_equal(got[1], want), "one-kernel form differs from the oracle chain"
    assert np.array_equal(got[0], got[1])


@gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 2, 8])
@pytest.mark.parametrize("name,nl", [("l4d2", 4), ("l6d3", 6), ("l6d6", 6),
                                     ("l4d2", 2)])  # nl = 2: one digit, both switch values take the two-kernel form
def test_both_forms_equal_the_oracle_and_each_other(ctxs, name, nl, C, B):
    check_both_forms(ctxs, name, nl, C, B)


@gpu
@pytest.mark.parametrize("C,env", [(9, {}),                              # 8 + 1 clients: the second group adds to `out`
                                   (16, {"MKCKKS_QSUM_GROUP": "15"})])   # 15 + 1
def test_client_groups(ctxs, C, env):
    check_both_forms(ctxs, "l4d2", 4, C, 1, **env)


def extreme_case(o, nl, C, alternating):
    """Every residue of c0, c1 and of the eval keys q - 1, or alternating 0 / q - 1; the same for every client, so one
    oracle re-encryption serves the whole chain."""
    mask = (np.arange(o.N) % 2 == 0) if alternating else np.ones(o.N, dtype=bool)
    ct = np.zeros((2, nl, o.N), dtype=np.uint64)
    evk = np.zeros((o.beta, 2, o.D, o.N), dtype=np.uint64)
    for l in range(nl):
        ct[:, l, mask] = int(o.moduli[l]) - 1
    for l in range(o.D):
        evk[:, :, l, mask] = int(o.moduli[l]) - 1
    one = o.reencrypt(ct, evk)
    want = one
    for _ in range(1, C):
        want = o.eval_add(want, one)
    cts = np.ascontiguousarray(np.broadcast_to(ct, (C, 1) + ct.shape))
    evks = np.ascontiguousarray(np.broadcast_to(evk, (C,) + evk.shape))
    return cts, evks, want


# (parameters, clients, switches): three digits with 8 clients (one run of 24 products on a pseudo-Mersenne limb), six
# digits with 8 clients and three digits with 12 clients in one group (both cross the end of a run)
BOUND_CASES = [("l6d3", 8, {}), ("l6d6", 8, {}), ("l6d3", 12, {"MKCKKS_QSUM_GROUP": "15"})]


def check_accumulator_bound(ctxs, name, C, alternating, **env):
    o = ctxs.oracle(name)
    cts, evks, want = extreme_case(o, 6, C, alternating)
    for form in FORMS:
        got = gpu_sum(ctxs(name, MKCKKS_Q0_WALK=form, **env), cts, evks, 6)
        assert np.array_equal(got[0], want), f"MKCKKS_Q0_WALK={form}"


@gpu
@pytest.mark.parametrize("alternating", [False, True])
@pytest.mark.parametrize("name,C,env", BOUND_CASES)
def test_accumulator_bound(ctxs, name, C, env, alternating):
    """Every residue q - 1, then alternating 0 / q - 1, through every client: whole runs of the deferred reduction and
    runs that end inside the client loop (see the module docstring for what these inputs do and do not reach)."""
    check_accumulator_bound(ctxs, name, C, alternating, **env)


@gpu
def test_512_point_rows(ctxs):
    check_both_forms(ctxs, "n17", 4, 2, 1)


@gpu
def test_weighted_instance(ctxs):
    """reencrypt_wsum with three distinct weights against the composition the weighted tests use:
    sum_c ReEncrypt((M_c c0_c, c1_c), M_c evk_c) on the oracle."""
    from tests.test_weighted_aggregation import device_wsum, oracle_wsum, rand_evks, scaled_evk
    from tests.test_gpu_parity import rand_ct
    name, nl, C, B = "l4d2", 4, 3, 2
    o = ctxs.oracle(name)
    rng = np.random.default_rng(53)
    cts = np.stack([rand_ct(rng, o, nl, B) for _ in range(C)])
    evks = rand_evks(rng, o, C)
    weights, sf_level = [0.3125, 2.5, 0.123456789], o.L - nl + 1
    evks_s = [scaled_evk(o, evks[c], weights[c], sf_level) for c in range(C)]
    want = np.stack([oracle_wsum(o, cts, evks_s, weights, sf_level, b) for b in range(B)])
    for form in FORMS:
        got, _ = device_wsum(ctxs(name, MKCKKS_Q0_WALK=form), cts, evks, weights, sf_level, nl)
        assert np.array_equal(got, want), f"MKCKKS_Q0_WALK={form}"


@gpu
def test_shoup_arithmetic_both_forms(ctxs):
    check_both_forms(ctxs, "l6d3", 6, 8, 3, MKCKKS_NO_PM="1")


@gpu
@pytest.mark.parametrize("alternating", [False, True])
@pytest.mark.parametrize("name,C,env", BOUND_CASES)
def test_shoup_arithmetic_accumulator_bound(ctxs, name, C, env, alternating):
    check_accumulator_bound(ctxs, name, C, alternating, MKCKKS_NO_PM="1", **env)


def test_path_choice():
    """auto takes the one-kernel form at the flagship's (32 tiles, 1 limb, 16 indices) and the two-kernel form at one
    index; the switch overrides both."""
    from ppqsflhe_amd import binding
    choice = binding.load_library().mkckks_q0_walk_choice
    AUTO = 2
    assert choice(32, 1, 16, AUTO) == 1
    assert choice(32, 1, 1, AUTO) == 0
    assert choice(32, 1, 2, AUTO) == 0  # the server pipeline's chunks of 2 indices
    for shape in ((32, 1, 16), (32, 1, 1)):
        assert choice(*shape, 0) == 0
        assert choice(*shape, 1) == 1
