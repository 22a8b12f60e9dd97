// const_fold_selftest -- the host tables and host forms behind two folded constants, against unsigned __int128 arithmetic
// (`make asan` builds it under -fsanitize=address,undefined; tests/test_const_fold.py runs it):
//
//  * ParamSet::modup_table_pscaled: the ModUp constants of the P targets carry ModDown's scale sc_k = N^-1 [(P/p_k)^-1]_{p_k},
//    so  sum_i x_i [S/s_i sc_k]  =  sc_k sum_i x_i [S/s_i]  (mod p_k)  for maximal and random sources, also through the
//    integer column accumulation the device uses (mac_cols + pm_reduce_cols / reduce_cols_lazy); Q targets are unchanged;
//  * canon_inverse_round: the canonical residue of an inverse round's output word, at the derived maximal lazy word, at 0,
//    at p - 1, at the multiples of p inside the bound, and on the outputs of the round's last butterfly (host forms);
//  * hat_as_doubles' constants of packed source 0: lo H0 + hi H1 = x [S/s_0] (mod t) for x = lo + 2^30 hi, evaluated
//    with the FMA sequence of fp_mulmod, each product within 0.51 t.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "params.hpp"

namespace {
using mk::u128;
using mk::u64;

struct Counts {
    unsigned long long scaled = 0, cols = 0, canon_pm = 0, canon_shoup = 0, halves = 0;
};

[[noreturn]] void fail(const std::string &what, u64 q) { throw std::runtime_error(what + " at modulus " + std::to_string(q)); }

u64 rng_state = 0x9E3779B97F4A7C15ull;
u64 next() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// sc_k, written out independently of ParamSet::moddown_scale
u64 scale_of(const mk::ParamSet &ps, uint32_t k) {
    const u64 p = ps.moduli[ps.L + k];
    u64 phat = 1;
    for (uint32_t m = 0; m < ps.K; ++m)
        if (m != k) phat = (u64)((u128)phat * (ps.moduli[ps.L + m] % p) % p);
    return (u64)((u128)mk::h_invmod(ps.n % p, p) * mk::h_invmod(phat, p) % p);
}

mk::LimbConst as_pm(const mk::LimbConst &in) {
    mk::LimbConst lc = in;
    lc.pm = 1;
    lc.pm_c = (uint32_t)(((u64)1 << lc.k) - lc.q);
    return lc;
}

// ---- A: the P-scaled ModUp tables ---------------------------------------------------------------------------------------
void check_scaled_tables(const mk::ParamSet &ps, uint32_t nl, Counts &n) {
    for (uint32_t part = 0; part < ps.num_parts(nl); ++part) {
        const mk::BaseConvTable t = ps.modup_table(nl, part), s = ps.modup_table_pscaled(nl, part);
        const size_t ni = t.src.size(), no = t.dst.size();
        if (s.src != t.src || s.dst != t.dst || s.hatinv != t.hatinv || s.hatinv_sh != t.hatinv_sh || s.hat.size() != t.hat.size())
            fail("scaled table: sources, targets or source constants differ", 0);
        for (size_t j = 0; j < no; ++j) {
            const uint32_t id = t.dst[j];
            const u64 p = ps.moduli[id];
            if (id < ps.L) {  // Q target: as it was
                for (size_t i = 0; i < ni; ++i)
                    if (s.hat[i * no + j] != t.hat[i * no + j]) fail("scaled table: a Q target changed", p);
                continue;
            }
            const u64 sc = scale_of(ps, id - ps.L);
            if (sc != ps.moddown_scale(id - ps.L)) fail("moddown_scale", p);
            for (size_t i = 0; i < ni; ++i) {
                const u64 h = s.hat[i * no + j];
                if (h >= p || h != (u64)((u128)t.hat[i * no + j] * sc % p)) fail("scaled constant", p);
            }
            const mk::LimbConst lc = as_pm(ps.limb[id]);
            const bool pm = mk::pm_eligible(p);
            for (int it = 0; it < 2000; ++it) {
                u128 plain = 0, scaled = 0;
                mk::Cols cols{0, 0, 0};
                for (size_t i = 0; i < ni; ++i) {
                    const u64 si = ps.moduli[t.src[i]], x = it == 0 ? si - 1 : it == 1 ? 0 : it == 2 ? (i & 1 ? si - 1 : 0) : next() % si;
                    plain += (u128)x * t.hat[i * no + j];    // <= 8 products below 2^120
                    scaled += (u128)x * s.hat[i * no + j];
                    if (ni <= 4) {
                        uint32_t a0, a1, b0, b1;
                        mk::split30(x, a0, a1);
                        mk::split30(s.hat[i * no + j], b0, b1);
                        mk::mac_cols(cols, a0, a1, b0, b1);
                    }
                }
                const u64 want = (u64)((u128)(u64)(plain % p) * sc % p);
                if ((u64)(scaled % p) != want) fail("scaled conversion differs from sc * conversion", p);
                ++n.scaled;
                if (ni <= 4) {  // the device's integer path of k_conv_col, host forms
                    if (pm && mk::pm_reduce_cols(cols, mk::pm_consts(lc)) % p != want) fail("pm_reduce_cols of the scaled columns", p);
                    if (mk::reduce_cols_lazy(cols, ps.limb[id]) % p != want) fail("reduce_cols_lazy of the scaled columns", p);
                    ++n.cols;
                }
            }
        }
    }
}

// ---- A: canonicalisation of the inverse round's output ------------------------------------------------------------------
void check_canon(const mk::LimbConst &lc_in, Counts &n) {
    const u64 p = lc_in.q;
    // Shoup instance: words below 2p
    {
        const mk::LimbConst &lc = lc_in;
        for (u64 v : {(u64)0, (u64)1, p - 1, p, p + 1, 2 * p - 1})
            if (mk::canon_inverse_round(v, lc, false) != v % p) fail("canon (Shoup) at an edge", p);
        for (int it = 0; it < 200000; ++it) {
            // the last stage's two outputs from arbitrary words: csub(x + y, 2p) for x, y < 2p, and shoup_lazy of any word
            const u64 w = next() % p, wp = mk::h_shoup(w, p), x = next() % (2 * p), y = next() % (2 * p);
            const u64 d = it % 3 == 0 ? next() : x + 2 * p - y;
            const u64 o1 = mk::csub(x + y, lc.q2), o2 = mk::shoup_lazy(d, w, wp, p);
            if (o1 >= 2 * p || o2 >= 2 * p) fail("Shoup round output not below 2p", p);
            if (mk::canon_inverse_round(o1, lc, false) != (u64)(((u128)x + y) % p)) fail("canon (Shoup) of the sum", p);
            if (mk::canon_inverse_round(o2, lc, false) != (u64)((u128)d * w % p)) fail("canon (Shoup) of the product", p);
            n.canon_shoup += 2;
        }
    }
    if (!mk::pm_eligible(p)) return;
    // pseudo-Mersenne instance: words below 2.375U = 19 * 2^(k-3)
    const mk::LimbConst lc = as_pm(lc_in);
    const mk::PmK P = mk::pm_consts(lc);
    const u64 U = (u64)1 << lc.k, bound = 19 * (U >> 3);  // exclusive
    if (!(bound > 2 * p && bound <= 3 * p)) fail("2.375U is not in (2p, 3p]", p);
    for (u64 v : {(u64)0, (u64)1, p - 1, p, p + 1, 2 * p - 1, 2 * p, 2 * p + 1, bound - 1, U, U + ((u64)1 << 30) - 1})
        if (mk::canon_inverse_round(v, lc, true) != v % p) fail("canon (pm) at an edge", p);
    for (u64 m = 0; m * p < bound; ++m) {  // multiples of p: canonical 0, never p
        if (mk::canon_inverse_round(m * p, lc, true) != 0) fail("canon (pm) of a multiple of p", p);
        const u64 top = m * p + (p - 1);
        if (top < bound && mk::canon_inverse_round(top, lc, true) != p - 1) fail("canon (pm) below a multiple of p", p);
    }
    for (int it = 0; it < 200000; ++it) {
        const u64 v = next() % bound;
        if (mk::canon_inverse_round(v, lc, true) != v % p) fail("canon (pm), random word", p);
        // the last stage of the round (gs_butterfly_pm) on inputs below 2.375U, maximal ones included
        const u64 x = it < 4 ? bound - 1 : next() % bound, y = it < 4 ? (it & 1 ? bound - 1 : 0) : next() % bound;
        const u64 w = it < 4 ? p - 1 : next() % p;
        const u64 d = (x + P.q3) - y;
        const u64 o1 = mk::pm_fold(x + y, P), o2 = mk::pm_lazy(d, mk::pm_tw(w, lc), mk::pm_tw_companion(w, lc), P);
        if (o1 >= bound || o2 >= bound) fail("pm round output not below 2.375U", p);
        if (mk::canon_inverse_round(o1, lc, true) != (u64)(((u128)x + y) % p)) fail("canon (pm) of the sum", p);
        if (mk::canon_inverse_round(o2, lc, true) != (u64)((u128)d * w % p)) fail("canon (pm) of the product", p);
        n.canon_pm += 3;
    }
}

// ---- B: the two double constants of packed source 0 ---------------------------------------------------------------------
// fp_mulmod of modarith.hpp, operation for operation (round-to-nearest multiplies, fused multiply-adds)
double fp_mulmod_host(double y, double w, double wq, double q) {
    const double h = y * w;
    const double l = std::fma(y, w, -h);
    const double b = std::rint(y * wq);
    const double c = std::fma(-b, q, h);
    return c + l;
}
double as_double(u64 bits) {
    double d;
    std::memcpy(&d, &bits, 8);
    return d;
}

void check_halves(const mk::ParamSet &ps, uint32_t nl, Counts &n) {
    for (uint32_t part = 0; part < ps.num_parts(nl); ++part) {
        for (int scaled = 0; scaled < 2; ++scaled) {
            const mk::BaseConvTable t = scaled ? ps.modup_table_pscaled(nl, part) : ps.modup_table(nl, part);
            const std::vector<u64> v = mk::hat_as_doubles(t, ps.moduli);
            const size_t cnt = t.hat.size(), no = t.dst.size();
            if (v.size() != 2 * cnt + 2 * no) fail("hat_as_doubles: size", 0);
            const u64 s0 = ps.moduli[t.src[0]];
            for (size_t j = 0; j < no; ++j) {
                const u64 q = ps.moduli[t.dst[j]];
                if ((long double)q >= 1.25L * (long double)((u64)1 << 50)) continue;  // not an fp64-class target
                const double qd = (double)q;
                const double H0 = as_double(v[j]), H0q = as_double(v[cnt + j]);
                const double H1 = as_double(v[2 * cnt + j]), H1q = as_double(v[2 * cnt + no + j]);
                const u64 h0 = t.hat[j], h1 = (u64)((u128)h0 * (((u64)1 << 30) % q) % q);
                if (H0 != (double)h0 || (u64)H0 != h0 || H1 != (double)h1 || (u64)H1 != h1) fail("half constants are not the exact integers", q);
                if (H0q != (double)((long double)h0 / (long double)q) || H1q != (double)((long double)h1 / (long double)q))
                    fail("half constants: quotients", q);
                auto one = [&](u64 lo, u64 hi) {
                    const double a = fp_mulmod_host((double)lo, H0, H0q, qd), b = fp_mulmod_host((double)hi, H1, H1q, qd);
                    if (std::fabs(a) > 0.51 * qd || std::fabs(b) > 0.51 * qd) fail("half product outside 0.51 q", q);
                    if (a != std::rint(a) || b != std::rint(b)) fail("half product is not an integer", q);
                    const long long sum = (long long)a + (long long)b;  // |sum| < 2^52
                    const u64 got = (u64)(((sum % (long long)q) + (long long)q) % (long long)q);
                    const u128 x = (u128)lo + ((u128)hi << 30);
                    if (got != (u64)(x * h0 % q)) fail("lo H0 + hi H1 differs from x [S/s_0]", q);
                    ++n.halves;
                };
                const u64 M = ((u64)1 << 30) - 1;
                one(0, 0);
                one((s0 - 1) & M, (s0 - 1) >> 30);  // x = s_0 - 1
                one(M, M);                           // both halves maximal
                one(M, 0);
                one(0, M);
                for (int it = 0; it < 20000; ++it) {
                    const u64 x = next() % s0;
                    one(x & M, x >> 30);
                }
            }
        }
    }
}
}  // namespace

int main() {
    struct Cfg { uint32_t log_n, depth, sbits, first, dnum; };
    try {
        Counts n;
        unsigned p_limbs = 0;
        // the shapes of tests/test_const_fold.py, the flagship (N = 2^16, L = 12, dnum 3) and N = 2^17, L = 20 (7 sources)
        for (const Cfg &c : {Cfg{14, 2, 40, 60, 2}, Cfg{14, 4, 40, 60, 3}, Cfg{17, 2, 50, 60, 2}, Cfg{16, 10, 50, 60, 3},
                             Cfg{17, 18, 50, 60, 3}}) {
            mk::ParamSet ps;
            ps.generate(c.log_n, c.depth, c.sbits, c.first, c.dnum, 60, 20);
            for (uint32_t nl : {ps.L, ps.L - 1, ps.alpha + 1, 2u}) {
                if (nl < 1 || nl > ps.L) continue;
                check_scaled_tables(ps, nl, n);
                check_halves(ps, nl, n);
            }
            for (uint32_t k = 0; k < ps.K; ++k, ++p_limbs) check_canon(ps.limb[ps.L + k], n);
            check_canon(ps.limb[0], n);  // q_0: the other integer-class modulus
            std::printf("ok log_n=%u L=%u dnum=%u K=%u\n", c.log_n, ps.L, c.dnum, ps.K);
        }
        if (!n.scaled || !n.cols || !n.canon_pm || !n.canon_shoup || !n.halves) throw std::runtime_error("a check never ran");
        std::printf("ok const fold: %u P limbs, scaled sums %llu, column forms %llu, canon pm %llu, canon shoup %llu, halves %llu\n",
                    p_limbs, n.scaled, n.cols, n.canon_pm, n.canon_shoup, n.halves);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "ERROR: %s\n", e.what());
        return 1;
    }
    return 0;
}
