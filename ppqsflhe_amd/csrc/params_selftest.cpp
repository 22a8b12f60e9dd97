// params_selftest -- params.cpp (parameter generation, CRT / base-conversion tables, twiddles) on the host only: the
// piece of the library that is plain C++ and can run under -fsanitize=address,undefined (`make asan`; GPU code cannot be
// sanitised on this pool).  Prints a checksum line per configuration; tests/test_sanitizers.py runs it.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include "params.hpp"

int main() {
    struct Cfg { uint32_t log_n, depth, sbits, first, dnum, aux = 60, extra = 20; };
    const Cfg cfgs[] = {{10, 3, 40, 60, 2}, {12, 1, 40, 60, 2}, {14, 2, 40, 60, 2}, {12, 18, 50, 60, 3}, {16, 10, 50, 60, 3}};
    try {
        for (const Cfg &c : cfgs) {
            mk::ParamSet ps;
            ps.generate(c.log_n, c.depth, c.sbits, c.first, c.dnum, 60, 20);
            unsigned long long sum = 0;
            for (uint32_t nl = 1; nl <= ps.L; ++nl) {
                for (uint32_t part = 0; part < ps.num_parts(nl); ++part) {
                    const mk::BaseConvTable t = ps.modup_table(nl, part);
                    if (t.hat.size() != t.src.size() * t.dst.size()) throw std::runtime_error("modup table shape");
                    for (mk::u64 v : t.hat) sum += v;
                }
                const mk::BaseConvTable md = ps.moddown_table(nl);
                for (mk::u64 v : md.hat) sum += v;
                (void)ps.const_factors(nl, ps.L - nl, 0.5);
            }
            std::vector<mk::u64> w, wsh;
            for (uint32_t id : {0u, ps.L - 1, ps.D - 1}) {
                ps.twiddles(id, false, w, wsh);
                ps.twiddles(id, true, w, wsh);
                sum += w[1] + wsh[ps.n - 1];
                sum += ps.p_mod(id % ps.L) + ps.p_inv_mod(id % ps.L);
            }
            std::printf("ok log_n=%u L=%u K=%u alpha=%u beta=%u checksum=%llu\n", ps.log_n, ps.L, ps.K, ps.alpha, ps.beta, sum);
        }
        // pseudo-Mersenne arithmetic of modarith.hpp (host mirror of the device code): congruence and the stated output
        // bounds on boundary and random operands, for every eligible prime the configurations above produce plus first
        // moduli of every width from 51 to 59 bits and special primes of 55 bits (the shifts of pm_fold, pm_lazy and
        // pm_reduce128 depend on the width k).  Every width a configuration asks for must turn up among the primes checked.
        {
            using mk::u64;
            typedef unsigned __int128 u128;
            unsigned long long checked = 0;
            u64 rng = 0x9E3779B97F4A7C15ull;
            auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
            u64 widths_wanted = 0, widths_seen = 0;  // bit k: an integer limb of k bits was asked for / was checked
            for (const Cfg &c : {Cfg{14, 2, 40, 60, 2}, Cfg{16, 10, 50, 60, 3}, Cfg{14, 2, 40, 55, 2}, Cfg{14, 2, 40, 58, 2},
                                 Cfg{17, 19, 50, 60, 3}, Cfg{12, 2, 40, 52, 2}, Cfg{12, 2, 40, 60, 2, 55}, Cfg{12, 2, 40, 51, 2},
                                 Cfg{12, 2, 40, 53, 2}, Cfg{12, 2, 40, 54, 2}, Cfg{12, 2, 40, 56, 2}, Cfg{12, 2, 40, 57, 2},
                                 Cfg{12, 2, 40, 59, 2}}) {
                mk::ParamSet ps;
                ps.generate(c.log_n, c.depth, c.sbits, c.first, c.dnum, c.aux, c.extra);
                for (uint32_t bits : {c.first, c.aux})
                    if (bits >= 51) widths_wanted |= (u64)1 << bits;
                for (uint32_t i = 0; i < ps.D; ++i) {
                    const u64 q = ps.moduli[i];
                    if (q < (5ull << 48) || !mk::pm_eligible(q)) continue;
                    mk::LimbConst lc = ps.limb[i];
                    widths_seen |= (u64)1 << lc.k;
                    lc.pm = 1;
                    lc.pm_c = (uint32_t)(((u64)1 << lc.k) - q);
                    const mk::PmK P = mk::pm_consts(lc);
                    const u64 U = (u64)1 << lc.k, amax = (U << 3) - 1;
                    const u64 as[] = {0, 1, q - 1, q, U - 1, U, 2 * q, amax, amax - 1, (U << 2) + 12345, 0xffffffffull,
                                      0x100000000ull, amax & ~0xffffffffull};
                    const u64 ws[] = {0, 1, q - 1, q / 2, 0xffffffffull, 0x100000000ull, q - 0xffffffffull};
                    auto check = [&](u64 a, u64 w) {
                        const u64 r = mk::pm_lazy(a, mk::pm_tw(w, lc), mk::pm_tw_companion(w, lc), P);
                        if (r % q != (u64)((u128)a * w % q)) throw std::runtime_error("pm_lazy: wrong residue");
                        if ((u128)r * 8 >= (u128)U * 19) throw std::runtime_error("pm_lazy: result not below 2.375 * 2^k");
                        if (r > P.q3) throw std::runtime_error("pm_lazy: result above 3q");
                        ++checked;
                    };
                    for (u64 a : as)
                        for (u64 w : ws) check(a, w);
                    for (int it = 0; it < 20000; ++it) check(next() & amax, next() % q);
                    // 128-bit accumulators of the eval-key inner product: up to 6 products (lazy word < 8U) x (residue < q)
                    for (int it = 0; it < 20000; ++it) {
                        u128 X = 0;
                        const int terms = 1 + it % 6;
                        for (int t = 0; t < terms; ++t) {
                            const u64 a = (it % 5 == 0) ? amax : (next() & amax), b = (it % 7 == 0) ? q - 1 : next() % q;
                            X += (u128)a * b;
                        }
                        const u64 r = mk::pm_reduce128((u64)(X >> 64), (u64)X, P, q);
                        if (r != (u64)(X % q)) throw std::runtime_error("pm_reduce128");
                        ++checked;
                    }
                    // column sums of up to 4 products of 60-bit numbers split in 30-bit halves (base conversion)
                    for (int it = 0; it < 20000; ++it) {
                        mk::Cols cs{0, 0, 0};
                        u128 X = 0;
                        for (int t = 0; t < 1 + it % 4; ++t) {
                            const u64 a = (it % 5 == 0) ? (1ull << 60) - 1 : next() >> 4, b = (it % 3 == 0) ? q - 1 : next() % q;
                            uint32_t a0, a1, b0, b1;
                            mk::split30(a, a0, a1);
                            mk::split30(b, b0, b1);
                            mk::mac_cols(cs, a0, a1, b0, b1);
                            X += (u128)a * b;
                        }
                        const u64 r = mk::pm_reduce_cols(cs, P);
                        if (r % q != (u64)(X % q) || r >= 2 * U + (U >> 3)) throw std::runtime_error("pm_reduce_cols");
                        ++checked;
                    }
                    const u64 xs[] = {0, q, U, ~0ull, ~0ull - 1, U - 1, amax};
                    for (u64 x : xs) {
                        const u64 f = mk::pm_fold(x, P);
                        if (f % q != x % q || f >= U + (1ull << 30)) throw std::runtime_error("pm_fold");
                    }
                    for (int it = 0; it < 20000; ++it) {
                        const u64 x = next(), f = mk::pm_fold(x, P);
                        if (f % q != x % q || f >= U + (1ull << 30)) throw std::runtime_error("pm_fold");
                    }
                }
            }
            if (!checked) throw std::runtime_error("no pseudo-Mersenne prime was exercised");
            for (uint32_t k = 51; k <= 60; ++k)
                if ((widths_wanted >> k & 1) && !(widths_seen >> k & 1))
                    throw std::runtime_error("no eligible pseudo-Mersenne prime of " + std::to_string(k) + " bits");
            std::printf("ok pseudo-Mersenne arithmetic (%llu products)\n", checked);
        }
        // Barrett / Shoup arithmetic of modarith.hpp (what every limb outside the fp64 and pseudo-Mersenne classes runs, and
        // every base conversion): exact against unsigned __int128 at the ends of the stated operand ranges, for every
        // modulus of the contexts of tests/test_parameter_lattice.py -- 18 to 60 bits wide
        {
            using mk::u64;
            typedef unsigned __int128 u128;
            unsigned long long checked = 0, moduli = 0;
            u64 rng = 0xD1B54A32D192ED03ull;
            auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
            auto fail = [](const char *what, u64 q) {
                throw std::runtime_error(std::string(what) + " at q = " + std::to_string(q));
            };
            u64 widths = 0;
            for (const Cfg &c : {Cfg{12, 2, 51, 60, 2}, Cfg{12, 2, 54, 60, 2}, Cfg{12, 2, 59, 60, 2}, Cfg{14, 3, 55, 60, 2},
                                 Cfg{16, 2, 56, 60, 3}, Cfg{12, 3, 30, 60, 2}, Cfg{16, 2, 21, 60, 2}, Cfg{17, 2, 24, 60, 2},
                                 Cfg{12, 2, 24, 40, 2}, Cfg{12, 2, 40, 45, 2}, Cfg{12, 2, 40, 52, 2}, Cfg{12, 2, 40, 60, 2, 45},
                                 Cfg{12, 2, 40, 60, 2, 55}, Cfg{12, 2, 40, 60, 2, 30, 18}, Cfg{12, 2, 40, 60, 2, 60, 30},
                                 Cfg{12, 6, 40, 60, 1}, Cfg{12, 4, 40, 60, 6}, Cfg{12, 8, 40, 60, 2}, Cfg{12, 14, 40, 60, 2},
                                 Cfg{12, 14, 40, 60, 2, 48}, Cfg{8, 3, 50, 60, 2}, Cfg{13, 2, 50, 60, 2}, Cfg{15, 2, 50, 60, 3}}) {
                mk::ParamSet ps;
                ps.generate(c.log_n, c.depth, c.sbits, c.first, c.dnum, c.aux, c.extra);
                for (uint32_t i = 0; i < ps.D; ++i) {
                    const mk::LimbConst &lc = ps.limb[i];
                    const u64 q = lc.q;
                    widths |= (u64)1 << lc.k;
                    ++moduli;
                    // mul_mod: a, b < q
                    const u64 ends[] = {0, 1, q - 1};
                    for (u64 a : ends)
                        for (u64 b : ends)
                            if (mk::mul_mod(a, b, lc) != (u64)((u128)a * b % q)) fail("mul_mod", q);
                    for (int it = 0; it < 2000; ++it) {
                        const u64 a = next() % q, b = next() % q;
                        if (mk::mul_mod(a, b, lc) != (u64)((u128)a * b % q)) fail("mul_mod", q);
                    }
                    // barrett_reduce128: x < 2^(k + 62), at the largest such x and below it
                    const u128 top = ((u128)1 << (lc.k + 62)) - 1;
                    for (int it = 0; it < 2000; ++it) {
                        const u128 x = it == 0 ? top : it == 1 ? top - q : (((u128)next() << 64) | next()) & top;
                        if (mk::barrett_reduce128((u64)(x >> 64), (u64)x, lc) != (u64)(x % q)) fail("barrett_reduce128", q);
                    }
                    // reduce_word: any 64-bit word
                    for (u64 x : {(u64)0, q, q - 1, 2 * q, ~(u64)0, ~(u64)0 - q})
                        if (mk::reduce_word(x, lc) != x % q) fail("reduce_word", q);
                    for (int it = 0; it < 2000; ++it) {
                        const u64 x = next();
                        if (mk::reduce_word(x, lc) != x % q) fail("reduce_word", q);
                    }
                    // reduce_wide: accumulators below 2^124
                    const u128 wide = ((u128)1 << 124) - 1;
                    for (int it = 0; it < 2000; ++it) {
                        const u128 x = it == 0 ? wide : it == 1 ? wide - q : it == 2 ? (wide >> 64) << 64
                                                                          : (((u128)next() << 64) | next()) & wide;
                        if (mk::reduce_wide((u64)(x >> 64), (u64)x, lc) != (u64)(x % q)) fail("reduce_wide", q);
                    }
                    // reduce_cols / reduce_cols_lazy: 1..4 products a b, a < 2^60, b < q; reduce_cols4: 5..8 of them.
                    // Round 0 of every term count: every product (2^60 - 1) (q - 1)
                    for (int it = 0; it < 4000; ++it) {
                        const int terms = 1 + it % 8;
                        mk::Cols cs{0, 0, 0};
                        mk::Cols4 c4{0, 0, 0, 0};
                        u128 X = 0;
                        for (int t = 0; t < terms; ++t) {
                            const u64 a = (it < 8 || it % 5 == 0) ? (1ull << 60) - 1 : next() >> 4;
                            const u64 b = (it < 8 || it % 3 == 0) ? q - 1 : next() % q;
                            uint32_t a0, a1, b0, b1;
                            mk::split30(a, a0, a1);
                            mk::split30(b, b0, b1);
                            if (terms <= 4) mk::mac_cols(cs, a0, a1, b0, b1);
                            else mk::mac_cols4(c4, a0, a1, b0, b1);
                            X += (u128)a * b;
                        }
                        if (terms <= 4) {
                            const u64 lazy = mk::reduce_cols_lazy(cs, lc);
                            if (lazy >= 4 * q || lazy % q != (u64)(X % q)) fail("reduce_cols_lazy", q);
                            if (mk::reduce_cols(cs, lc) != (u64)(X % q)) fail("reduce_cols", q);
                        } else if (mk::reduce_cols4(c4, lc) != (u64)(X % q)) fail("reduce_cols4", q);
                    }
                    // shoup_lazy: any 64-bit a, result below 2q
                    const u64 as[] = {0, q - 1, 2 * q - 1, 4 * q - 1, ~(u64)0};
                    for (int it = 0; it < 2000; ++it) {
                        const u64 w = it == 0 ? 0 : it == 1 ? 1 : it == 2 ? q - 1 : next() % q, wp = mk::h_shoup(w, q);
                        for (u64 a : as) {
                            const u64 r = mk::shoup_lazy(a, w, wp, q);
                            if (r >= 2 * q || r % q != (u64)((u128)a * w % q)) fail("shoup_lazy", q);
                        }
                        const u64 a = next(), r = mk::shoup_lazy(a, w, wp, q);
                        if (r >= 2 * q || r % q != (u64)((u128)a * w % q)) fail("shoup_lazy", q);
                        if (mk::shoup_mul(a, w, wp, q) != (u64)((u128)a * w % q)) fail("shoup_mul", q);
                    }
                    checked += 2009 + 2000 + 2006 + 2000 + 4000 + 2000 * 7;
                }
            }
            for (uint32_t k : {18u, 20u, 30u, 45u, 52u, 55u, 60u})
                if (!(widths >> k & 1)) throw std::runtime_error("no modulus of " + std::to_string(k) + " bits");
            std::printf("ok Barrett arithmetic (%llu moduli, %llu checks)\n", moduli, checked);
        }
        mk::ParamSet bad;
        try {
            bad.generate(30, 1, 40, 60, 2, 60, 20);
            std::printf("unexpected: log_n=30 accepted\n");
            return 1;
        } catch (const std::invalid_argument &) {
            std::printf("ok invalid parameters are refused\n");
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "ERROR: %s\n", e.what());
        return 1;
    }
    return 0;
}
