// pm_glue_selftest -- the pseudo-Mersenne primitives of modarith.hpp (pm_lazy, pm_fold, pm_reduce128, pm_reduce_cols,
// csub, mac128) against the formulas they replaced and against unsigned __int128 arithmetic, on the host (`make
// asan` builds it under -fsanitize=address,undefined; tests/test_pm_glue.py runs it).
//
// The device forms were rewritten to spend fewer instructions between the multiplies (carry-out of the multiplier instead
// of word splitting, chained multiply-adds).  Every lazy bound of the transforms and every stored bit rests on each
// primitive returning the SAME 64-bit word as before, not merely the same residue; the formulas of the parent are kept
// here verbatim (namespace old) and compared word for word.  The device code itself is compared on the GPU by
// tools/ubench_fpmod.hip and by the parity suite.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <vector>

#include "params.hpp"

namespace old {  // modarith.hpp before the rewrite, host branches, verbatim
using mk::Cols;
using mk::PmK;
using mk::u128;
using mk::u64;
inline void mul128(u64 a, u64 b, u64 &hi, u64 &lo) {
    u128 p = (u128)a * b;
    lo = (u64)p;
    hi = (u64)(p >> 64);
}
inline u64 csub(u64 x, u64 m) {
    const u64 t = x + (0 - m);
    return (int64_t)t < 0 ? x : t;
}
inline u64 pm_fold(u64 x, const PmK &P) {
    const uint32_t xh = (uint32_t)(x >> 32);
    const u64 lo = ((u64)(xh & P.m_f) << 32) | (uint32_t)x;
    return (u64)(xh >> P.s_f) * P.c + lo;
}
inline u64 hi32_pair(u64 y) { return y >> 32; }
inline u64 pm_lazy(u64 a, u64 wt, u64 wxt, const PmK &P) {
    const uint32_t a0 = (uint32_t)a, a1 = (uint32_t)(a >> 32);
    const u64 y0 = (u64)a0 * (uint32_t)wt;
    u64 z = (u64)a0 * (uint32_t)(wt >> 32) + hi32_pair(y0);
    const u64 y1 = (u64)a1 * (uint32_t)wxt + (u64)(uint32_t)y0;
    z = (u64)a1 * (uint32_t)(wxt >> 32) + z;
    z += hi32_pair(y1);
    const u64 lo = (((u64)(uint32_t)z << 32) | (uint32_t)y1) >> P.t;
    return (u64)(uint32_t)(z >> 32) * P.c2 + lo;
}
inline u64 pm_reduce128(u64 hi, u64 lo, const PmK &P, u64 q) {
    const u64 m0 = (u64)(uint32_t)hi * P.c64 + (u64)(uint32_t)lo;
    u64 m1 = (u64)(uint32_t)(hi >> 32) * P.c64 + hi32_pair(lo);
    m1 += hi32_pair(m0);
    const uint32_t yh = (uint32_t)(m1 >> P.s_f);
    const u64 ylo = ((u64)((uint32_t)m1 & P.m_f) << 32) | (uint32_t)m0;
    return csub((u64)yh * P.c + ylo, q);
}
inline u64 pm_reduce_cols(const Cols &c, const PmK &P) {
    const u64 t = c.c2 + (c.c1 >> 30);
    const u64 m0 = (u64)(uint32_t)t * P.e60;
    const u64 m1 = (u64)(uint32_t)(t >> 32) * P.e60 + hi32_pair(m0);  // T = m1 2^32 + low word of m0
    const uint32_t yh = (uint32_t)(m1 >> P.s_f);
    const u64 ylo = ((u64)((uint32_t)m1 & P.m_f) << 32) | (uint32_t)m0;
    const u64 a = c.c0 + ((c.c1 & 0x3FFFFFFFull) << 30);
    return (u64)yh * P.c + ylo + old::pm_fold(a, P);  // (qualified: PmK would also find mk::pm_fold)
}
inline void mac128(u64 &hi, u64 &lo, u64 a, u64 b) {
    u64 ph, pl;
    mul128(a, b, ph, pl);
    lo += pl;
    hi += ph + (lo < pl ? 1 : 0);
}
}  // namespace old

namespace {
using mk::u128;
using mk::u64;

struct Counts {
    unsigned long long lazy = 0, carry1 = 0, carry0 = 0, fold = 0, red128 = 0, cols = 0, csub = 0, mac = 0;
};

[[noreturn]] void fail(const char *what, u64 q) { throw std::runtime_error(std::string(what) + " at q = " + std::to_string(q)); }

void check_prime(const mk::LimbConst &lc_in, Counts &n, u64 &rng) {
    auto next = [&]() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
    mk::LimbConst lc = lc_in;
    const u64 q = lc.q;
    lc.pm = 1;
    lc.pm_c = (uint32_t)(((u64)1 << lc.k) - q);
    const mk::PmK P = mk::pm_consts(lc);
    const u64 U = (u64)1 << lc.k, amax = (U << 3) - 1;  // pm_lazy takes a < 8U

    // ---- pm_lazy -------------------------------------------------------------------------------------------------------
    auto lazy = [&](u64 a, u64 w) {
        const u64 wt = mk::pm_tw(w, lc), wxt = mk::pm_tw_companion(w, lc);
        const u64 r = mk::pm_lazy(a, wt, wxt, P);
        if (r != old::pm_lazy(a, wt, wxt, P)) fail("pm_lazy: word differs from the earlier formula", q);
        if (r % q != (u64)((u128)a * w % q)) fail("pm_lazy: wrong residue", q);
        if ((u128)r * 8 >= (u128)U * 19) fail("pm_lazy: result not below 2.375 * 2^k", q);
        // the carry the device form takes from the multiplier: bit 64 of a_lo wt_lo + a_hi wxt_lo
        const u128 low = (u128)(uint32_t)a * (uint32_t)wt + (u128)(uint32_t)(a >> 32) * (uint32_t)wxt;
        if (low >> 65) fail("pm_lazy: low sum above 2^65", q);
        ((low >> 64) ? n.carry1 : n.carry0)++;
        ++n.lazy;
    };
    // boundary words: the largest a; the largest low word with the largest high word the range allows (2^31 - 1 at k = 60);
    // a full low word alone; a full high word alone
    const u64 a_hi_max = amax >> 32;
    const u64 as[] = {amax, (a_hi_max << 32) | 0xffffffffull, 0xffffffffull, a_hi_max << 32, 0, 1, q - 1, q, U - 1, U,
                      amax - 1, 0x100000000ull};
    // w = q - 1 (with its companion), small w, w with full low / high words
    const u64 ws[] = {q - 1, 0, 1, q / 2, 0xffffffffull, 0x100000000ull, q - 0xffffffffull, q - 2};
    for (u64 a : as)
        for (u64 w : ws) lazy(a, w);
    for (int it = 0; it < 1000000; ++it) lazy(next() & amax, next() % q);

    // ---- pm_fold: any 64-bit word ----------------------------------------------------------------------------------------
    auto fold = [&](u64 x) {
        const u64 f = mk::pm_fold(x, P);
        if (f != old::pm_fold(x, P)) fail("pm_fold: word differs from the earlier formula", q);
        if (f % q != x % q || f >= U + (1ull << 30)) fail("pm_fold", q);
        ++n.fold;
    };
    for (u64 x : {(u64)0, q, U, ~(u64)0, ~(u64)0 - 1, U - 1, amax, q - 1, (u64)0xffffffffull, (u64)0x100000000ull}) fold(x);
    for (int it = 0; it < 1000000; ++it) fold(next());

    // ---- mac128 + pm_reduce128: accumulators of up to six products (lazy word < 8U) x (residue < q) -----------------------
    auto acc6 = [&](int terms, bool amaxed, bool bmaxed) {
        u128 X = 0;
        u64 hi = 0, lo = 0, ohi = 0, olo = 0;
        for (int t = 0; t < terms; ++t) {
            const u64 a = amaxed ? amax : (next() & amax), b = bmaxed ? q - 1 : next() % q;
            X += (u128)a * b;
            mk::mac128(hi, lo, a, b);
            old::mac128(ohi, olo, a, b);
            if (hi != ohi || lo != olo) fail("mac128: words differ from the earlier formula", q);
            if (hi != (u64)(X >> 64) || lo != (u64)X) fail("mac128: wrong sum", q);
            ++n.mac;
        }
        const u64 r = mk::pm_reduce128(hi, lo, P, q);
        if (r != old::pm_reduce128(hi, lo, P, q)) fail("pm_reduce128: word differs from the earlier formula", q);
        if (r != (u64)(X % q)) fail("pm_reduce128: wrong residue", q);
        ++n.red128;
    };
    for (int terms = 1; terms <= 6; ++terms) acc6(terms, true, true);  // terms = 6: six maximal products
    for (int it = 0; it < 1000000 / 4; ++it) acc6(1 + it % 6, it % 5 == 0, it % 7 == 0);
    // mac128 on any accumulator that leaves room for the product, and pm_reduce128 with a low word that makes the
    // multiplier carry (lo close to 2^64)
    for (int it = 0; it < 200000; ++it) {
        u64 hi = next() >> 4, lo = it % 3 == 0 ? ~(u64)0 - (next() & 0xffff) : next();
        u64 ohi = hi, olo = lo;
        const u128 X = (((u128)hi << 64) | lo) + (u128)amax * (q - 1);
        mk::mac128(hi, lo, amax, q - 1);
        old::mac128(ohi, olo, amax, q - 1);
        if (hi != ohi || lo != olo || hi != (u64)(X >> 64) || lo != (u64)X) fail("mac128 (carry into the high word)", q);
        ++n.mac;
        // X < 2^(2k+6) is the range of pm_reduce128
        const u64 h2 = next() >> (122 - 2 * lc.k), l2 = ~(u64)0 - (next() & 0xffffffffull);
        const u64 r = mk::pm_reduce128(h2, l2, P, q);
        if (r != old::pm_reduce128(h2, l2, P, q)) fail("pm_reduce128 (carrying low word): word differs", q);
        if (r != (u64)(((((u128)h2) << 64) | l2) % q)) fail("pm_reduce128 (carrying low word): wrong residue", q);
        ++n.red128;
    }

    // ---- pm_reduce128_wide: any 128-bit value; k_qsum3_int's runs of 31 maximal products on top of a carried residue ------------
    {
        u128 X = q - 1;  // the canonical value carried over from the previous run
        u64 hi = 0, lo = q - 1;
        for (int t = 0; t < 31; ++t) {
            X += (u128)amax * (q - 1);
            mk::mac128(hi, lo, amax, q - 1);
            if (hi != (u64)(X >> 64) || lo != (u64)X) fail("mac128: wrong sum in a run of 31", q);
            if (mk::pm_reduce128_wide(hi, lo, P, q) != (u64)(X % q)) fail("pm_reduce128_wide: wrong residue in a run of 31", q);
        }
        for (u64 h : {(u64)0, (u64)1, (u64)0xffffffffull, (u64)0x100000000ull, ~(u64)0 - 1, ~(u64)0})
            for (u64 l : {(u64)0, q - 1, q, (u64)0xffffffffull, (u64)(~(u64)0 - 0xffffffffull), ~(u64)0})
                if (mk::pm_reduce128_wide(h, l, P, q) != (u64)((((u128)h << 64) | l) % q)) fail("pm_reduce128_wide: boundary words", q);
        for (int it = 0; it < 500000; ++it) {
            const u64 h = next(), l = it % 3 == 0 ? ~(u64)0 - (next() & 0xffffffffull) : next();
            if (mk::pm_reduce128_wide(h, l, P, q) != (u64)((((u128)h << 64) | l) % q)) fail("pm_reduce128_wide: wrong residue", q);
        }
    }

    // ---- pm_reduce_cols: column sums of up to 4 products of 60-bit numbers split in 30-bit halves --------------------------
    for (int it = 0; it < 1000000 / 2; ++it) {
        mk::Cols cs{0, 0, 0};
        u128 X = 0;
        const int terms = it < 4 ? 4 : 1 + it % 4;
        for (int t = 0; t < terms; ++t) {
            const u64 a = (it < 4 || it % 5 == 0) ? (1ull << 60) - 1 : next() >> 4, b = (it < 4 || it % 3 == 0) ? q - 1 : next() % q;
            uint32_t a0, a1, b0, b1;
            mk::split30(a, a0, a1);
            mk::split30(b, b0, b1);
            mk::mac_cols(cs, a0, a1, b0, b1);
            X += (u128)a * b;
        }
        const u64 r = mk::pm_reduce_cols(cs, P);
        if (r != old::pm_reduce_cols(cs, P)) fail("pm_reduce_cols: word differs from the earlier formula", q);
        if (r % q != (u64)(X % q) || r >= 2 * U + (U >> 3)) fail("pm_reduce_cols", q);
        ++n.cols;
    }

    // ---- csub: x, m < 2^63 ----------------------------------------------------------------------------------------------
    auto cs = [&](u64 x, u64 m) {
        const u64 r = mk::csub(x, m);
        if (r != old::csub(x, m) || r != (x >= m ? x - m : x)) fail("csub", q);
        ++n.csub;
    };
    for (u64 m : {q, 2 * q, 4 * q})
        for (u64 x : {(u64)0, m - 1, m, m + 1, 2 * m - 1, (u64)((1ull << 63) - 1)}) cs(x, m);
    for (int it = 0; it < 1000000; ++it) cs(next() >> 1, it & 1 ? q : 2 * q);
}
}  // namespace

int main() {
    struct Cfg { uint32_t log_n, depth, sbits, first, dnum, aux; };
    try {
        Counts n;
        u64 rng = 0x9E3779B97F4A7C15ull;
        unsigned primes = 0;
        u64 widths = 0;
        // the reference context (N = 2^14, depth 2, 40-bit scaling, dnum 2: q0 and the special primes are 60-bit
        // pseudo-Mersenne primes), then contexts whose first modulus has 55 and 58 bits
        for (const Cfg &c : {Cfg{14, 2, 40, 60, 2, 60}, Cfg{14, 2, 40, 55, 2, 60}, Cfg{14, 2, 40, 58, 2, 60}}) {
            mk::ParamSet ps;
            ps.generate(c.log_n, c.depth, c.sbits, c.first, c.dnum, c.aux, 20);
            for (uint32_t i = 0; i < ps.D; ++i) {
                const mk::LimbConst &lc = ps.limb[i];
                if (!mk::pm_eligible(lc.q)) continue;
                if (c.first == 60 ? lc.k != 60 : lc.k != c.first) continue;  // 60-bit primes once, from the reference context
                check_prime(lc, n, rng);
                widths |= (u64)1 << lc.k;
                ++primes;
                std::printf("ok q=%llu (%u bits)\n", (unsigned long long)lc.q, lc.k);
            }
        }
        for (uint32_t k : {55u, 58u, 60u})
            if (!(widths >> k & 1)) throw std::runtime_error("no pseudo-Mersenne prime of " + std::to_string(k) + " bits");
        if (!n.carry1 || !n.carry0) throw std::runtime_error("pm_lazy: the carry was never 1 or never 0");
        std::printf("ok pm glue: %u primes, pm_lazy %llu (carry 1: %llu, carry 0: %llu), pm_fold %llu, mac128 %llu, "
                    "pm_reduce128 %llu, pm_reduce_cols %llu, csub %llu\n",
                    primes, n.lazy, n.carry1, n.carry0, n.fold, n.mac, n.red128, n.cols, n.csub);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "ERROR: %s\n", e.what());
        return 1;
    }
    return 0;
}
