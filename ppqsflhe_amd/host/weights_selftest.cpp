// weights_selftest -- stand-alone checks of the weighted aggregation's host arithmetic, built plain and under
// AddressSanitizer + UBSan (make weights-asan; driven by tests/test_weighted_surface.py):
//   * ParamSet::const_factors_qp against 128-bit arithmetic on all D limbs of QP, its agreement with const_factors on the
//     Q limbs, and const_fits at the edges of what the 128-bit conversion can hold;
//   * parse_weights (weights.hpp) on well-formed and hostile --weights values.
// Needs no device and no library: it compiles params.cpp itself.
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>

#include "../csrc/params.hpp"
#include "weights.hpp"

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static void check_constants(uint32_t log_n, uint32_t depth, uint32_t sbits, uint32_t dnum) {
    mk::ParamSet ps;
    ps.generate(log_n, depth, sbits, 60, dnum, 60, 20);
    const double weights[] = {0.0, 1.0, 0.5, 5.0 / 17.0, 1.0 / 3.0, 1e-9, 1234.5678, -0.25, 3.0e9};
    for (uint32_t level = 0; level < ps.L; ++level)
        for (double w : weights) {
            EXPECT(ps.const_fits(level, w));
            const std::vector<mk::u64> f = ps.const_factors_qp(level, w);
            EXPECT(f.size() == ps.D);
            // sf < 2^61 here, so the product is far below 2^125 and the integer is trunc(w * sf + 0.5) itself
            const __int128 big = (__int128)(w * ps.sf[level] + 0.5);
            for (uint32_t i = 0; i < ps.D; ++i) {
                __int128 r = big % (__int128)ps.moduli[i];
                if (r < 0) r += (__int128)ps.moduli[i];
                EXPECT(f[i] == (mk::u64)r);
                EXPECT(f[i] < ps.moduli[i]);
            }
            for (uint32_t nl = 1; nl <= ps.L; ++nl) {
                const std::vector<mk::u64> g = ps.const_factors(nl, level, w);
                for (uint32_t i = 0; i < nl; ++i) EXPECT(g[i] == f[i]);
            }
        }
    // the edges: not finite, and constants at / beyond 125 bits
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double edge = std::ldexp(1.0, 125) / ps.sf[1];
    EXPECT(!ps.const_fits(1, inf) && !ps.const_fits(1, -inf) && !ps.const_fits(1, nan));
    EXPECT(!ps.const_fits(1, edge * 1.0001) && !ps.const_fits(1, -edge * 1.0001) && !ps.const_fits(1, 1e300));
    EXPECT(ps.const_fits(1, edge * 0.999) && ps.const_fits(1, -edge * 0.999));
    EXPECT(!ps.const_fits(ps.L + 100, 0.5));  // no such scaling-factor level
    (void)ps.const_factors_qp(1, edge * 0.999);
    (void)ps.const_factors_qp(1, -edge * 0.999);
    for (double bad : {inf, nan, edge * 1.0001, 1e300}) {
        bool threw = false;
        try {
            (void)ps.const_factors_qp(1, bad);
        } catch (const std::invalid_argument &) {
            threw = true;
        }
        EXPECT(threw);
    }
    std::printf("ok constants log_n=%u L=%u D=%u\n", log_n, ps.L, ps.D);
}

static bool parses(const char *text, size_t n, std::vector<double> *out = nullptr) {
    std::vector<double> w;
    const std::string err = mkh::parse_weights(text, n, w);
    if (!err.empty()) return false;
    if (out) *out = w;
    double sum = 0;
    for (double v : w) {
        EXPECT(v >= 0 && v <= 1);
        sum += v;
    }
    EXPECT(w.size() == n && std::fabs(sum - 1.0) < 1e-12);
    return true;
}

static void check_parser() {
    std::vector<double> w;
    EXPECT(parses("3,1,4", 3, &w) && w[0] == 3.0 / 8 && w[1] == 1.0 / 8 && w[2] == 4.0 / 8);
    EXPECT(parses("1", 1, &w) && w[0] == 1.0);
    EXPECT(parses("0,0,2.5e3", 3, &w) && w[0] == 0 && w[2] == 1.0);
    EXPECT(parses("1e308,1e308", 2, &w) && w[0] == 0.5);           // the sum of the raw values overflows
    EXPECT(parses("5e-324,5e-324", 2, &w) && w[0] == 0.5);         // denormals
    EXPECT(parses("-0,1", 2, &w) && w[0] == 0.0);
    EXPECT(parses("+1,.5,5.", 3));
    EXPECT(!parses("", 1) && !parses(",", 2) && !parses("1,", 2) && !parses(",1", 2) && !parses("1,,2", 3));
    EXPECT(!parses("1,2", 3) && !parses("1,2,3", 2) && !parses("1", 0));
    EXPECT(!parses("-1,2", 2) && !parses("1,-1e-300", 2));
    EXPECT(!parses("nan,1", 2) && !parses("inf,1", 2) && !parses("1e999,1", 2) && !parses("0x10,1", 2));
    EXPECT(!parses("1 ,2", 2) && !parses(" 1,2", 2) && !parses("1;2", 2) && !parses("a,b", 2) && !parses("1e,2", 2));
    EXPECT(!parses("0,0,0", 3) && !parses("0", 1));
    EXPECT(!parses(std::string(100000, '1').c_str(), 1));           // one endless token
    std::string many;
    for (int i = 0; i < 200000; ++i) many += "1,";
    EXPECT(!parses(many.c_str(), 3));
    // the messages the hosts print
    EXPECT(mkh::parse_weights("1,2", 3, w).find("2 value(s) for 3 client(s)") != std::string::npos);
    EXPECT(mkh::parse_weights("1,-2,3", 3, w).find("negative") != std::string::npos);
    EXPECT(mkh::parse_weights("1,x,3", 3, w).find("non-negative numbers") != std::string::npos);
    EXPECT(mkh::parse_weights("0,0,0", 3, w).find("all be zero") != std::string::npos);
    std::printf("ok parser\n");
}

int main() {
    check_constants(10, 3, 40, 2);
    check_constants(14, 2, 40, 2);
    check_constants(12, 10, 50, 3);
    check_parser();
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok weights selftest\n");
    return 0;
}
