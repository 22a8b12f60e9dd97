// cheb_selftest -- the Chebyshev bookkeeping of evalPoly --cheb (poly.hpp: the interval, the fit, the block rewrite, the
// headroom rule) as a stand-alone program without the library; built plain and under -fsanitize=address,undefined
// (Makefile), run by tests/test_cheb_cli.py.
#include <cstdio>

#include "poly.hpp"
using namespace mkh;

static int failures = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                           \
        }                                                         \
    } while (0)

// T_0(u) .. T_n(u) by the ladder rule of mkckks.h: T_k = 2 T_i T_j - T_{i-j}, i = ceil(k / 2), j = k - i
static std::vector<double> ladder(double u, uint32_t n) {
    std::vector<double> T = {1.0, u};
    for (uint32_t k = 2; k <= n; ++k) {
        const uint32_t i = (k + 1) / 2, j = k - i;
        T.push_back(2.0 * T[i] * T[j] - T[i - j]);
    }
    return T;
}

int main() {
    // --cheb a,b
    double a = 0, b = 0;
    CHECK(parse_interval("-1,1", a, b).empty() && a == -1.0 && b == 1.0 && !cheb_mapped(a, b));
    CHECK(parse_interval("0.25,4", a, b).empty() && a == 0.25 && b == 4.0 && cheb_mapped(a, b));
    CHECK(parse_interval("-1,1.0000001", a, b).empty() && cheb_mapped(a, b));
    CHECK(parse_interval("1e-3,2.5e1", a, b).empty() && a == 1e-3 && b == 25.0);
    for (const char *bad : {"", "1", "1,", ",1", "1,1", "2,1", "a,b", "1,2,3", "1,2x", "nan,1", "0,inf", "1 2"})
        CHECK(!parse_interval(bad, a, b).empty());
    // the limbs a series needs: those of the polynomial of its degree, one more when the interval is mapped
    for (uint32_t d = POLY_MIN_DEGREE; d <= POLY_MAX_DEGREE; ++d) {
        const PolyPlan p = poly_plan(d);
        CHECK(cheb_fit_error(d, p.depth + 1, false).empty() && !cheb_fit_error(d, p.depth, false).empty());
        CHECK(cheb_fit_error(d, p.depth + 2, true).empty() && !cheb_fit_error(d, p.depth + 1, true).empty());
    }
    CHECK(cheb_fit_error(3, 3, false) == "degree 3 needs 4 limbs (depth 3 and one limb for the result), the input has 3");
    CHECK(cheb_fit_error(3, 4, true) ==
          "degree 3 needs 5 limbs (depth 4, the map onto [-1, 1] included, and one limb for the result), the input has 4");
    // --function
    CHECK(cheb_function("invsqrt") && cheb_function("sigmoid") && cheb_function("tanh") && cheb_function("exp") && !cheb_function("cos"));
    CHECK(cheb_function_error("tanh", 15, -1, 1).empty() && cheb_function_error("invsqrt", 31, 0.25, 4).empty());
    CHECK(!cheb_function_error("invsqrt", 31, 0.0, 4).empty() && !cheb_function_error("invsqrt", 31, -1, 4).empty());
    CHECK(!cheb_function_error("cos", 15, -1, 1).empty() && !cheb_function_error("tanh", 1, -1, 1).empty() &&
          !cheb_function_error("tanh", 64, -1, 1).empty());
    CHECK(cheb_function("sigmoid")(0.0) == 0.5 && cheb_function("invsqrt")(4.0) == 0.5 && cheb_function("exp")(0.0) == 1.0);
    // the fit interpolates: at its own nodes it is the function, and its error on the interval is the known one (the
    // interpolant of 1 / sqrt(t) on [0.25, 4]: 3.0e-4 at d = 15, 6.1e-8 at d = 31, 7.5e-14 at d = 63)
    const double pi = 3.14159265358979323846;
    const struct { uint32_t d; double lo, hi; } known[] = {{15, 2.5e-4, 3.5e-4}, {31, 5.0e-8, 7.0e-8}, {63, 1.0e-14, 3.0e-13}};
    for (const auto &kn : known) {
        const std::vector<double> c = cheb_fit(cheb_function("invsqrt"), 0.25, 4.0, kn.d);
        CHECK(c.size() == kn.d + 1);
        for (uint32_t k = 0; k <= kn.d; ++k) {
            const double u = std::sin(0.5 * pi / (kn.d + 1) * (2.0 * k - kn.d)), t = 0.5 * (3.75 * u + 4.25);
            CHECK(std::fabs(cheb_value(c, u) - 1.0 / std::sqrt(t)) < 1e-13);
        }
        double worst = 0;
        for (int s = 0; s <= 20000; ++s) {
            const double t = 0.25 + 3.75 * s / 20000.0, u = (2.0 * t - 4.25) / 3.75;
            worst = std::max(worst, std::fabs(cheb_value(c, u) - 1.0 / std::sqrt(t)));
        }
        CHECK(worst > kn.lo && worst < kn.hi);
        double sum = 0;
        for (double v : c) sum += std::fabs(v);
        CHECK(sum < 2.5);  // where the power basis has coefficients of 5.0, 9.3e2 and 3.6e8
    }
    {  // tanh is odd: the even coefficients vanish to rounding; a constant fits exactly
        const std::vector<double> c = cheb_fit(cheb_function("tanh"), -1.0, 1.0, 15);
        for (uint32_t k = 0; k <= 15; k += 2) CHECK(std::fabs(c[k]) < 1e-15);
        CHECK(std::fabs(c[1] - 0.811675685131559) < 1e-14);
        const std::vector<double> one = cheb_fit([](double) { return 1.0; }, -3.0, 5.0, 7);
        CHECK(std::fabs(one[0] - 1.0) < 1e-15);
        for (uint32_t k = 1; k <= 7; ++k) CHECK(std::fabs(one[k]) < 1e-15);
    }
    // the ladder rule is the Chebyshev polynomials: T_k(cos x) = cos(k x)
    for (double x : {0.1, 0.7, 1.3, 2.9}) {
        const std::vector<double> T = ladder(std::cos(x), 63);
        for (uint32_t k = 0; k <= 63; ++k) CHECK(std::fabs(T[k] - std::cos(k * x)) < 1e-12);
    }
    // the rewrite: sum_j sum_i m_{j,i} T_i T_{jB} is the series, on every degree; a zero series gives zeros
    for (uint32_t d = POLY_MIN_DEGREE; d <= POLY_MAX_DEGREE; ++d) {
        const PolyPlan p = poly_plan(d);
        std::vector<double> c(d + 1);
        for (uint32_t k = 0; k <= d; ++k) c[k] = std::sin(1.0 + 0.37 * k * (d + 1));  // fixed values in [-1, 1]
        const std::vector<double> m = cheb_rewrite(c, p.B, p.G);
        CHECK(m.size() == (size_t)p.B * p.G);
        for (double u : {-1.0, -0.6, 0.0, 0.3, 0.99, 1.0}) {
            const std::vector<double> T = ladder(u, p.B * p.G);
            double got = 0;
            for (uint32_t j = 0; j < p.G; ++j)
                for (uint32_t i = 0; i < p.B; ++i) got += m[j * p.B + i] * T[i] * T[j * p.B];
            CHECK(std::fabs(got - cheb_value(c, u)) < 1e-11);
        }
        for (double v : cheb_rewrite(std::vector<double>(d + 1, 0.0), p.B, p.G)) CHECK(v == 0.0);
    }
    {  // a known rewrite, degree 3 (B = G = 2): T_3 = 2 T_1 T_2 - T_1
        const std::vector<double> m = cheb_rewrite({0.5, 0.25, -1.0, 3.0}, 2, 2);
        CHECK(m[0] == 0.5 && m[1] == 0.25 - 3.0 && m[2] == -1.0 && m[3] == 6.0);
    }
    // headroom: Sigma = 2^120 and sum |m| = 2 need 121 bits below log2 q - 1
    const std::vector<double> two = {1.0, -0.5, 0.25, -0.25};
    double need = 0;
    CHECK(cheb_headroom_error(two, 120.0, 140.0, &need).empty() && need == 121.0);
    CHECK(cheb_headroom_error(two, 120.0, 122.5, nullptr).empty() && !cheb_headroom_error(two, 120.0, 122.0, nullptr).empty());
    CHECK(cheb_headroom_error(two, 120.0, 100.0, nullptr).find("no headroom") != std::string::npos);
    CHECK(cheb_headroom_error({0.0, 0.0, 0.0, 0.0}, 120.0, 10.0, nullptr).empty());  // the zero series needs nothing
    if (failures) {
        std::printf("cheb selftest: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("cheb selftest ok\n");
    return 0;
}
