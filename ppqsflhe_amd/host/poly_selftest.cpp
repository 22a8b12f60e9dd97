// poly_selftest -- the header bookkeeping of evalPoly (poly.hpp) as a stand-alone program without the library; built
// plain and under -fsanitize=address,undefined (Makefile), run by tests/test_poly_surface.py.
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

int main() {
    // the plan on every degree: B the smallest power of two with B^2 >= d + 1, G = ceil((d + 1) / B), 2 <= G <= B
    for (uint32_t d = POLY_MIN_DEGREE; d <= POLY_MAX_DEGREE; ++d) {
        const PolyPlan p = poly_plan(d);
        CHECK(p.B == 2 || p.B == 4 || p.B == 8);
        CHECK(p.B * p.B >= d + 1 && (p.B == 2 || (p.B / 2) * (p.B / 2) < d + 1));
        CHECK(p.G >= 2 && p.G <= p.B && p.B * p.G >= d + 1 && p.B * (p.G - 1) < d + 1);
        CHECK(p.depth == poly_ceil_log2(p.B) + poly_ceil_log2(p.G - 1) + 2);
        CHECK(p.n_relin == (p.B - 1) + (p.G - 2) + 1 && (d < 8 || p.n_relin < d - 1));  // fewer than Horner's d - 1 from d = 8 on
        CHECK(poly_fit_error(d, p.depth + 1).empty() && !poly_fit_error(d, p.depth).empty() && !poly_fit_error(d, 0).empty());
    }
    CHECK(poly_ceil_log2(1) == 0 && poly_ceil_log2(2) == 1 && poly_ceil_log2(3) == 2 && poly_ceil_log2(7) == 3 && poly_ceil_log2(8) == 3);
    // known plans: d = 3 -> B 2, G 2, depth 3; d = 15 -> B 4, G 4, depth 6, 6 relinearisations; d = 63 -> B 8, G 8, depth 8
    PolyPlan p = poly_plan(3);
    CHECK(p.B == 2 && p.G == 2 && p.depth == 3 && p.n_relin == 2);
    p = poly_plan(15);
    CHECK(p.B == 4 && p.G == 4 && p.depth == 6 && p.n_relin == 6);
    p = poly_plan(63);
    CHECK(p.B == 8 && p.G == 8 && p.depth == 8 && p.n_relin == 14);
    p = poly_plan(16);
    CHECK(p.B == 8 && p.G == 3 && p.depth == 6);
    CHECK(poly_fit_error(3, 3) == "degree 3 needs 4 limbs (depth 3 and one limb for the result), the input has 3");
    // the header of the result
    ProductMeta in;
    in.nl = 4; in.level = 1; in.noise_deg = 1; in.slots = 512; in.scale = 1.0e12;
    const ProductMeta r = poly_result(in, poly_plan(3), 1.1e12);
    CHECK(r.nl == 1 && r.level == 4 && r.noise_deg == 1 && r.slots == 512 && r.scale == 1.1e12);
    // --coeffs
    std::vector<double> c;
    CHECK(parse_coeffs("0,1,0,-0.3333", c).empty() && c.size() == 4 && c[1] == 1.0 && c[3] == -0.3333);
    CHECK(parse_coeffs("1e-3,2.5,-7", c).empty() && c.size() == 3 && c[0] == 1e-3);
    CHECK(parse_coeffs("1,2,0", c).empty() && c.size() == 3);  // a zero leading coefficient keeps its place
    CHECK(!parse_coeffs("", c).empty() && !parse_coeffs("1", c).empty() && !parse_coeffs("1,2", c).empty());
    CHECK(!parse_coeffs("1,,2", c).empty() && !parse_coeffs("1,2,", c).empty() && !parse_coeffs(",1,2", c).empty());
    CHECK(!parse_coeffs("1,2,x", c).empty() && !parse_coeffs("1,2,3x", c).empty() && !parse_coeffs("1,nan,3", c).empty());
    CHECK(!parse_coeffs("1,inf,3", c).empty() && !parse_coeffs("1,1e999,3", c).empty() && !parse_coeffs("1, ,3", c).empty());
    std::string big = "1";
    for (int i = 0; i < 63; ++i) big += ",1";
    CHECK(parse_coeffs(big, c).empty() && c.size() == 64);
    CHECK(parse_coeffs(big + ",1", c).find("[2, 63]") != std::string::npos);
    // headroom: Sigma = 2^120 and sum |c_k| = 2 need 121 bits below log2 q - 1
    const std::vector<double> ones = {1.0, -0.5, 0.25, -0.25};
    CHECK(poly_headroom_error(ones, 1.0, 120.0, 140.0).empty());
    CHECK(poly_headroom_error(ones, 1.0, 120.0, 122.5).empty() && !poly_headroom_error(ones, 1.0, 120.0, 122.0).empty());
    CHECK(!poly_headroom_error(ones, 1.0e6, 120.0, 140.0).empty() && poly_headroom_error(ones, 8.0, 120.0, 140.0).empty());
    CHECK(poly_headroom_error(ones, 1.0, 120.0, 100.0).find("no headroom") != std::string::npos);
    CHECK(!poly_headroom_error(ones, 0.0, 120.0, 140.0).empty() && !poly_headroom_error(ones, -1.0, 120.0, 140.0).empty());
    CHECK(!poly_headroom_error(ones, std::nan(""), 120.0, 140.0).empty() && !poly_headroom_error(ones, 1e300, 120.0, 140.0).empty());
    CHECK(poly_headroom_error({0.0, 0.0, 0.0}, 1.0, 120.0, 10.0).empty());  // the zero polynomial needs nothing
    if (failures) {
        std::printf("poly selftest: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("poly selftest ok\n");
    return 0;
}
