// bsgs_selftest -- stand-alone checks of the baby-step giant-step plan of linearTransform --bsgs (bsgs.hpp), built plain
// and under AddressSanitizer + UBSan (make bsgs-asan; driven by tests/test_bsgs_plan.py):
//   * the step rule: reduction to (-slots/2, slots/2], the floor modulus, values of a repeated step summed, steps at
//     +-slots/2; `auto` on the steps of a 128 x 128 block (n1 = 16, 30 keys) and of a 4 x 4 block (n1 = 4: 1,2,3,-4);
//   * the plan applied by its own formula sum_G rot_G(sum_b p_{G,b} * rot_b(x)) equals the diagonal method on the slots;
//   * the refusals: a plan above 64 baby or giant steps (with the counts), an n1 that is no number.
// `bsgs_selftest plan <slots> <n1|auto> <diagonals.json>` prints the plan of a diagonals file as JSON (n1, giants, present,
// steps, values), for a comparison of the roll with numpy.
// Needs no device and no library.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "bsgs.hpp"

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

using mkh::BsgsPlan;
using mkh::Diagonals;

static Diagonals make(const std::vector<int32_t> &steps, size_t slots, unsigned seed) {
    Diagonals d;
    d.steps = steps;
    d.values.resize(steps.size() * slots);
    uint32_t x = seed * 2654435761u + 1u;
    for (double &v : d.values) {
        x = x * 1664525u + 1013904223u;
        v = (double)(x >> 8) / (double)(1u << 24) - 0.5;
    }
    mkh::diagonals_finish(d, slots);
    return d;
}

static std::vector<double> rot(const std::vector<double> &x, long long r) {
    const long long S = (long long)x.size();
    std::vector<double> y(x.size());
    for (long long j = 0; j < S; ++j) y[(size_t)j] = x[(size_t)mkh::bsgs_floor_mod(j + r, S)];
    return y;
}

// the diagonal method against the plan's own formula
static double plan_error(const Diagonals &d, const BsgsPlan &p, size_t slots) {
    std::vector<double> x(slots), want(slots, 0.0), got(slots, 0.0);
    for (size_t j = 0; j < slots; ++j) x[j] = std::sin(0.37 * (double)j + 0.1);
    for (size_t k = 0; k < d.steps.size(); ++k) {
        const std::vector<double> xr = rot(x, d.steps[k]);
        for (size_t j = 0; j < slots; ++j) want[j] += d.values[k * slots + j] * xr[j];
    }
    for (size_t t = 0; t < p.giants.size(); ++t) {
        std::vector<double> inner(slots, 0.0);
        for (size_t b = 0; b < p.n1; ++b) {
            if (!p.present[t * p.n1 + b]) continue;
            const std::vector<double> xb = rot(x, p.babies[b]);
            for (size_t j = 0; j < slots; ++j) inner[j] += p.values[(t * p.n1 + b) * slots + j] * xb[j];
        }
        const std::vector<double> r = rot(inner, p.giants[t]);
        for (size_t j = 0; j < slots; ++j) got[j] += r[j];
    }
    double e = 0;
    for (size_t j = 0; j < slots; ++j) e = std::fmax(e, std::fabs(got[j] - want[j]));
    return e;
}

static std::vector<int32_t> range(int lo, int hi) {
    std::vector<int32_t> v;
    for (int r = lo; r <= hi; ++r) v.push_back(r);
    return v;
}

static void test_rule() {
    EXPECT(mkh::bsgs_reduce_step(5, 8) == -3 && mkh::bsgs_reduce_step(4, 8) == 4 && mkh::bsgs_reduce_step(-4, 8) == 4);
    EXPECT(mkh::bsgs_reduce_step(-3, 8) == -3 && mkh::bsgs_reduce_step(16, 8) == 0 && mkh::bsgs_reduce_step(-13, 8) == 3);
    EXPECT(mkh::bsgs_floor_mod(-3, 4) == 1 && mkh::bsgs_floor_mod(-4, 4) == 0 && mkh::bsgs_floor_mod(7, 4) == 3);
    BsgsPlan p;
    {  // the 128 x 128 block
        const Diagonals d = make(range(-127, 127), 512, 1);
        EXPECT(mkh::bsgs_plan(d, 512, 0, true, p).empty());
        EXPECT(p.n1 == 16 && p.n_babies == 15 && p.n_giants == 15 && p.key_steps.size() == 30 && p.giants.size() == 16);
        EXPECT(plan_error(d, p, 512) < 1e-12);
        EXPECT(mkh::bsgs_plan(d, 512, 32, false, p).empty() && p.n1 == 32 && p.key_steps.size() == 38 && p.values.empty());
    }
    {  // a 4 x 4 block: the tie between n1 = 2 and n1 = 4 goes to 4
        const Diagonals d = make(range(-3, 3), 64, 2);
        EXPECT(mkh::bsgs_plan(d, 64, 0, true, p).empty());
        EXPECT(p.n1 == 4 && p.key_steps == (std::vector<int32_t>{1, 2, 3, -4}));
        EXPECT(p.giants == (std::vector<int32_t>{-4, 0}));
        EXPECT(p.present == (std::vector<uint8_t>{0, 1, 1, 1, 1, 1, 1, 1}));  // (-4, 0) is step -4: absent
        EXPECT(mkh::bsgs_steps_line(p) == "[lintrans] bsgs n1=4 babies=3 giants=1 steps=1,2,3,-4");
        EXPECT(plan_error(d, p, 64) < 1e-12);
        EXPECT(mkh::bsgs_plan(d, 64, 2, true, p).empty() && p.n1 == 2 && p.giants == (std::vector<int32_t>{-4, -2, 0, 2}));
        EXPECT(plan_error(d, p, 64) < 1e-12);
        EXPECT(mkh::bsgs_plan(d, 64, 1, true, p).empty() && p.giants.size() == 7 && p.n_babies == 0 && plan_error(d, p, 64) < 1e-12);
        EXPECT(mkh::bsgs_plan(d, 64, 3, true, p).empty() && plan_error(d, p, 64) < 1e-12);
    }
    {  // a repeated step (also one that repeats only after the reduction) is summed
        const Diagonals d = make({1, 5, 1, 0, 5 - 16, -2}, 16, 3);
        EXPECT(mkh::bsgs_plan(d, 16, 4, true, p).empty());
        EXPECT(p.giants == (std::vector<int32_t>{-4, 0, 4}) && plan_error(d, p, 16) < 1e-12);
        size_t present = 0;
        for (uint8_t f : p.present) present += f;
        EXPECT(present == 4);  // steps 0, 1, 5, -2
    }
    {  // steps at +-slots/2 are one step
        const Diagonals d = make({8, -8, 7, -7}, 16, 4);
        EXPECT(mkh::bsgs_plan(d, 16, 4, true, p).empty());
        EXPECT(p.giants == (std::vector<int32_t>{-8, 4, 8}) && plan_error(d, p, 16) < 1e-12);
        EXPECT(p.key_steps == (std::vector<int32_t>{1, 3, -8, 4, 8}));
    }
}

static void test_refusals() {
    BsgsPlan p;
    p.n1 = 77;
    const Diagonals d = make(range(-127, 127), 4096, 5);
    std::string err = mkh::bsgs_plan(d, 4096, 2, true, p);
    EXPECT(err.find("2 baby steps and 128 giant steps") != std::string::npos && p.n1 == 77);
    err = mkh::bsgs_plan(d, 4096, 128, false, p);
    EXPECT(err.find("128 baby steps and 2 giant steps") != std::string::npos && err.find("at most 64") != std::string::npos);
    Diagonals none;
    EXPECT(!mkh::bsgs_plan(none, 16, 0, false, p).empty());
    uint32_t n1 = 9;
    EXPECT(mkh::bsgs_parse_n1("auto", n1).empty() && n1 == 0);
    EXPECT(mkh::bsgs_parse_n1("16", n1).empty() && n1 == 16);
    for (const char *bad : {"", "0", "-4", "4x", "x", "99999999999999999999"}) EXPECT(!mkh::bsgs_parse_n1(bad, n1).empty());
}

static int print_plan(size_t slots, const std::string &n1_arg, const std::string &path) {
    Diagonals d;
    uint32_t n1 = 0;
    std::string err = mkh::bsgs_parse_n1(n1_arg, n1);
    if (err.empty()) err = mkh::load_diagonals(path, false, slots, d);
    BsgsPlan p;
    if (err.empty()) err = mkh::bsgs_plan(d, slots, n1, true, p);
    if (!err.empty()) {
        std::printf("ERROR: %s\n", err.c_str());
        return 1;
    }
    std::printf("{\"n1\": %u, \"giants\": [", p.n1);
    for (size_t t = 0; t < p.giants.size(); ++t) std::printf("%s%d", t ? ", " : "", p.giants[t]);
    std::printf("], \"steps\": [");
    for (size_t k = 0; k < p.key_steps.size(); ++k) std::printf("%s%d", k ? ", " : "", p.key_steps[k]);
    std::printf("], \"present\": [");
    for (size_t k = 0; k < p.present.size(); ++k) std::printf("%s%d", k ? ", " : "", (int)p.present[k]);
    std::printf("], \"values\": [");
    for (size_t k = 0; k < p.values.size(); ++k) std::printf("%s%.17g", k ? ", " : "", p.values[k]);
    std::printf("]}\n");
    return 0;
}

int main(int argc, char *argv[]) {
    if (argc == 5 && std::string(argv[1]) == "plan") return print_plan((size_t)std::atol(argv[2]), argv[3], argv[4]);
    test_rule();
    test_refusals();
    if (failures) {
        std::printf("bsgs_selftest: %d failure(s)\n", failures);
        return 1;
    }
    std::printf("bsgs_selftest ok\n");
    return 0;
}
