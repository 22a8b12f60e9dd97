// lintrans_selftest -- stand-alone checks of linearTransform's host code (lintrans.hpp), built plain and under
// AddressSanitizer + UBSan (make lintrans-asan; driven by tests/test_linear_transform_surface.py):
//   * the reader of {"diagonals": [{"step", "values"}]}: zero padding, duplicate and negative steps, a diagonal as long as
//     the slots, and its refusals (no list, an empty list, a step that is no integer or out of range, too many values,
//     values that are not numbers or not finite);
//   * the --block builder: for n = 1, 2, 4 and n = slots the 2n - 1 masked diagonals applied by the diagonal method
//     out[j] = sum_r diag_r[j] in[(j + r) mod slots] equal the dense product of every aligned n-slot block with the matrix,
//     and its refusals (n not a power of two, n above the slots, a ragged row, an entry that is not finite);
//   * max_abs_sum and the headroom rule on both sides of its bound.
// Needs no device and no library.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "lintrans.hpp"

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

using mkh::Diagonals;
using mkh::Json;

static std::string parse(const std::string &text, size_t slots, Diagonals &d, bool block = false) {
    Json doc;
    try {
        doc = Json::parse(text);
    } catch (const std::exception &) {
        return "unparsable";
    }
    return block ? mkh::block_diagonals(doc, slots, d) : mkh::parse_diagonals(doc, slots, d);
}

static void test_reader() {
    Diagonals d;
    EXPECT(parse("{\"diagonals\": [{\"step\": 0, \"values\": [1, 2.5]}, {\"step\": -3, \"values\": []}, "
                 "{\"step\": 0, \"values\": [-4, 0, 0, 1]}]}", 4, d).empty());
    EXPECT(d.steps.size() == 3 && d.steps[0] == 0 && d.steps[1] == -3 && d.steps[2] == 0);
    const double want[12] = {1, 2.5, 0, 0, 0, 0, 0, 0, -4, 0, 0, 1};
    EXPECT(d.values.size() == 12);
    for (size_t i = 0; i < 12 && i < d.values.size(); ++i) EXPECT(d.values[i] == want[i]);
    EXPECT(d.max_abs_sum == 5.0);
    const char *bad[] = {"{}", "{\"diagonals\": 3}", "{\"diagonals\": []}", "{\"diagonals\": [{\"values\": [1]}]}",
                         "{\"diagonals\": [{\"step\": 1.5, \"values\": [1]}]}", "{\"diagonals\": [{\"step\": \"1\", \"values\": [1]}]}",
                         "{\"diagonals\": [{\"step\": 1073741824, \"values\": [1]}]}", "{\"diagonals\": [{\"step\": -1073741824, \"values\": [1]}]}",
                         "{\"diagonals\": [{\"step\": 1, \"values\": 1}]}", "{\"diagonals\": [{\"step\": 1, \"values\": [1, 2, 3, 4, 5]}]}",
                         "{\"diagonals\": [{\"step\": 1, \"values\": [\"x\"]}]}", "{\"diagonals\": [{\"step\": 1, \"values\": [1e999]}]}",
                         "{\"diagonals\": [{\"step\": 1}]}", "[1]"};
    for (const char *t : bad) {
        Diagonals keep;
        keep.steps.push_back(7);
        EXPECT(!parse(t, 4, keep).empty());
        EXPECT(keep.steps.size() == 1 && keep.steps[0] == 7);  // a refusal leaves the output alone
    }
    EXPECT(parse("{\"diagonals\": [{\"step\": 1073741823, \"values\": [1]}]}", 4, d).empty() && d.steps[0] == 1073741823);
}

static void test_block(size_t n, size_t slots) {
    std::string text = "{\"matrix\": [";
    std::vector<double> M(n * n);
    for (size_t i = 0; i < n; ++i) {
        text += i ? ", [" : "[";
        for (size_t c = 0; c < n; ++c) {
            M[i * n + c] = (double)((i * 7 + c * 3) % 11) - 5.0 + 0.25 * (double)c;
            char buf[40];
            std::snprintf(buf, sizeof buf, "%s%.17g", c ? ", " : "", M[i * n + c]);
            text += buf;
        }
        text += "]";
    }
    text += "]}";
    Diagonals d;
    EXPECT(parse(text, slots, d, true).empty());
    EXPECT(d.steps.size() == 2 * n - 1 && d.values.size() == (2 * n - 1) * slots);
    if (d.steps.size() != 2 * n - 1) return;
    std::vector<double> in(slots), out(slots, 0.0);
    for (size_t j = 0; j < slots; ++j) in[j] = 1.0 + (double)((j * 5) % 13);
    double max_sum = 0;
    for (size_t k = 0; k < d.steps.size(); ++k) {
        EXPECT(d.steps[k] == (int32_t)k - (int32_t)(n - 1));
        for (size_t j = 0; j < slots; ++j) {
            const long long src = ((long long)j + d.steps[k]) % (long long)slots;
            out[j] += d.values[k * slots + j] * in[(size_t)((src + (long long)slots) % (long long)slots)];
        }
    }
    for (size_t j = 0; j < slots; ++j) {
        double dense = 0, sum = 0;
        for (size_t c = 0; c < n; ++c) {
            dense += M[(j % n) * n + c] * in[j - j % n + c];
            sum += std::fabs(M[(j % n) * n + c]);
        }
        EXPECT(out[j] == dense);  // small integers and quarters: exact in doubles
        max_sum = std::fmax(max_sum, sum);
    }
    EXPECT(d.max_abs_sum == max_sum);
}

static void test_block_refusals() {
    Diagonals d;
    const char *bad[] = {"{}", "{\"matrix\": []}", "{\"matrix\": 1}", "{\"matrix\": [[1, 2, 3], [4, 5, 6], [7, 8, 9]]}",
                         "{\"matrix\": [[1, 2], [3]]}", "{\"matrix\": [[1, 2], 3]}", "{\"matrix\": [[1, \"x\"], [3, 4]]}",
                         "{\"matrix\": [[1, 1e999], [3, 4]]}"};
    for (const char *t : bad) EXPECT(!parse(t, 8, d, true).empty());
    // 16 rows on 8 slots
    std::string big = "{\"matrix\": [";
    for (int i = 0; i < 16; ++i) big += std::string(i ? ", " : "") + "[0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0]";
    EXPECT(!parse(big + "]}", 8, d, true).empty());
    EXPECT(parse(big + "]}", 16, d, true).empty() && d.max_abs_sum == 0.0);
}

static void test_headroom() {
    EXPECT(mkh::diagonals_headroom_error(60, 40, 0.0, 50, 1).empty());   // all-zero diagonals need no room
    EXPECT(mkh::diagonals_headroom_error(60, 40, 4.0, 104, 2).empty());  // 102 < 103
    EXPECT(!mkh::diagonals_headroom_error(60, 40, 8.0, 104, 2).empty()); // 103 is not below 103
    EXPECT(!mkh::diagonals_headroom_error(60, 40, 1.0, 100, 2).empty());
}

int main() {
    test_reader();
    for (size_t n : {1, 2, 4, 8}) test_block(n, 8);
    test_block(4, 64);
    test_block_refusals();
    test_headroom();
    if (failures) {
        std::printf("lintrans selftest: %d FAILURE(S)\n", failures);
        return 1;
    }
    std::printf("lintrans selftest ok\n");
    return 0;
}
