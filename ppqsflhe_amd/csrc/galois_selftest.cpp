// galois_selftest.cpp -- the index arithmetic of galois.hpp on the host, built with AddressSanitizer + UBSan
// (make -C ppqsflhe_amd/csrc asan).  For every ring size the library accepts and a set of Galois elements:
//   - galois_src is a permutation of [0, N) and satisfies its defining congruence;
//   - block property: the words of an aligned block of 2^b words come from ONE aligned source block, and a 16-byte pair
//     stays a pair: src(2c + 1) = src(2c) ^ 1 (what k_automorph is built on);
//   - on a ternary vector sigma_g then sigma_{g^-1} is the identity, and sigma_g keeps the multiset of magnitudes;
//   - 5^r and 5^-r multiply to 1 mod 2N, step 0 gives 1, steps repeat with period N / 2.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "galois.hpp"

using namespace mk;

static int fails = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            if (++fails > 20) std::exit(1);                                \
        }                                                                  \
    } while (0)

static std::vector<int8_t> sigma_s8(const std::vector<int8_t> &s, uint32_t g, uint32_t log_n) {
    std::vector<int8_t> out(s.size(), 0);
    for (uint32_t k = 0; k < s.size(); ++k) {
        bool neg;
        const uint32_t p = galois_coeff_target(k, g, log_n, &neg);
        out[p] = neg ? (int8_t)-s[k] : s[k];
    }
    return out;
}

static void check_element(uint32_t log_n, uint32_t g) {
    const uint32_t n = 1u << log_n, two_n = 2u * n;
    CHECK(galois_valid(g, log_n));
    std::vector<uint32_t> src(n);
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = galois_src(i, g, log_n);
        CHECK(s < n);
        if (s >= n) return;
        src[i] = s;
        CHECK(!seen[s]);
        seen[s] = 1;
        const uint64_t lhs = 2u * galois_brev(s, log_n) + 1u, rhs = (uint64_t)(2u * galois_brev(i, log_n) + 1u) * g;
        CHECK(lhs == rhs % two_n);
    }
    for (uint32_t c = 0; c < n / 2; ++c) CHECK(src[2 * c + 1] == (src[2 * c] ^ 1u));
    for (uint32_t b = 1; b <= log_n; ++b) {
        const uint32_t mask = ~((1u << b) - 1u);
        for (uint32_t i = 0; i < n; ++i) CHECK((src[i] & mask) == (src[i & mask] & mask));
    }
    // sigma_{g^-1} after sigma_g on a ternary vector, and on EVALUATION indices
    const uint32_t gi = galois_inverse(g, log_n);
    CHECK(galois_valid(gi, log_n));
    CHECK(((uint64_t)g * gi) % two_n == 1);
    std::vector<int8_t> s(n);
    uint32_t x = 12345u + g;
    for (uint32_t k = 0; k < n; ++k) {
        x = x * 1664525u + 1013904223u;
        s[k] = (int8_t)((x >> 16) % 3) - 1;
    }
    const std::vector<int8_t> back = sigma_s8(sigma_s8(s, g, log_n), gi, log_n);
    CHECK(back == s);
    for (uint32_t i = 0; i < n; ++i) CHECK(galois_src(galois_src(i, g, log_n), gi, log_n) == i);
}

int main() {
    CHECK(!galois_valid(2, 10) && !galois_valid(2048, 10) && !galois_valid(2049, 10) && galois_valid(2047, 10));
    for (uint32_t log_n = 8; log_n <= 17; ++log_n) {
        const uint32_t n = 1u << log_n, two_n = 2u * n;
        CHECK(galois_element(0, log_n) == 1);
        CHECK(galois_element(1, log_n) == 5);
        CHECK(galois_element((int32_t)(n / 2), log_n) == 1);
        for (int32_t r : {1, 2, 3, 7, 255, 1000, (int32_t)(n / 4 - 1), (int32_t)(n / 4 - 7), (int32_t)(n / 2 - 1)}) {
            const uint32_t g = galois_element(r, log_n), gi = galois_element(-r, log_n);
            CHECK(((uint64_t)g * gi) % two_n == 1);
            CHECK(gi == galois_inverse(g, log_n));
            CHECK(galois_element(r + (int32_t)(n / 2), log_n) == g);
        }
        CHECK(galois_element(INT32_MIN, log_n) == 1 && galois_element(INT32_MAX, log_n) == galois_element(-1, log_n));
        for (uint32_t g : {1u, 5u, galois_element(-1, log_n), galois_element(3, log_n), galois_element((int32_t)(n / 4 - 7), log_n),
                           two_n - 1u, 3u, two_n - 3u})
            check_element(log_n, g);
    }
    if (fails) return 1;
    std::printf("galois selftest ok\n");
    return 0;
}
