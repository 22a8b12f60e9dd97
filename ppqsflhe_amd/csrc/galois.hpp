// galois.hpp -- index arithmetic of the ring automorphisms sigma_g(a)(X) = a(X^g), g odd < 2N, shared by the device
// kernels (galois_kernels.hpp), the engine and the hosts.  Plain integer functions, no tables; galois_selftest.cpp
// checks them on the host.
//
// EVALUATION format stores X[i] = a(psi^(2 brev(i) + 1)), so sigma_g is a gather that is the same for
// every limb: sigma_g(X)[i] = X[src(i)] with 2 brev(src(i)) + 1 = (2 brev(i) + 1) g mod 2N.
// Block property: with k = brev(i) the source's k is (g (2k + 1) - 1) / 2 mod N, whose low m bits depend on the low m
// bits of k only; the low bits of k are the high bits of i.  So the words of one aligned block of 2^b words all come
// from ONE aligned source block of 2^b words (galois_src of any of them, high bits), permuted inside it.
// CKKS slot j sits at zeta^(5^j) (codec_kernels.hpp): g = 5^r mod 2N rotates the slots left by r, g = 2N - 1 conjugates.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MK_GALOIS_HD __host__ __device__
#else
#define MK_GALOIS_HD
#endif

namespace mk {

MK_GALOIS_HD inline uint32_t galois_brev(uint32_t x, uint32_t log_n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __brev(x) >> (32 - log_n);
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0F0F0F0Fu) | ((x & 0x0F0F0F0Fu) << 4);
    x = ((x >> 8) & 0x00FF00FFu) | ((x & 0x00FF00FFu) << 8);
    x = (x >> 16) | (x << 16);
    return x >> (32 - log_n);
#endif
}

// a Galois element of the ring of dimension 2^log_n: odd and below 2N
MK_GALOIS_HD inline bool galois_valid(uint32_t g, uint32_t log_n) { return (g & 1u) && g < (2u << log_n); }

// source index of word i < N of sigma_g in EVALUATION format.  g (2k + 1) < 2^36 wraps in 32 bits; only its low
// log_n + 1 <= 18 bits are used
MK_GALOIS_HD inline uint32_t galois_src(uint32_t i, uint32_t g, uint32_t log_n) {
    const uint32_t k = galois_brev(i, log_n);
    const uint32_t ks = ((g * (2u * k + 1u)) >> 1) & ((1u << log_n) - 1u);
    return galois_brev(ks, log_n);
}

// COEFFICIENT format: coefficient k of a goes to position k g mod 2N of sigma_g(a); a position at or above N means
// position - N with the sign flipped (X^N = -1).  Returns the position below N, *negate says whether the sign flips
MK_GALOIS_HD inline uint32_t galois_coeff_target(uint32_t k, uint32_t g, uint32_t log_n, bool *negate) {
    const uint32_t n = 1u << log_n;
    const uint32_t t = (k * g) & (2u * n - 1u);
    *negate = t >= n;
    return t & (n - 1u);
}

// 5^step mod 2N; 5 has order N / 2 in (Z / 2N)*, so a negative step is the inverse element and step 0 gives 1
inline uint32_t galois_element(int32_t step, uint32_t log_n) {
    const uint32_t mask = (2u << log_n) - 1u;
    const int64_t order = (int64_t)1 << (log_n - 1);
    uint64_t e = (uint64_t)(((int64_t)step % order + order) % order);
    uint32_t r = 1u, b = 5u;
    for (; e; e >>= 1, b = (b * b) & mask)
        if (e & 1u) r = (r * b) & mask;
    return r;
}

// g^-1 mod 2N for odd g (Newton's iteration doubles the correct low bits: 3 -> 6 -> 12 -> 24)
inline uint32_t galois_inverse(uint32_t g, uint32_t log_n) {
    uint32_t x = g;  // g g = 1 mod 8
    for (int it = 0; it < 3; ++it) x *= 2u - g * x;
    return x & ((2u << log_n) - 1u);
}

}  // namespace mk
