// sampler_kernels.hpp -- encryption / key-generation randomness on the GPU.
//
// Stands in for OpenFHE's TernaryUniformGeneratorImpl, DiscreteGaussianGeneratorImpl (sigma = 3.19, CC.json "dp")
// and DiscreteUniformGeneratorImpl ([upstream] core/lib/math/*generator*; SURVEY 2.1 "sample_ternary/gauss/uniform"),
// consumed by KeyGen / ReKeyGen / Encrypt (keyGen.cpp:33, REkeyGen.cpp:52, encryptModelWeights.cpp:83).
// OpenFHE's PRNG stream (blake2-based) cannot be reproduced, so parity is distributional; what consumes the samples
// is bit-exact.  Generator: the ChaCha20 block function (RFC 8439) under a 256-bit key drawn from the OS by the hosts:
// a cryptographic PRF, so published outputs (the uniform polynomial a of a public key) say nothing about the other
// streams.  Counter based: block b of stream `sid`, attempt `att` is ChaCha20(key, counter = b mod 2^32,
// nonce = (b >> 32, sid, att)); element i takes 64-bit word i % 8 of block i / 8 -- a pure function of (key, sid, i),
// independent of launch geometry.
// Decode-time flooding normals (chacha_normal_pair, used by k_flood in codec_kernels.hpp): the pair of work-array
// position i of item t is z0, z1 from 64-bit words 2(k%4) and 2(k%4)+1 of block k/4, k = t*N/2 + i, nonce
// (b >> 32, sid, 0) -- Box-Muller on 53-bit uniforms u1 = ((w0 >> 11) + 1) * 2^-53 in (0, 1] (finite log),
// u2 = (w1 >> 11) * 2^-53: z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = sqrt(-2 ln u1) sin(2 pi u2).
#pragma once
#include "modarith.hpp"

namespace mk {

struct ChaChaKey {
    uint32_t k[8];
};
MK_D uint32_t rotl32(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }
#define MK_CHACHA_QR(a, b, c, d) \
    a += b; d ^= a; d = rotl32(d, 16); c += d; b ^= c; b = rotl32(b, 12); \
    a += b; d ^= a; d = rotl32(d, 8);  c += d; b ^= c; b = rotl32(b, 7);
// the 16 output words of one block
MK_D void chacha20_block(const ChaChaKey &key, uint32_t counter, uint32_t n0, uint32_t n1, uint32_t n2, uint32_t (&out)[16]) {
    uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key.k[0], key.k[1], key.k[2], key.k[3],
                      key.k[4],    key.k[5],    key.k[6],    key.k[7],    counter,  n0,       n1,       n2};
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = s[i];
#pragma unroll 1
    for (int r = 0; r < 10; ++r) {
        MK_CHACHA_QR(x[0], x[4], x[8], x[12])
        MK_CHACHA_QR(x[1], x[5], x[9], x[13])
        MK_CHACHA_QR(x[2], x[6], x[10], x[14])
        MK_CHACHA_QR(x[3], x[7], x[11], x[15])
        MK_CHACHA_QR(x[0], x[5], x[10], x[15])
        MK_CHACHA_QR(x[1], x[6], x[11], x[12])
        MK_CHACHA_QR(x[2], x[7], x[8], x[13])
        MK_CHACHA_QR(x[3], x[4], x[9], x[14])
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) out[i] = x[i] + s[i];
}
#undef MK_CHACHA_QR
// 64-bit word `w` (0..7) of block b of stream sid
MK_D u64 chacha_u64(const ChaChaKey &key, uint32_t sid, uint64_t b, uint32_t att, int w) {
    uint32_t o[16];
    chacha20_block(key, (uint32_t)b, (uint32_t)(b >> 32), sid, att, o);
    u64 r = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (i == w) r = ((u64)o[2 * i + 1] << 32) | o[2 * i];
    return r;
}

// raw block (known-answer test hook: RFC 8439 2.3.2)
__global__ void k_chacha_block(uint32_t *out, ChaChaKey key, uint32_t counter, uint32_t n0, uint32_t n1, uint32_t n2) {
    uint32_t o[16];
    chacha20_block(key, counter, n0, n1, n2, o);
    if (threadIdx.x == 0 && blockIdx.x == 0)
        for (int i = 0; i < 16; ++i) out[i] = o[i];
}

// two independent N(0,1) samples for element k of stream sid (mapping in the header comment)
MK_D double2 chacha_normal_pair(const ChaChaKey &key, uint32_t sid, uint64_t k) {
    uint32_t o[16];
    const uint64_t b = k >> 2;
    chacha20_block(key, (uint32_t)b, (uint32_t)(b >> 32), sid, 0, o);
    u64 w0 = 0, w1 = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j == (int)(k & 3)) {
            w0 = ((u64)o[4 * j + 1] << 32) | o[4 * j];
            w1 = ((u64)o[4 * j + 3] << 32) | o[4 * j + 2];
        }
    const double u1 = (double)((w0 >> 11) + 1) * 0x1p-53, u2 = (double)(w1 >> 11) * 0x1p-53;
    const double r = sqrt(-2.0 * log(u1));
    double s, c;
    sincospi(2.0 * u2, &s, &c);
    return double2{r * c, r * s};
}

// uniform over {-1, 0, 1}: 64-bit multiply-shift (bias < 2^-62)
__global__ void k_sample_ternary(int8_t *out, size_t n, ChaChaKey key, uint32_t sid) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 r = chacha_u64(key, sid, i >> 3, 0, (int)(i & 7));
    out[i] = (int8_t)((int)mulhi64(r, 3) - 1);
}

// discrete Gaussian D_{Z,sigma} by inversion of the cumulative table of |x| (thr[k] = 2^64 * P(|x| <= k)), sign from
// an independent word; tail cut at GAUSS_TABLE-1 >= 12 sigma for sigma <= 3.2.  Element i: words 2(i%4), 2(i%4)+1 of
// block i/4.
constexpr int GAUSS_TABLE = 48;
struct GaussTable {
    u64 thr[GAUSS_TABLE];
    int count;
};
__global__ void k_sample_gauss(int32_t *out, size_t n, ChaChaKey key, uint32_t sid, GaussTable t) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t o[16];
    const uint64_t b = i >> 2;
    chacha20_block(key, (uint32_t)b, (uint32_t)(b >> 32), sid, 0, o);
    u64 r = 0;
    uint32_t sign = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (j == (int)(i & 3)) {
            r = ((u64)o[4 * j + 1] << 32) | o[4 * j];
            sign = o[4 * j + 2] & 1u;
        }
    int k = 0;
    while (k < t.count - 1 && r >= t.thr[k]) ++k;
    out[i] = sign ? -k : k;
}

// wide ("flooding") Gaussian for the re-randomisation before a key switch (mkckks_sample_gauss_wide): element i is
// rint(sigma * z), z = component i % 2 of chacha_normal_pair(key, sid, i / 2) -- a rounded continuous normal, which is a
// stand-in for D_{Z,sigma} only for sigma >= 2^6 (the host checks the range).  |z| <= sqrt(2 * 53 ln 2) < 8.6 (u1 >= 2^-53),
// so |e| < 2^60 at sigma = 2^56.  One lane = one pair, two stores.
__global__ void k_sample_gauss_wide(int64_t *out, size_t n, double sigma, ChaChaKey key, uint32_t sid) {
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (2 * p >= n) return;
    const double2 z = chacha_normal_pair(key, sid, p);
    out[2 * p] = (int64_t)rint(sigma * z.x);
    if (2 * p + 1 < n) out[2 * p + 1] = (int64_t)rint(sigma * z.y);
}

// uniform residues in [0, q) per limb by rejection (accept r < 2^64 - (2^64 mod q)); out [items][slots][N]
__global__ void k_sample_uniform(u64 *out, uint32_t n, uint32_t nl, uint32_t L, const LimbConst *limb, ChaChaKey key,
                                 uint32_t sid) {
    const uint32_t slot = blockIdx.y, idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const LimbConst lc = limb[slot < nl ? slot : L + (slot - nl)];
    const size_t pos = ((size_t)blockIdx.z * gridDim.y + slot) * n + idx;
    const u64 limit = 0 - lc.c64;  // floor(2^64 / q) * q
    u64 r = 0;
    for (uint32_t attempt = 0; attempt < 64; ++attempt) {
        r = chacha_u64(key, sid, pos >> 3, attempt, (int)(pos & 7));
        if (r < limit) break;
    }
    out[pos] = reduce_word(r, lc);
}

// ---- seeded ciphertexts: c1 = a is word i*N + j of stream (key, sid), i.e. k_sample_uniform(n_polys = 1) -------------
// One lane = one ChaCha20 block = 8 consecutive words of one limb (N % 8 == 0: a block never spans two limbs), computed
// once; a rejected word (r >= 2^64 - (2^64 mod q), probability (2^64 mod q) / 2^64: rare) recomputes only its own
// block at attempts 1..63, as k_sample_uniform does.  The 64 B of a lane go out as four 16-B stores: a wave writes
// 4 KiB, whole lines.
constexpr uint32_t SEED_ITEMS = 64;  // items per launch: keys + stream ids by value in the kernel arguments (2.3 KiB)
struct SeedTable {
    ChaChaKey key[SEED_ITEMS];
    uint32_t sid[SEED_ITEMS];
};
MK_D void uniform_block8(const ChaChaKey &key, uint32_t sid, uint64_t b, const LimbConst &lc, u64 (&w)[8]) {
    const u64 limit = 0 - lc.c64;  // floor(2^64 / q) * q
    uint32_t o[16];
    chacha20_block(key, (uint32_t)b, (uint32_t)(b >> 32), sid, 0, o);
    uint32_t rej = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        w[k] = ((u64)o[2 * k + 1] << 32) | o[2 * k];
        rej |= (uint32_t)(w[k] >= limit) << k;
    }
    while (rej) {
        const int k = __ffs(rej) - 1;
        rej &= rej - 1;
        u64 r = 0;
        for (uint32_t attempt = 1; attempt < 64; ++attempt) {
            r = chacha_u64(key, sid, b, attempt, k);
            if (r < limit) break;
        }
#pragma unroll
        for (int m = 0; m < 8; ++m)
            if (m == k) w[m] = r;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = reduce_word(w[k], lc);
}

// c1 of a batch u64[n][2][nl][N] in place (component 0 untouched); item blockIdx.z uses (t.key[z], t.sid[z])
__global__ __launch_bounds__(256) void k_expand_seeded(u64 *ct, uint32_t n, uint32_t nl, const LimbConst *limb, SeedTable t) {
    const uint32_t item = blockIdx.z, slot = blockIdx.y, j8 = blockIdx.x * blockDim.x + threadIdx.x;
    if (j8 >= n / 8) return;
    const LimbConst lc = limb[slot];
    u64 w[8];
    uniform_block8(t.key[item], t.sid[item], (uint64_t)slot * (n / 8) + j8, lc, w);
    u64 *dst = ct + ((size_t)(2 * item + 1) * nl + slot) * n + (size_t)j8 * 8;
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<ulong2 *>(dst + 2 * k) = ulong2{w[2 * k], w[2 * k + 1]};
}

// ---- t-of-n key sharing (mkckks_share_key): share[p] = sk + sum_{k=1}^{t-1} r_k (p+1)^k mod q_i ----------------------
// r_k is the polynomial of stream (key, sid0 + k - 1) in the seeded-ciphertext definition above (uniform_block8), and
// it exists in registers only: r_k together with one share gives sk away, so the coefficient polynomials never reach
// HBM.  One lane = one ChaCha20 block = 8 consecutive coefficients of one limb; blockIdx.z = a group of SHAMIR_GROUP
// parties, each with its own 8 accumulator words (64 words a lane); the blocks are recomputed per group.  Horner from
// k = t - 1 down to 1: acc = (acc + r_k) * x, x = p + 1 <= 64 (the group's tail past n_parties is computed and not
// stored) -- mul_mod's product stays below 2^(k+7), exact for fp64-class and 60-bit limbs alike.  Per party the 64 B of
// a lane go out as four 16-B stores: a wave writes 4 KiB, whole lines.
constexpr uint32_t SHAMIR_GROUP = 8;
__global__ __launch_bounds__(256) void k_shamir_share(const u64 *sk, u64 *shares, uint32_t n, uint32_t nl, uint32_t n_parties,
                                                      uint32_t threshold, const LimbConst *limb, ChaChaKey key, uint32_t sid0) {
    const uint32_t slot = blockIdx.y, j8 = blockIdx.x * blockDim.x + threadIdx.x, p0 = blockIdx.z * SHAMIR_GROUP;
    if (j8 >= n / 8) return;
    const LimbConst lc = limb[slot];
    const uint64_t b = (uint64_t)slot * (n / 8) + j8;
    u64 acc[SHAMIR_GROUP][8];
#pragma unroll
    for (uint32_t g = 0; g < SHAMIR_GROUP; ++g)
#pragma unroll
        for (int w = 0; w < 8; ++w) acc[g][w] = 0;
#pragma unroll 1
    for (uint32_t k = threshold - 1; k >= 1; --k) {
        u64 r[8];
        uniform_block8(key, sid0 + (k - 1), b, lc, r);
#pragma unroll
        for (uint32_t g = 0; g < SHAMIR_GROUP; ++g)
#pragma unroll
            for (int w = 0; w < 8; ++w) acc[g][w] = mul_mod(add_mod(acc[g][w], r[w], lc.q), (u64)(p0 + g + 1), lc);
    }
    const size_t off = (size_t)slot * n + (size_t)j8 * 8;
    ulong2 s[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) s[w] = *reinterpret_cast<const ulong2 *>(sk + off + 2 * w);
#pragma unroll
    for (uint32_t g = 0; g < SHAMIR_GROUP; ++g) {
        if (p0 + g >= n_parties) break;  // wave-uniform
        u64 *dst = shares + (size_t)(p0 + g) * nl * n + off;
#pragma unroll
        for (int w = 0; w < 4; ++w)
            *reinterpret_cast<ulong2 *>(dst + 2 * w) =
                ulong2{add_mod(acc[g][2 * w], s[w].x, lc.q), add_mod(acc[g][2 * w + 1], s[w].y, lc.q)};
    }
}

// secret-key encryption with a seeded a: c0 = pt + ee - a*s mod q_i (the products of k_fma: mul_mod), where item t's a is
// stream (key, sid0 + t); pt, ee, c0 u64[n_items][nl][N], s u64[.][N] (first nl limbs)
__global__ __launch_bounds__(256) void k_encrypt_seeded(const u64 *pt, const u64 *ee, const u64 *s, u64 *c0, uint32_t n,
                                                        uint32_t nl, const LimbConst *limb, ChaChaKey key, uint32_t sid0) {
    const uint32_t item = blockIdx.z, slot = blockIdx.y, j8 = blockIdx.x * blockDim.x + threadIdx.x;
    if (j8 >= n / 8) return;
    const LimbConst lc = limb[slot];
    u64 a[8];
    uniform_block8(key, sid0 + item, (uint64_t)slot * (n / 8) + j8, lc, a);
    const size_t off = ((size_t)item * nl + slot) * n + (size_t)j8 * 8, soff = (size_t)slot * n + (size_t)j8 * 8;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const ulong2 m = *reinterpret_cast<const ulong2 *>(pt + off + 2 * k);
        const ulong2 e = *reinterpret_cast<const ulong2 *>(ee + off + 2 * k);
        const ulong2 sk = *reinterpret_cast<const ulong2 *>(s + soff + 2 * k);
        const u64 p0 = mul_mod(a[2 * k], sk.x, lc), p1 = mul_mod(a[2 * k + 1], sk.y, lc);
        ulong2 r;
        r.x = sub_mod(add_mod(m.x, e.x, lc.q), p0, lc.q);
        r.y = sub_mod(add_mod(m.y, e.y, lc.q), p1, lc.q);
        *reinterpret_cast<ulong2 *>(c0 + off + 2 * k) = r;
    }
}

}  // namespace mk
