// galois_kernels.hpp -- the ring automorphism sigma_g on the device (index arithmetic and its proofs: galois.hpp).
//
// k_automorph: EVALUATION format, out[i] = in[galois_src(i)] on every (polynomial, limb) row of a batch in one launch.
// It moves canonical residues and does no arithmetic, so one instance serves every arithmetic class and ring size.
// A workgroup owns one aligned tile of 2^log_t words (8 KiB where N >= 1024) of one row: by the block property its
// words all come from one aligned source tile, which is read whole with coalesced 16-byte loads into LDS, permuted on
// the way out of LDS and written with coalesced 16-byte stores -- every fetched line is used whole.  Words 2c and 2c + 1
// of a row differ in the top bit of brev(i), which moves the source's brev by N / 2: src(2c + 1) = src(2c) ^ 1, so a
// 16-byte pair stays a pair (possibly swapped) and one index serves 16 bytes.
// Bounds: every index is masked to its tile, the source tile base is below N by construction.
#pragma once
#include <hip/hip_runtime.h>

#include "galois.hpp"
#include "modarith.hpp"

namespace mk {

constexpr uint32_t AUTO_THREADS = 256;
constexpr uint32_t AUTO_LOG_TILE = 10;  // words per tile: 2^10 (the whole row on smaller rings)

// grid.x = rows << (log_n - log_t), rows = (polynomial, limb) pairs, N words apart in both in and out
__global__ __launch_bounds__(AUTO_THREADS) void k_automorph(const u64 *in, u64 *out, uint32_t g, uint32_t log_n,
                                                            uint32_t log_t) {
    __shared__ ulonglong2 tile[(1u << AUTO_LOG_TILE) / 2];
    const uint32_t tmask = (1u << log_t) - 1u;
    const uint32_t dbase = (blockIdx.x & ((1u << (log_n - log_t)) - 1u)) << log_t;
    const size_t row = (size_t)(blockIdx.x >> (log_n - log_t)) << log_n;
    const uint32_t sbase = galois_src(dbase, g, log_n) & ~tmask;
    const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(in + row + sbase);
    ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(out + row + dbase);
    // a tile has at most 2 * AUTO_THREADS pairs: a thread's two loads are in flight together
    const uint32_t pairs = 1u << (log_t - 1);
    const uint32_t ca = threadIdx.x, cb = ca + AUTO_THREADS;
    // only the stores are predicated: a pair index past the tile loads the tile's last pair again (in bounds) and parks
    // it in the unused part of the LDS array, so nothing stands between the two loads
    const ulonglong2 va = src[min(ca, pairs - 1u)], vb = src[min(cb, pairs - 1u)];
    tile[ca] = va;
    tile[cb] = vb;
    __syncthreads();
    const uint32_t sa = galois_src(dbase + 2u * ca, g, log_n) & tmask, sb = galois_src(dbase + 2u * cb, g, log_n) & tmask;
    const ulonglong2 ta = tile[sa >> 1], tb = tile[sb >> 1];
    if (ca < pairs) dst[ca] = (sa & 1u) ? make_ulonglong2(ta.y, ta.x) : ta;
    if (cb < pairs) dst[cb] = (sb & 1u) ? make_ulonglong2(tb.y, tb.x) : tb;
}
static_assert((1u << AUTO_LOG_TILE) / 2 == 2 * AUTO_THREADS, "k_automorph: two pairs per thread are the LDS array");

// COEFFICIENT format, ternary secret int8[N]: coefficient k goes to position k g mod 2N, negated when it wraps past N
__global__ void k_automorph_s8(const int8_t *s, int8_t *out, uint32_t g, uint32_t log_n) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (1u << log_n)) return;
    bool neg;
    const uint32_t p = galois_coeff_target(k, g, log_n, &neg);
    const int8_t v = s[k];
    out[p] = neg ? (int8_t)-v : v;
}

}  // namespace mk
