// cheb_kernels.hpp -- one step of the Chebyshev ladder before its relinearisation, and the affine map in front of it
// ("Chebyshev series"; include/mkckks.h: "Chebyshev series").
//
// k_cheb_tensor<SQUARE, TERM>: EVALUATION format, pointwise mod q_l on every (ciphertext, limb) row of the first nl limbs:
//     d0 = 2 a0 b0 - M t0          TERM: t = (t0, t1) a ciphertext (T_1);  !TERM: t0 = 1, t1 = 0 (the constant T_0)
//     d1 = 2 (a0 b1 + a1 b0) - M t1
//     d2 = 2 a1 b1
// the tensor product of T_i = a and T_j = b, doubled, minus M T_{i-j}: T_{i+j} = 2 T_i T_j - T_{i-j} with the scales made equal
// in the integer M = rint(S_a S_b / S_t).  The table m u64[nl] holds M' = (q_l - (M mod q_l)) mod q_l, so every term is added:
// d0 = 2 a0 b0 + M' t0.  It is limb-uniform: a uniform load.
// A thread owns two words (16 bytes) of its row.  It loads them from a0, a1, b0, b1 (two polynomials in the square
// instance) and t0, t1 (TERM) with all loads issued before the arithmetic, and stores each output once.  a, b and t are
// read where they are, through their own limb counts (component stride nl_x * N, item stride 2 * nl_x * N); only the first
// nl limbs are touched.  No LDS, no scratch.  It reads and writes the same words of a row only.
//
// Arithmetic classes, block-uniform from the limb table as in tensor_kernels.hpp; every class stores canonical residues.
// Inputs are canonical, M' < q < 2^60, k = bit length of q (2^(k-1) <= q < 2^k, k <= 60).
//   fp64 (q < 1.25 * 2^50, sums exact below 2^53 >= 6.4 q): a product is fp_mulmod_any, |.| <= 0.97 q, for a first factor
//       with |.| <= q and a second in [0, q): residues and M' are both.  Doubling an exact integer is exact.
//       d0 = 2 p + p': 2 * 0.97 q + 0.97 q = 2.91 q (!TERM: 1.94 q + M' <= 2.94 q);  d1 = 2 (p + p) + p': 4 * 0.97 q + 0.97 q =
//       4.85 q;  d2 = 1.94 q.  All inside fp_reduce's 2^53: one reduction (in fp_to_canonical) per output.
//   pseudo-Mersenne (q = 2^k - c): 128-bit sums of whole products, mac128(x < 2^63, y < 2^60).  The doubling rides on a
//       factor: 2 a0 < 2^61, and 4 a0 < 2^62 in the square instance (d1 = (4 a0) a1).  d1 is at most 4 q^2 + q^2 < 2^(2k+3),
//       inside pm_reduce128's range 2^(2k+6): one reduction per output.
//   Shoup/Barrett (any other integer limb): barrett_reduce128 takes X < 2^(k+62).  d0 = (2 a0) b0 + M' t0 < 3 q^2 < 2^(2k+2) <=
//       2^(k+62) for k <= 60 (!TERM: 2 q^2 + q): one reduction.  d2 = (2 a1) b1 < 2^(2k+1): one reduction.  d1 with a term would
//       be 5 q^2 < 2^(2k+3), which fits only for k <= 59, and a 60-bit limb is allowed: d1 is REDUCED TWICE.  First
//       p = a0 b1 + a1 b0 < 2 q^2 (the window of k_tensor's d1) to a residue, then 2 p + M' t1 < 2 q + q^2 < 2^(2k+1).  Without a
//       term the second step is add_mod(p, p).
//
// k_affine: out = Ma * in + (Mc, 0) on u64[items][2][nl][N], constants u64[2][nl] (Ma then Mc, canonical), mul_mod and
// add_mod of canonical residues in every class; a thread reads its words before it writes them: out may be in.
// Bounds: idx < N is checked; rows are (item, limb) with limb < nl <= every operand's nl (the host checks it), item <
// gridDim.z; the host passes the strides.
#pragma once
#include <hip/hip_runtime.h>

#include "modarith.hpp"
#include "ntt_radix.hpp"
#include "tensor_kernels.hpp"

namespace mk {

constexpr uint32_t CHEB_THREADS = 256;

struct ChebArgs {
    const u64 *a, *b, *t;  // u64[items][2][nl_x][N]; t is not read in the constant instances
    const u64 *m;          // u64[nl]: (q - M mod q) mod q
    u64 *o01, *o2;         // (d0, d1) of item i at o01 + i * o01_stride, d1 nl * N words after d0; d2 at o2 + i * o2_stride
    size_t o01_stride, o2_stride;
    uint32_t nl_a, nl_b, nl_t, n, nl;
};

// one word: (a0, a1) (x) (b0, b1), doubled, plus m (t0, t1); per arithmetic class
template <int CLS, bool SQUARE, bool TERM>
struct ChebWord;

template <bool SQUARE, bool TERM>
struct ChebWord<TENSOR_INT, SQUARE, TERM> {
    static MK_D void run(u64 a0, u64 a1, u64 b0, u64 b1, u64 t0, u64 t1, u64 m, const LimbConst &lc, const PmK &, u64 &r0,
                         u64 &r1, u64 &r2) {
        u64 h, l;
        mul128(2 * a0, b0, h, l);
        if (TERM) {
            mac128_split(h, l, t0, m);
        } else {
            l += m;
            h += l < m ? 1 : 0;
        }
        r0 = barrett_reduce128(h, l, lc);
        if (SQUARE) {
            mul128(2 * a0, a1, h, l);
        } else {
            mul128(a0, b1, h, l);
            mac128_split(h, l, a1, b0);
        }
        const u64 p = barrett_reduce128(h, l, lc);  // the first of d1's two reductions
        if (TERM) {
            mul128(t1, m, h, l);
            const u64 s = l + 2 * p;
            h += s < l ? 1 : 0;
            r1 = barrett_reduce128(h, s, lc);
        } else {
            r1 = add_mod(p, p, lc.q);
        }
        mul128(2 * a1, b1, h, l);
        r2 = barrett_reduce128(h, l, lc);
    }
};

template <bool SQUARE, bool TERM>
struct ChebWord<TENSOR_PM, SQUARE, TERM> {
    static MK_D void run(u64 a0, u64 a1, u64 b0, u64 b1, u64 t0, u64 t1, u64 m, const LimbConst &lc, const PmK &P, u64 &r0,
                         u64 &r1, u64 &r2) {
        u64 h0 = 0, l0 = TERM ? 0 : m, h1 = 0, l1 = 0, h2 = 0, l2 = 0;
        mac128(h0, l0, 2 * a0, b0);
        if (SQUARE) {
            mac128(h1, l1, 4 * a0, a1);
        } else {
            mac128(h1, l1, 2 * a0, b1);
            mac128(h1, l1, 2 * a1, b0);
        }
        mac128(h2, l2, 2 * a1, b1);
        if (TERM) {
            mac128(h0, l0, t0, m);
            mac128(h1, l1, t1, m);
        }
        r0 = pm_reduce128(h0, l0, P, lc.q);
        r1 = pm_reduce128(h1, l1, P, lc.q);
        r2 = pm_reduce128(h2, l2, P, lc.q);
    }
};

template <bool SQUARE, bool TERM>
struct ChebWord<TENSOR_FP, SQUARE, TERM> {
    static MK_D void run(u64 a0, u64 a1, u64 b0, u64 b1, u64 t0, u64 t1, u64 m, const LimbConst &lc, const PmK &, u64 &r0,
                         u64 &r1, u64 &r2) {
        const double q = lc.qd, qi = lc.qinv, md = u52_to_double(m);
        const double x0 = u52_to_double(a0), x1 = u52_to_double(a1);
        const double y0 = SQUARE ? x0 : u52_to_double(b0), y1 = SQUARE ? x1 : u52_to_double(b1);
        double d0 = 2.0 * fp_mulmod_any(x0, y0, q, qi);
        double d1 = SQUARE ? 4.0 * fp_mulmod_any(x0, x1, q, qi)
                           : 2.0 * (fp_mulmod_any(x0, y1, q, qi) + fp_mulmod_any(x1, y0, q, qi));
        const double d2 = 2.0 * fp_mulmod_any(x1, y1, q, qi);
        if (TERM) {
            d0 += fp_mulmod_any(u52_to_double(t0), md, q, qi);
            d1 += fp_mulmod_any(u52_to_double(t1), md, q, qi);
        } else {
            d0 += md;
        }
        r0 = fp_to_canonical(d0, q, qi);
        r1 = fp_to_canonical(d1, q, qi);
        r2 = fp_to_canonical(d2, q, qi);
    }
};

template <int CLS, bool SQUARE, bool TERM>
MK_D void cheb_row(const ChebArgs &c, const LimbConst &lc, uint32_t slot, uint32_t item, uint32_t idx) {
    const PmK P = CLS == TENSOR_PM ? pm_consts(lc) : PmK{};
    const size_t row = (size_t)slot * c.n + idx;
    const size_t ca = (size_t)c.nl_a * c.n, cb = (size_t)c.nl_b * c.n, ct = (size_t)c.nl_t * c.n;
    const u64 *pa = c.a + (size_t)item * 2 * ca + row;
    const ulong2 a0 = ld_stream2(reinterpret_cast<const ulong2 *>(pa));
    const ulong2 a1 = ld_stream2(reinterpret_cast<const ulong2 *>(pa + ca));
    ulong2 b0 = a0, b1 = a1, t0{0, 0}, t1{0, 0};
    if (!SQUARE) {
        const u64 *pb = c.b + (size_t)item * 2 * cb + row;
        b0 = ld_stream2(reinterpret_cast<const ulong2 *>(pb));
        b1 = ld_stream2(reinterpret_cast<const ulong2 *>(pb + cb));
    }
    if (TERM) {
        const u64 *pt = c.t + (size_t)item * 2 * ct + row;
        t0 = ld_stream2(reinterpret_cast<const ulong2 *>(pt));
        t1 = ld_stream2(reinterpret_cast<const ulong2 *>(pt + ct));
    }
    const u64 m = c.m[slot];
    ulong2 r0, r1, r2;
    ChebWord<CLS, SQUARE, TERM>::run(a0.x, a1.x, b0.x, b1.x, t0.x, t1.x, m, lc, P, r0.x, r1.x, r2.x);
    ChebWord<CLS, SQUARE, TERM>::run(a0.y, a1.y, b0.y, b1.y, t0.y, t1.y, m, lc, P, r0.y, r1.y, r2.y);
    u64 *o01 = c.o01 + (size_t)item * c.o01_stride + row;
    *reinterpret_cast<ulong2 *>(o01) = r0;
    *reinterpret_cast<ulong2 *>(o01 + (size_t)c.nl * c.n) = r1;
    *reinterpret_cast<ulong2 *>(c.o2 + (size_t)item * c.o2_stride + row) = r2;
}

// grid (N / (2 * CHEB_THREADS), nl, items); one limb per workgroup, so the class switch is block-uniform
template <bool SQUARE, bool TERM>
__global__ __launch_bounds__(CHEB_THREADS) void k_cheb_tensor(ChebArgs c, const LimbConst *limb) {
    const uint32_t slot = blockIdx.y, item = blockIdx.z;
    const uint32_t idx = (blockIdx.x * CHEB_THREADS + threadIdx.x) * 2;
    if (idx >= c.n) return;
    const LimbConst lc = limb[slot];  // Q limbs: the limb id is the slot
    if (lc.fp) cheb_row<TENSOR_FP, SQUARE, TERM>(c, lc, slot, item, idx);
    else if (lc.pm) cheb_row<TENSOR_PM, SQUARE, TERM>(c, lc, slot, item, idx);
    else cheb_row<TENSOR_INT, SQUARE, TERM>(c, lc, slot, item, idx);
}

// grid (N / (2 * CHEB_THREADS), 2 * nl, items): slot < nl is component 0, which takes the additive constant
__global__ __launch_bounds__(CHEB_THREADS) void k_affine(const u64 *in, u64 *out, const u64 *f, uint32_t n, uint32_t nl,
                                                         const LimbConst *limb) {
    const uint32_t slot = blockIdx.y, item = blockIdx.z;
    const uint32_t idx = (blockIdx.x * CHEB_THREADS + threadIdx.x) * 2;
    if (idx >= n) return;
    const uint32_t l = slot < nl ? slot : slot - nl;
    const LimbConst lc = limb[l];
    const u64 ma = f[l], mc = slot < nl ? f[nl + l] : 0;
    const size_t off = ((size_t)item * 2 * nl + slot) * n + idx;
    ulong2 v = ld_stream2(reinterpret_cast<const ulong2 *>(in + off));
    v.x = add_mod(mul_mod(v.x, ma, lc), mc, lc.q);
    v.y = add_mod(mul_mod(v.y, ma, lc), mc, lc.q);
    *reinterpret_cast<ulong2 *>(out + off) = v;
}

}  // namespace mk
