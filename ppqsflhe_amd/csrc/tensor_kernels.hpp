// tensor_kernels.hpp -- the tensor product of two-component ciphertexts ("ciphertext products").
//
// k_tensor: EVALUATION format, pointwise mod q_i on every (ciphertext, limb) row of a chunk in one launch:
//     (d0, d1, d2) = sum over terms of (a0 b0, a0 b1 + a1 b0, a1 b1)
// A thread owns two words (16 bytes) of its row.  Per term it loads them from a0, a1, b0, b1 (two polynomials in the
// square instance) with all loads issued before the arithmetic -- the loads of term t + 1 are issued before the arithmetic
// of term t -- keeps the three sums in registers and stores each output once.  No LDS, no scratch.
// It reads and writes the same words of a row only, so d0 / d1 may be written over a or b (mkckks_mult_relin_batch).
//
// Arithmetic classes, block-uniform from the limb table (the flags the engine set under MKCKKS_NO_FP64 / MKCKKS_NO_PM):
// every class stores canonical residues, so the bits do not depend on the class.  Inputs are canonical, q < 2^60.
//   fp64 (q < 1.25 * 2^50): a product is fp_mulmod_any, the exact integer x y - b q with |.| <= 0.97 q.  Sums of such
//       integers are exact below 2^53 >= 6.4 q, and fp_reduce brings a sum with |.| < 2^53 back to |.| <= 0.51 q.  d1
//       takes two products per term: reduced every TENSOR_FP_TERMS = 2 terms the sums stay within
//       0.51 q + 4 * 0.97 q = 4.39 q.  One reduction serves both products of d1.
//   pseudo-Mersenne (q = 2^k - c): 128-bit sums of whole products (mac128: x < 2^63, y < 2^60), one pm_reduce128 per
//       output.  Its range is X < 2^(2k+6), i.e. 64 products of canonical residues (each below 2^(2k)): d1 holds
//       2 * TENSOR_PM_TERMS = 32 products plus one carried residue when it is folded.
//   Shoup/Barrett (any other integer limb): d1 of a term is the 128-bit sum of its two products, below 2 q^2 < 2^(k+61),
//       inside barrett_reduce128's window 2^(k+62) (k = bit length of q): one reduction.  Terms are added canonically.
// The square instance forms 2 a0 a1 as (2 a0) a1 on the integer classes (2 a0 < 2^61: inside every range above) and as
// 2 fp_mulmod_any(a0, a1) on fp64 (|.| <= 1.94 q, the same bound as two products).
// Bounds: idx < N is checked; rows are (item, limb) with limb < nl, item < gridDim.z; the host passes the strides.
#pragma once
#include <hip/hip_runtime.h>

#include "modarith.hpp"
#include "ntt_radix.hpp"

namespace mk {

constexpr uint32_t TENSOR_THREADS = 256;
constexpr uint32_t TENSOR_FP_TERMS = 2, TENSOR_PM_TERMS = 16;

struct TensorArgs {
    const u64 *a, *b;    // u64[n_terms][items][2][nl][N]; b == a selects nothing here: the host launches k_tensor<true>
    u64 *o01, *o2;       // (d0, d1) of item t at o01 + t * o01_stride, d1 nl * N words after d0; d2 at o2 + t * o2_stride
    size_t term_stride;  // words between the terms of a and b
    size_t o01_stride, o2_stride;
    uint32_t n_terms, n, nl;
};

enum { TENSOR_INT = 0, TENSOR_PM = 1, TENSOR_FP = 2 };

// the three running sums of one word, per arithmetic class
template <int CLS>
struct TensorAcc;

template <>
struct TensorAcc<TENSOR_INT> {
    u64 d0 = 0, d1 = 0, d2 = 0;  // canonical
    MK_D void term(u64 p0, u64 h1, u64 l1, u64 p2, const LimbConst &lc) {
        d0 = add_mod(d0, p0, lc.q);
        d1 = add_mod(d1, barrett_reduce128(h1, l1, lc), lc.q);
        d2 = add_mod(d2, p2, lc.q);
    }
    MK_D void mac(u64 a0, u64 a1, u64 b0, u64 b1, const LimbConst &lc, const PmK &) {
        u64 h = 0, l = 0;
        mac128_split(h, l, a0, b1);
        mac128_split(h, l, a1, b0);
        term(mul_mod(a0, b0, lc), h, l, mul_mod(a1, b1, lc), lc);
    }
    MK_D void mac_sq(u64 a0, u64 a1, const LimbConst &lc, const PmK &) {
        u64 h, l;
        mul128(2 * a0, a1, h, l);
        term(mul_mod(a0, a0, lc), h, l, mul_mod(a1, a1, lc), lc);
    }
    MK_D void fold(const LimbConst &, const PmK &) {}
    MK_D void finish(u64 &r0, u64 &r1, u64 &r2, const LimbConst &, const PmK &) {
        r0 = d0;
        r1 = d1;
        r2 = d2;
    }
    static constexpr uint32_t FOLD_TERMS = 0;
};

template <>
struct TensorAcc<TENSOR_PM> {
    u64 h0 = 0, l0 = 0, h1 = 0, l1 = 0, h2 = 0, l2 = 0;
    MK_D void mac(u64 a0, u64 a1, u64 b0, u64 b1, const LimbConst &, const PmK &) {
        mac128(h0, l0, a0, b0);
        mac128(h1, l1, a0, b1);
        mac128(h1, l1, a1, b0);
        mac128(h2, l2, a1, b1);
    }
    MK_D void mac_sq(u64 a0, u64 a1, const LimbConst &, const PmK &) {
        mac128(h0, l0, a0, a0);
        mac128(h1, l1, 2 * a0, a1);
        mac128(h2, l2, a1, a1);
    }
    MK_D void fold(const LimbConst &lc, const PmK &P) {
        l0 = pm_reduce128(h0, l0, P, lc.q);
        l1 = pm_reduce128(h1, l1, P, lc.q);
        l2 = pm_reduce128(h2, l2, P, lc.q);
        h0 = h1 = h2 = 0;
    }
    MK_D void finish(u64 &r0, u64 &r1, u64 &r2, const LimbConst &lc, const PmK &P) {
        r0 = pm_reduce128(h0, l0, P, lc.q);
        r1 = pm_reduce128(h1, l1, P, lc.q);
        r2 = pm_reduce128(h2, l2, P, lc.q);
    }
    static constexpr uint32_t FOLD_TERMS = TENSOR_PM_TERMS;
};

template <>
struct TensorAcc<TENSOR_FP> {
    double d0 = 0.0, d1 = 0.0, d2 = 0.0;
    MK_D void mac(u64 a0, u64 a1, u64 b0, u64 b1, const LimbConst &lc, const PmK &) {
        const double x0 = u52_to_double(a0), x1 = u52_to_double(a1), y0 = u52_to_double(b0), y1 = u52_to_double(b1);
        d0 += fp_mulmod_any(x0, y0, lc.qd, lc.qinv);
        d1 += fp_mulmod_any(x0, y1, lc.qd, lc.qinv) + fp_mulmod_any(x1, y0, lc.qd, lc.qinv);
        d2 += fp_mulmod_any(x1, y1, lc.qd, lc.qinv);
    }
    MK_D void mac_sq(u64 a0, u64 a1, const LimbConst &lc, const PmK &) {
        const double x0 = u52_to_double(a0), x1 = u52_to_double(a1);
        d0 += fp_mulmod_any(x0, x0, lc.qd, lc.qinv);
        d1 += 2.0 * fp_mulmod_any(x0, x1, lc.qd, lc.qinv);
        d2 += fp_mulmod_any(x1, x1, lc.qd, lc.qinv);
    }
    MK_D void fold(const LimbConst &lc, const PmK &) {
        d0 = fp_reduce(d0, lc.qd, lc.qinv);
        d1 = fp_reduce(d1, lc.qd, lc.qinv);
        d2 = fp_reduce(d2, lc.qd, lc.qinv);
    }
    MK_D void finish(u64 &r0, u64 &r1, u64 &r2, const LimbConst &lc, const PmK &) {
        r0 = fp_to_canonical(d0, lc.qd, lc.qinv);
        r1 = fp_to_canonical(d1, lc.qd, lc.qinv);
        r2 = fp_to_canonical(d2, lc.qd, lc.qinv);
    }
    static constexpr uint32_t FOLD_TERMS = TENSOR_FP_TERMS;
};

template <int CLS, bool SQUARE>
MK_D void tensor_row(const TensorArgs &t, const LimbConst &lc, size_t in_off, size_t o01_off, size_t o2_off) {
    const size_t comp = (size_t)t.nl * t.n;
    const PmK P = CLS == TENSOR_PM ? pm_consts(lc) : PmK{};
    TensorAcc<CLS> x, y;
    const ulong2 *pa = reinterpret_cast<const ulong2 *>(t.a + in_off);
    const ulong2 *pb = reinterpret_cast<const ulong2 *>(t.b + in_off);
    const size_t comp2 = comp / 2, term2 = t.term_stride / 2;  // in 16-byte units
    ulong2 a0 = ld_stream2(pa), a1 = ld_stream2(pa + comp2), b0 = a0, b1 = a1;
    if (!SQUARE) {
        b0 = ld_stream2(pb);
        b1 = ld_stream2(pb + comp2);
    }
    uint32_t pending = 0;
    for (uint32_t k = 0; k < t.n_terms; ++k) {
        ulong2 na0 = a0, na1 = a1, nb0 = b0, nb1 = b1;
        if (k + 1 < t.n_terms) {  // the next term's words are on their way while this term is multiplied
            pa += term2;
            pb += term2;
            na0 = ld_stream2(pa);
            na1 = ld_stream2(pa + comp2);
            if (!SQUARE) {
                nb0 = ld_stream2(pb);
                nb1 = ld_stream2(pb + comp2);
            }
        }
        if (TensorAcc<CLS>::FOLD_TERMS && pending == TensorAcc<CLS>::FOLD_TERMS) {
            x.fold(lc, P);
            y.fold(lc, P);
            pending = 0;
        }
        if (SQUARE) {
            x.mac_sq(a0.x, a1.x, lc, P);
            y.mac_sq(a0.y, a1.y, lc, P);
        } else {
            x.mac(a0.x, a1.x, b0.x, b1.x, lc, P);
            y.mac(a0.y, a1.y, b0.y, b1.y, lc, P);
        }
        ++pending;
        a0 = na0;
        a1 = na1;
        b0 = nb0;
        b1 = nb1;
    }
    ulong2 r0, r1, r2;
    x.finish(r0.x, r1.x, r2.x, lc, P);
    y.finish(r0.y, r1.y, r2.y, lc, P);
    *reinterpret_cast<ulong2 *>(t.o01 + o01_off) = r0;
    *reinterpret_cast<ulong2 *>(t.o01 + o01_off + comp) = r1;
    *reinterpret_cast<ulong2 *>(t.o2 + o2_off) = r2;
}

// grid (N / (2 * TENSOR_THREADS), nl, items); one limb per workgroup, so the class switch is block-uniform
template <bool SQUARE>
__global__ __launch_bounds__(TENSOR_THREADS) void k_tensor(TensorArgs t, const LimbConst *limb) {
    const uint32_t slot = blockIdx.y, item = blockIdx.z;
    const uint32_t idx = (blockIdx.x * TENSOR_THREADS + threadIdx.x) * 2;
    if (idx >= t.n) return;
    const LimbConst lc = limb[slot];  // Q limbs: the limb id is the slot
    const size_t row = (size_t)slot * t.n + idx;
    const size_t in_off = (size_t)item * 2 * t.nl * t.n + row;
    const size_t o01_off = (size_t)item * t.o01_stride + row, o2_off = (size_t)item * t.o2_stride + row;
    if (lc.fp) tensor_row<TENSOR_FP, SQUARE>(t, lc, in_off, o01_off, o2_off);
    else if (lc.pm) tensor_row<TENSOR_PM, SQUARE>(t, lc, in_off, o01_off, o2_off);
    else tensor_row<TENSOR_INT, SQUARE>(t, lc, in_off, o01_off, o2_off);
}

}  // namespace mk
