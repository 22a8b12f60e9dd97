// poly_kernels.hpp -- the fused outer sum of a Paterson-Stockmeyer evaluation ("polynomial evaluation").
//
// k_poly_tensor<B>: EVALUATION format, pointwise mod q_t on every (ciphertext, limb) row of the first nl_T limbs:
//     Q'_j       = (M_{j,0}, 0) + sum_{0 < i < B} M_{j,i} b_i              two components, registers only
//     (d0,d1,d2) = (Q'_0, 0) + sum_{0 < j < G} Q'_j (x) g_j                (x) the tensor product of k_tensor
// with b_i = x^i (babies), g_j = y^j (giants) and M the integer constants of the call.  This is the definition
//     sum_{j>=1} [Q_j (x) g_j + M_{j,0} (g_j, 0)] + (Q_0, 0) + (M_{0,0}, 0, 0)
// with the constant column and the constant term written as the virtual baby x^0 = (1, 0): (M, 0) (x) (g0, g1) =
// (M g0, M g1, 0).  Every sum is exact mod q_t, so the bits are those of any other order.
// A thread owns two words (16 bytes) of its row.  It loads the B - 1 babies once and keeps them in registers (B is a
// template parameter: the registers are statically indexed), then walks the giants: the loads of giant j + 1 are issued
// before the arithmetic of giant j.  Babies and giants sit at different levels: each is read where it is, through its own
// limb count (component stride nl * N, item stride 2 * nl * N); only the first nl_T limbs are touched.  The constants
// M u64[G][B][nl_T] are limb-uniform: uniform loads.  Each output word is stored once.  No LDS, no scratch.
//
// Arithmetic classes, block-uniform from the limb table as in tensor_kernels.hpp; every class stores canonical residues.
// Inputs are canonical, M < q < 2^60, k = bit length of q.
//   fp64 (q < 1.25 * 2^50, sums exact below 2^53 >= 6.4 q): a constant product is fp_mulmod_any(b, M), |.| <= 0.97 q
//       (b and M in [0, q)).  Q' starts at M_{j,0} <= q and is reduced after every POLY_FP_INNER = 4 products: at most
//       q + 4 * 0.97 q = 4.88 q before the first reduction, 0.51 q + 4 * 0.97 q = 4.39 q after it.  Q' is then brought to
//       |.| <= 0.51 q by one more fp_reduce BEFORE it enters fp_mulmod_any as the signed factor (that needs |y| <= q and
//       then gives |.| <= 0.75 q).  d1 takes two such products per giant, 1.5 q: reduced every POLY_FP_GIANTS = 3 giants
//       the sums stay within 0.51 q + 3 * 1.5 q = 5.01 q, the start value Q'_0 (<= 0.51 q) included.
//   pseudo-Mersenne (q = 2^k - c): Q' is a 128-bit sum of at most 7 whole products and M_{j,0}, below 2^(2k+3), inside
//       pm_reduce128's range 2^(2k+6): one reduction, canonical.  The outer sums multiply that REDUCED value, so a term
//       is below 2^(2k) as in k_tensor and d1 holds at most 2 * 7 products and the residue Q'_0: below 2^(2k+4).  The fold
//       period of k_tensor (16 terms) is never reached with G - 1 <= 7 giants: one pm_reduce128 per output.
//   Shoup/Barrett: Q' is the 128-bit sum of its products and M_{j,0}: B <= 4 gives at most 3 q^2 + q < 2^(k+62), inside
//       barrett_reduce128's window; B = 8 gives at most 7 q^2 + q < 2^123 and goes through reduce_wide.  The outer sum is
//       TensorAcc<TENSOR_INT> unchanged: canonical terms added canonically.
// Bounds: idx < N is checked; rows are (item, limb) with limb < nl_T <= every operand's nl (the host checks it), item <
// gridDim.z; operand j of the giants is read for j < G - 1 <= POLY_MAX_B - 1 only.
#pragma once
#include <hip/hip_runtime.h>

#include "modarith.hpp"
#include "ntt_radix.hpp"
#include "params.hpp"
#include "tensor_kernels.hpp"

namespace mk {

constexpr uint32_t POLY_THREADS = 256;
constexpr uint32_t POLY_FP_INNER = 4, POLY_FP_GIANTS = 3;

struct PolyOpnd {
    const u64 *p;  // u64[items][2][nl][N]; its first nl_T limbs are read
    uint32_t nl, pad_;
};
struct PolyArgs {
    PolyOpnd baby[POLY_MAX_B - 1];   // x^1 .. x^(B-1)
    PolyOpnd giant[POLY_MAX_B - 1];  // y^1 .. y^(G-1)
    const u64 *m;                    // u64[G][B][nl_T]
    u64 *out3;                       // u64[items][3][nl_T][N]
    uint32_t G, n, nl_T;
};

// one word of a thread's pair: Q' of a giant index and the three running sums, per arithmetic class
template <int CLS>
struct PolyWord;

template <>
struct PolyWord<TENSOR_INT> {
    typedef u64 opnd;
    TensorAcc<TENSOR_INT> acc;
    u64 q0, q1;
    static MK_D opnd conv(u64 v) { return v; }
    template <int B>
    MK_D void inner(const opnd (&b)[B - 1][2], const u64 *m, uint32_t ms, const LimbConst &lc, const PmK &) {
        u64 h0 = 0, l0 = m[0], h1 = 0, l1 = 0;
#pragma unroll
        for (int i = 0; i < B - 1; ++i) {
            const u64 mi = m[(size_t)(i + 1) * ms];
            mac128_split(h0, l0, b[i][0], mi);
            mac128_split(h1, l1, b[i][1], mi);
        }
        q0 = B <= 4 ? barrett_reduce128(h0, l0, lc) : reduce_wide(h0, l0, lc);
        q1 = B <= 4 ? barrett_reduce128(h1, l1, lc) : reduce_wide(h1, l1, lc);
    }
    MK_D void start(const LimbConst &, const PmK &) {
        acc.d0 = q0;
        acc.d1 = q1;
    }
    MK_D void giant(u64 g0, u64 g1, const LimbConst &lc, const PmK &P) { acc.mac(q0, q1, g0, g1, lc, P); }
    MK_D void fold(const LimbConst &, const PmK &) {}
    static constexpr uint32_t FOLD_GIANTS = 0;
};

template <>
struct PolyWord<TENSOR_PM> {
    typedef u64 opnd;
    TensorAcc<TENSOR_PM> acc;
    u64 q0, q1;
    static MK_D opnd conv(u64 v) { return v; }
    template <int B>
    MK_D void inner(const opnd (&b)[B - 1][2], const u64 *m, uint32_t ms, const LimbConst &lc, const PmK &P) {
        u64 h0 = 0, l0 = m[0], h1 = 0, l1 = 0;
#pragma unroll
        for (int i = 0; i < B - 1; ++i) {
            const u64 mi = m[(size_t)(i + 1) * ms];
            mac128(h0, l0, b[i][0], mi);
            mac128(h1, l1, b[i][1], mi);
        }
        q0 = pm_reduce128(h0, l0, P, lc.q);
        q1 = pm_reduce128(h1, l1, P, lc.q);
    }
    MK_D void start(const LimbConst &, const PmK &) {
        acc.l0 = q0;
        acc.l1 = q1;
    }
    MK_D void giant(u64 g0, u64 g1, const LimbConst &lc, const PmK &P) { acc.mac(q0, q1, g0, g1, lc, P); }
    MK_D void fold(const LimbConst &, const PmK &) {}
    static constexpr uint32_t FOLD_GIANTS = 0;  // 2 * 7 products and a residue stay inside pm_reduce128's range
};

template <>
struct PolyWord<TENSOR_FP> {
    typedef double opnd;
    TensorAcc<TENSOR_FP> acc;
    double q0, q1;  // |.| <= 0.51 q
    static MK_D opnd conv(u64 v) { return u52_to_double(v); }
    template <int B>
    MK_D void inner(const opnd (&b)[B - 1][2], const u64 *m, uint32_t ms, const LimbConst &lc, const PmK &) {
        double s0 = u52_to_double(m[0]), s1 = 0.0;
#pragma unroll
        for (int i = 0; i < B - 1; ++i) {
            if (i && i % (int)POLY_FP_INNER == 0) {
                s0 = fp_reduce(s0, lc.qd, lc.qinv);
                s1 = fp_reduce(s1, lc.qd, lc.qinv);
            }
            const double mi = u52_to_double(m[(size_t)(i + 1) * ms]);
            s0 += fp_mulmod_any(b[i][0], mi, lc.qd, lc.qinv);
            s1 += fp_mulmod_any(b[i][1], mi, lc.qd, lc.qinv);
        }
        q0 = fp_reduce(s0, lc.qd, lc.qinv);
        q1 = fp_reduce(s1, lc.qd, lc.qinv);
    }
    MK_D void start(const LimbConst &, const PmK &) {
        acc.d0 = q0;
        acc.d1 = q1;
    }
    MK_D void giant(u64 g0, u64 g1, const LimbConst &lc, const PmK &) {
        const double y0 = u52_to_double(g0), y1 = u52_to_double(g1);
        acc.d0 += fp_mulmod_any(q0, y0, lc.qd, lc.qinv);
        acc.d1 += fp_mulmod_any(q0, y1, lc.qd, lc.qinv) + fp_mulmod_any(q1, y0, lc.qd, lc.qinv);
        acc.d2 += fp_mulmod_any(q1, y1, lc.qd, lc.qinv);
    }
    MK_D void fold(const LimbConst &lc, const PmK &P) { acc.fold(lc, P); }
    static constexpr uint32_t FOLD_GIANTS = POLY_FP_GIANTS;
};

template <int CLS, int B>
MK_D void poly_row(const PolyArgs &t, const LimbConst &lc, uint32_t slot, uint32_t item, uint32_t idx) {
    typedef typename PolyWord<CLS>::opnd opnd;
    const PmK P = CLS == TENSOR_PM ? pm_consts(lc) : PmK{};
    const size_t row = (size_t)slot * t.n + idx;
    opnd bx[B - 1][2], by[B - 1][2];  // the babies' two components, word x and word y of the pair
#pragma unroll
    for (int i = 0; i < B - 1; ++i) {
        const size_t comp = (size_t)t.baby[i].nl * t.n;
        const u64 *p = t.baby[i].p + (size_t)item * 2 * comp + row;
        const ulong2 v0 = ld_stream2(reinterpret_cast<const ulong2 *>(p));
        const ulong2 v1 = ld_stream2(reinterpret_cast<const ulong2 *>(p + comp));
        bx[i][0] = PolyWord<CLS>::conv(v0.x);
        bx[i][1] = PolyWord<CLS>::conv(v1.x);
        by[i][0] = PolyWord<CLS>::conv(v0.y);
        by[i][1] = PolyWord<CLS>::conv(v1.y);
    }
    auto load_giant = [&](uint32_t j, ulong2 &g0, ulong2 &g1) {  // y^(j+1)
        const size_t comp = (size_t)t.giant[j].nl * t.n;
        const u64 *p = t.giant[j].p + (size_t)item * 2 * comp + row;
        g0 = ld_stream2(reinterpret_cast<const ulong2 *>(p));
        g1 = ld_stream2(reinterpret_cast<const ulong2 *>(p + comp));
    };
    ulong2 g0, g1;
    load_giant(0, g0, g1);  // G >= 2
    const u64 *m = t.m + slot;  // M_{j,i} of this limb at m[(j * B + i) * nl_T]
    const uint32_t ms = t.nl_T;
    PolyWord<CLS> x, y;
    x.template inner<B>(bx, m, ms, lc, P);
    y.template inner<B>(by, m, ms, lc, P);
    x.start(lc, P);
    y.start(lc, P);
    uint32_t pending = 0;
    for (uint32_t j = 1; j < t.G; ++j) {
        ulong2 n0 = g0, n1 = g1;
        if (j + 1 < t.G) load_giant(j, n0, n1);  // the next giant's words are on their way while this one is multiplied
        const u64 *mj = m + (size_t)j * B * ms;
        x.template inner<B>(bx, mj, ms, lc, P);
        y.template inner<B>(by, mj, ms, lc, P);
        if (PolyWord<CLS>::FOLD_GIANTS && pending == PolyWord<CLS>::FOLD_GIANTS) {
            x.fold(lc, P);
            y.fold(lc, P);
            pending = 0;
        }
        x.giant(g0.x, g1.x, lc, P);
        y.giant(g0.y, g1.y, lc, P);
        ++pending;
        g0 = n0;
        g1 = n1;
    }
    ulong2 r0, r1, r2;
    x.acc.finish(r0.x, r1.x, r2.x, lc, P);
    y.acc.finish(r0.y, r1.y, r2.y, lc, P);
    const size_t comp = (size_t)t.nl_T * t.n;
    u64 *o = t.out3 + (size_t)item * 3 * comp + row;
    *reinterpret_cast<ulong2 *>(o) = r0;
    *reinterpret_cast<ulong2 *>(o + comp) = r1;
    *reinterpret_cast<ulong2 *>(o + 2 * comp) = r2;
}

// grid (N / (2 * POLY_THREADS), nl_T, items); one limb per workgroup, so the class switch is block-uniform
template <int B>
__global__ __launch_bounds__(POLY_THREADS) void k_poly_tensor(PolyArgs t, const LimbConst *limb) {
    const uint32_t slot = blockIdx.y, item = blockIdx.z;
    const uint32_t idx = (blockIdx.x * POLY_THREADS + threadIdx.x) * 2;
    if (idx >= t.n) return;
    const LimbConst lc = limb[slot];  // Q limbs: the limb id is the slot
    if (lc.fp) poly_row<TENSOR_FP, B>(t, lc, slot, item, idx);
    else if (lc.pm) poly_row<TENSOR_PM, B>(t, lc, slot, item, idx);
    else poly_row<TENSOR_INT, B>(t, lc, slot, item, idx);
}

}  // namespace mk
