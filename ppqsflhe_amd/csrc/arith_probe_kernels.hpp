// arith_probe_kernels.hpp -- diagnostics: run ONE primitive of modarith.hpp / ntt_kernels.hpp / ntt_radix.hpp per element.
//
// The primitives exist in a host form and a device form (inline assembly, carries in scalar pairs); whole-kernel tests
// feed them canonical residues only and cannot steer a lazy word to the top of its documented range.  The probe takes
// arbitrary operand planes, so a test can (Engine::debug_arith, mkckks_debug_arith; tests/test_device_arith.py).
// Nothing on the hot path calls this.  Plain C++ and vector stores only: no atomics, no LDS.
//
// Planes as the kernels see them ("expanded", built by Engine::debug_arith): the op's data planes, then for each of
// its n_tw twiddles the table entry w' (Shoup: w; pseudo-Mersenne: w << t; fp64: (double) w), then the n_tw companions
// (Shoup: floor(w 2^64 / q); pseudo-Mersenne: (w 2^32 mod q) << t; fp64: w / q).  The caller passes w only.
#pragma once
#include "ntt_radix.hpp"

namespace mk {

enum ProbeTw : uint32_t { PTW_NONE = 0, PTW_SHOUP = 1, PTW_PM = 2, PTW_FP = 3 };
enum ProbeClass : uint32_t { PCL_INT = 0, PCL_PM = 1, PCL_FP = 2 };

// X(name, id, user input planes (twiddles last), output planes, twiddles, companion kind, class, has a host form)
// The ids are the MKCKKS_OP_* values of include/mkckks.h (engine.hip asserts the two lists agree).
#define MK_PROBE_OPS(X)                                          \
    X(CSUB, 0, 2, 1, 0, PTW_NONE, PCL_INT, 1)                    \
    X(ADD_MOD, 1, 2, 1, 0, PTW_NONE, PCL_INT, 1)                 \
    X(SUB_MOD, 2, 2, 1, 0, PTW_NONE, PCL_INT, 1)                 \
    X(SHOUP_LAZY, 3, 2, 1, 1, PTW_SHOUP, PCL_INT, 1)             \
    X(SHOUP_MUL, 4, 2, 1, 1, PTW_SHOUP, PCL_INT, 1)              \
    X(MUL_MOD, 5, 2, 1, 0, PTW_NONE, PCL_INT, 1)                 \
    X(BARRETT_REDUCE128, 6, 2, 1, 0, PTW_NONE, PCL_INT, 1)       \
    X(REDUCE_WIDE, 7, 2, 1, 0, PTW_NONE, PCL_INT, 1)             \
    X(REDUCE_WORD, 8, 1, 1, 0, PTW_NONE, PCL_INT, 1)             \
    X(REDUCE_COLS_LAZY, 9, 3, 1, 0, PTW_NONE, PCL_INT, 1)        \
    X(REDUCE_COLS, 10, 3, 1, 0, PTW_NONE, PCL_INT, 1)            \
    X(REDUCE_COLS4, 11, 4, 1, 0, PTW_NONE, PCL_INT, 1)           \
    X(MAC128, 12, 4, 2, 0, PTW_NONE, PCL_INT, 1)                 \
    X(MAC128_SPLIT, 13, 4, 2, 0, PTW_NONE, PCL_INT, 1)           \
    X(CT_BUTTERFLY_C4, 14, 3, 2, 1, PTW_SHOUP, PCL_INT, 1)       \
    X(CT_BUTTERFLY_NC, 15, 3, 2, 1, PTW_SHOUP, PCL_INT, 1)       \
    X(GS_BUTTERFLY, 16, 3, 2, 1, PTW_SHOUP, PCL_INT, 1)          \
    X(CANON8, 17, 1, 1, 0, PTW_NONE, PCL_INT, 1)                 \
    X(RADIX_FORWARD4, 18, 31, 16, 15, PTW_SHOUP, PCL_INT, 1)     \
    X(RADIX_INVERSE4, 19, 31, 16, 15, PTW_SHOUP, PCL_INT, 1)     \
    X(PM_FOLD, 20, 1, 1, 0, PTW_NONE, PCL_PM, 1)                 \
    X(PM_LAZY, 21, 2, 1, 1, PTW_PM, PCL_PM, 1)                   \
    X(PM_REDUCE128, 22, 2, 1, 0, PTW_NONE, PCL_PM, 1)            \
    X(PM_REDUCE_COLS, 23, 3, 1, 0, PTW_NONE, PCL_PM, 1)          \
    X(CT_BUTTERFLY_PM_F, 24, 3, 2, 1, PTW_PM, PCL_PM, 1)         \
    X(CT_BUTTERFLY_PM_N, 25, 3, 2, 1, PTW_PM, PCL_PM, 1)         \
    X(GS_BUTTERFLY_PM, 26, 3, 2, 1, PTW_PM, PCL_PM, 1)           \
    X(RADIX_FORWARD_PM4, 27, 31, 16, 15, PTW_PM, PCL_PM, 1)      \
    X(RADIX_INVERSE_PM4, 28, 31, 16, 15, PTW_PM, PCL_PM, 1)      \
    X(FP_MULMOD, 29, 2, 1, 1, PTW_FP, PCL_FP, 0)                 \
    X(FP_REDUCE, 30, 1, 1, 0, PTW_NONE, PCL_FP, 0)               \
    X(FP_TO_CANONICAL, 31, 1, 1, 0, PTW_NONE, PCL_FP, 0)         \
    X(FP_MULMOD_ANY, 32, 2, 1, 0, PTW_NONE, PCL_FP, 0)           \
    X(U52_TO_DOUBLE, 33, 1, 1, 0, PTW_NONE, PCL_FP, 0)           \
    X(SPLIT30_D, 34, 1, 2, 0, PTW_NONE, PCL_FP, 0)               \
    X(CT_BUTTERFLY_FP, 35, 3, 2, 1, PTW_FP, PCL_FP, 0)           \
    X(CT_BUTTERFLY_FP_NR, 36, 3, 2, 1, PTW_FP, PCL_FP, 0)        \
    X(GS_BUTTERFLY_FP, 37, 3, 2, 1, PTW_FP, PCL_FP, 0)           \
    X(RADIX_FORWARD_FP4, 38, 31, 16, 15, PTW_FP, PCL_FP, 0)      \
    X(RADIX_INVERSE_FP4, 39, 31, 16, 15, PTW_FP, PCL_FP, 0)

enum ProbeOp : uint32_t {
#define X(name, id, n_in, n_out, n_tw, tw, cls, host) POP_##name = id,
    MK_PROBE_OPS(X)
#undef X
        POP_COUNT = 40
};

struct ProbeDesc {
    uint32_t n_in, n_out, n_tw, tw, cls, host;
};
// false for an unknown op
inline bool probe_desc(uint32_t op, ProbeDesc &d) {
    switch (op) {
#define X(name, id, n_in, n_out, n_tw, tw, cls, host) \
    case id: d = ProbeDesc{n_in, n_out, n_tw, tw, cls, host}; return true;
        MK_PROBE_OPS(X)
#undef X
        default: return false;
    }
}

struct ProbeK {  // wave-uniform constants of the probed modulus
    LimbConst lc;
    PmK P;  // valid for the pseudo-Mersenne ops only
};

// element i of the ops that have a host form; `in` holds the expanded planes [.][n], `out` the output planes [.][n]
template <uint32_t OP>
MK_HD void probe_hd(const ProbeK &K, const u64 *in, u64 *out, size_t n, size_t i) {
    const LimbConst &L = K.lc;
    auto I = [&](int p) { return in[(size_t)p * n + i]; };
    auto O = [&](int p, u64 v) { out[(size_t)p * n + i] = v; };
    if constexpr (OP == POP_CSUB) O(0, csub(I(0), I(1)));
    else if constexpr (OP == POP_ADD_MOD) O(0, add_mod(I(0), I(1), L.q));
    else if constexpr (OP == POP_SUB_MOD) O(0, sub_mod(I(0), I(1), L.q));
    else if constexpr (OP == POP_SHOUP_LAZY) O(0, shoup_lazy(I(0), I(1), I(2), L.q));
    else if constexpr (OP == POP_SHOUP_MUL) O(0, shoup_mul(I(0), I(1), I(2), L.q));
    else if constexpr (OP == POP_MUL_MOD) O(0, mul_mod(I(0), I(1), L));
    else if constexpr (OP == POP_BARRETT_REDUCE128) O(0, barrett_reduce128(I(0), I(1), L));
    else if constexpr (OP == POP_REDUCE_WIDE) O(0, reduce_wide(I(0), I(1), L));
    else if constexpr (OP == POP_REDUCE_WORD) O(0, reduce_word(I(0), L));
    else if constexpr (OP == POP_REDUCE_COLS_LAZY) O(0, reduce_cols_lazy(Cols{I(0), I(1), I(2)}, L));
    else if constexpr (OP == POP_REDUCE_COLS) O(0, reduce_cols(Cols{I(0), I(1), I(2)}, L));
    else if constexpr (OP == POP_REDUCE_COLS4) O(0, reduce_cols4(Cols4{I(0), I(1), I(2), I(3)}, L));
    else if constexpr (OP == POP_MAC128 || OP == POP_MAC128_SPLIT) {
        u64 hi = I(0), lo = I(1);
        if constexpr (OP == POP_MAC128) mac128(hi, lo, I(2), I(3));
        else mac128_split(hi, lo, I(2), I(3));
        O(0, hi);
        O(1, lo);
    } else if constexpr (OP == POP_CT_BUTTERFLY_C4 || OP == POP_CT_BUTTERFLY_NC || OP == POP_GS_BUTTERFLY ||
                         OP == POP_CT_BUTTERFLY_PM_F || OP == POP_CT_BUTTERFLY_PM_N || OP == POP_GS_BUTTERFLY_PM) {
        u64 x = I(0), y = I(1);
        const u64 w = I(2), wc = I(3);
        if constexpr (OP == POP_CT_BUTTERFLY_C4) ct_butterfly_c4(x, y, w, wc, L.q, L.q2, L.q2 + L.q2);
        else if constexpr (OP == POP_CT_BUTTERFLY_NC) ct_butterfly_nc(x, y, w, wc, L.q, L.q2);
        else if constexpr (OP == POP_GS_BUTTERFLY) gs_butterfly(x, y, w, wc, L.q, L.q2);
        else if constexpr (OP == POP_CT_BUTTERFLY_PM_F) ct_butterfly_pm_f(x, y, w, wc, K.P);
        else if constexpr (OP == POP_CT_BUTTERFLY_PM_N) ct_butterfly_pm_n(x, y, w, wc, K.P);
        else gs_butterfly_pm(x, y, w, wc, K.P);
        O(0, x);
        O(1, y);
    } else if constexpr (OP == POP_CANON8) O(0, canon8(I(0), L.q, L.q2));
    else if constexpr (OP == POP_RADIX_FORWARD4 || OP == POP_RADIX_INVERSE4 || OP == POP_RADIX_FORWARD_PM4 ||
                       OP == POP_RADIX_INVERSE_PM4) {
        u64 x[16], w[15], wc[15];
#pragma unroll
        for (int k = 0; k < 16; ++k) x[k] = I(k);
#pragma unroll
        for (int k = 0; k < 15; ++k) {
            w[k] = I(16 + k);
            wc[k] = I(31 + k);
        }
        if constexpr (OP == POP_RADIX_FORWARD4) radix_forward<4>(x, w, wc, L.q, L.q2);
        else if constexpr (OP == POP_RADIX_INVERSE4) radix_inverse<4>(x, w, wc, L.q, L.q2);
        else if constexpr (OP == POP_RADIX_FORWARD_PM4) radix_forward_pm<4>(x, w, wc, K.P);
        else radix_inverse_pm<4>(x, w, wc, K.P);
#pragma unroll
        for (int k = 0; k < 16; ++k) O(k, x[k]);
    } else if constexpr (OP == POP_PM_FOLD) O(0, pm_fold(I(0), K.P));
    else if constexpr (OP == POP_PM_LAZY) O(0, pm_lazy(I(0), I(1), I(2), K.P));
    else if constexpr (OP == POP_PM_REDUCE128) O(0, pm_reduce128(I(0), I(1), K.P, L.q));
    else if constexpr (OP == POP_PM_REDUCE_COLS) O(0, pm_reduce_cols(Cols{I(0), I(1), I(2)}, K.P));
}

// element i of the device-only ops (fp64 class): doubles travel as bit patterns
template <uint32_t OP>
MK_D void probe_d(const ProbeK &K, const u64 *in, u64 *out, size_t n, size_t i) {
    const double q = K.lc.qd, qinv = K.lc.qinv;
    auto I = [&](int p) { return in[(size_t)p * n + i]; };
    auto O = [&](int p, u64 v) { out[(size_t)p * n + i] = v; };
    if constexpr (OP == POP_FP_MULMOD) O(0, dbits(fp_mulmod(bitsd(I(0)), bitsd(I(1)), bitsd(I(2)), q)));
    else if constexpr (OP == POP_FP_REDUCE) O(0, dbits(fp_reduce(bitsd(I(0)), q, qinv)));
    else if constexpr (OP == POP_FP_TO_CANONICAL) O(0, fp_to_canonical(bitsd(I(0)), q, qinv));
    else if constexpr (OP == POP_FP_MULMOD_ANY) O(0, dbits(fp_mulmod_any(bitsd(I(0)), bitsd(I(1)), q, qinv)));
    else if constexpr (OP == POP_U52_TO_DOUBLE) O(0, dbits(u52_to_double(I(0))));
    else if constexpr (OP == POP_SPLIT30_D) {
        uint32_t lo, hi;
        split30_d(I(0), lo, hi);
        O(0, lo);
        O(1, hi);
    } else if constexpr (OP == POP_CT_BUTTERFLY_FP || OP == POP_CT_BUTTERFLY_FP_NR || OP == POP_GS_BUTTERFLY_FP) {
        u64 x = I(0), y = I(1);
        if constexpr (OP == POP_CT_BUTTERFLY_FP) ct_butterfly_fp(x, y, I(2), I(3), q, qinv);
        else if constexpr (OP == POP_CT_BUTTERFLY_FP_NR) ct_butterfly_fp_nr(x, y, I(2), I(3), q);
        else gs_butterfly_fp(x, y, I(2), I(3), q, qinv);
        O(0, x);
        O(1, y);
    } else if constexpr (OP == POP_RADIX_FORWARD_FP4 || OP == POP_RADIX_INVERSE_FP4) {
        u64 x[16], w[15], wc[15];
#pragma unroll
        for (int k = 0; k < 16; ++k) x[k] = I(k);
#pragma unroll
        for (int k = 0; k < 15; ++k) {
            w[k] = I(16 + k);
            wc[k] = I(31 + k);
        }
        if constexpr (OP == POP_RADIX_FORWARD_FP4) radix_forward_fp<4>(x, w, wc, q, qinv);
        else radix_inverse_fp<4>(x, w, wc, q, qinv);
#pragma unroll
        for (int k = 0; k < 16; ++k) O(k, x[k]);
    }
}

constexpr int PROBE_THREADS = 256;
// HD_FORM: the op is written as an MK_HD function (probe_hd); what runs here is its DEVICE form either way
template <uint32_t OP, bool HD_FORM>
__global__ __launch_bounds__(PROBE_THREADS) void k_arith_probe(ProbeK K, const u64 *__restrict__ in, u64 *__restrict__ out,
                                                               size_t n) {
    for (size_t i = (size_t)blockIdx.x * PROBE_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * PROBE_THREADS) {
        if constexpr (HD_FORM) probe_hd<OP>(K, in, out, n, i);
        else probe_d<OP>(K, in, out, n, i);
    }
}

}  // namespace mk
