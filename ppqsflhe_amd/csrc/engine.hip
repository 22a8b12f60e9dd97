// engine.hip -- gfx950 kernels + launch sequences for the PRE / aggregation hot path.
//
// Reference call sites replaced (paths relative to /root/reference; OpenFHE internals
// are [upstream]):
//   changeCipherDomain.cpp:74,89,105        cc->ReEncrypt       -> Engine::reencrypt
//   aggregateEncryptedWeights.cpp:82,91,106 cc->EvalAdd         -> Engine::eval_add / eval_sum
//   aggregateEncryptedWeights.cpp:83,92,107 cc->EvalMult(.,0.5) -> Engine::rescale (+ factors)
//   aggregateEncryptedWeights.cpp:82-83     cc->EvalMult(.,pt)  -> Engine::mult_plain / mult_plain_rescale (per-slot weights)
//   encryptModelWeights.cpp:83,91,110       cc->Encrypt         -> Engine::encrypt (+ lift_ntt)
//   decryptModelWeights.cpp:81,90,108       cc->Decrypt         -> Engine::decrypt
//   keyGen.cpp:33 / REkeyGen.cpp:52         KeyGen / ReKeyGen   -> Engine::keygen / rekeygen
//
// Data layout in HBM: limb-major u64, one limb = N contiguous words, so every kernel
// streams 8-B (or 16-B) words with unit stride per lane; the limb (modulus) is uniform per
// workgroup (blockIdx.y), so all per-limb constants sit in SGPRs.
#include "engine.hpp"
#include "comm.hpp"
#include "dispatch.hpp"
#include "ntt_radix.hpp"
#include "qsum_kernels.hpp"
#include "fanout_kernels.hpp"
#include "codec_kernels.hpp"
#include "galois_kernels.hpp"
#include "tensor_kernels.hpp"
#include "lintrans_kernels.hpp"
#include "bsgs_kernels.hpp"
#include "poly_kernels.hpp"
#include "cheb_kernels.hpp"
#include "relshare_kernels.hpp"
#include "sampler_kernels.hpp"
#include "arith_probe_kernels.hpp"
#include "../../include/mkckks.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <type_traits>
#include <cstdlib>
#include <cstring>

namespace mk {

// =====================================================================================
// NTT kernels (schedule described in ntt_kernels.hpp)
// =====================================================================================

template <bool INV>
__global__ __launch_bounds__(NTT_THREADS) void k_ntt_col(NttIo io, NttTables T, const u64 *scale,
                                                         const u64 *scale_sh) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const uint32_t poly = blockIdx.y / io.nslots, s = blockIdx.y % io.nslots;
    if (ntt_slot_skipped(io, poly, io.vslot0 + s)) return;  // block-uniform
    const uint32_t id = limb_id_of(io.vslot0 + s, io.nl, T.L);
    const LimbConst lc = T.limb[id];
    const uint32_t n = 1u << T.log_n, r1 = 1u << T.log_r1, r2 = 1u << T.log_r2;
    const u64 *src = io.in + (size_t)poly * io.in_stride + (size_t)(io.in_slot0 + s) * n;
    u64 *dst = io.out + (size_t)poly * io.out_stride + (size_t)(io.out_slot0 + s) * n;
    const uint32_t c0 = blockIdx.x * NTT_COLS;
    const uint32_t pairs = r1 * (NTT_COLS / 2);
    for (uint32_t e = threadIdx.x; e < pairs; e += NTT_THREADS) {
        const uint32_t r = e / (NTT_COLS / 2), cp = (e % (NTT_COLS / 2)) * 2;
        const ulong2 v = *reinterpret_cast<const ulong2 *>(src + (size_t)r * r2 + c0 + cp);
        lds[r * NTT_COLS + cp] = v.x;
        lds[r * NTT_COLS + cp + 1] = v.y;
    }
    __syncthreads();
    const u64 *tw = (INV ? T.itw : T.tw) + (size_t)id * n;
    const u64 *tw_sh = (INV ? T.itw_sh : T.tw_sh) + (size_t)id * n;
    lds_stages<INV>(lds, NTT_COLS, (int)T.log_r1, 1, NTT_COLS, true, tw, tw_sh, lc.q, lc.q2,
                    [](int) { return 1; });
    u64 sc = 0, sc_sh = 0;
    if (INV) {
        sc = scale ? scale[id] : lc.ninv;
        sc_sh = scale ? scale_sh[id] : lc.ninv_sh;
    }
    for (uint32_t e = threadIdx.x; e < pairs; e += NTT_THREADS) {
        const uint32_t r = e / (NTT_COLS / 2), cp = (e % (NTT_COLS / 2)) * 2;
        ulong2 v;
        v.x = lds[r * NTT_COLS + cp];
        v.y = lds[r * NTT_COLS + cp + 1];
        if (INV) {  // last pass of the inverse: scale by N^-1 (x folded constant), canonical
            v.x = shoup_mul(v.x, sc, sc_sh, lc.q);
            v.y = shoup_mul(v.y, sc, sc_sh, lc.q);
        }
        *reinterpret_cast<ulong2 *>(dst + (size_t)r * r2 + c0 + cp) = v;
    }
}

template <bool INV>
__global__ __launch_bounds__(NTT_THREADS) void k_ntt_row(NttIo io, NttTables T) {
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    const uint32_t poly = blockIdx.y / io.nslots, s = blockIdx.y % io.nslots;
    if (ntt_slot_skipped(io, poly, io.vslot0 + s)) return;  // block-uniform
    const uint32_t id = limb_id_of(io.vslot0 + s, io.nl, T.L);
    const LimbConst lc = T.limb[id];
    const uint32_t n = 1u << T.log_n, r1 = 1u << T.log_r1, r2 = 1u << T.log_r2;
    const uint32_t tile = n < (uint32_t)NTT_TILE ? n : (uint32_t)NTT_TILE;
    const uint32_t rows = tile >> T.log_r2, row0 = blockIdx.x * rows;
    const u64 *src = io.in + (size_t)poly * io.in_stride + (size_t)(io.in_slot0 + s) * n + (size_t)row0 * r2;
    u64 *dst = io.out + (size_t)poly * io.out_stride + (size_t)(io.out_slot0 + s) * n + (size_t)row0 * r2;
    for (uint32_t e = threadIdx.x; e < tile / 2; e += NTT_THREADS) {
        const ulong2 v = reinterpret_cast<const ulong2 *>(src)[e];
        lds[2 * e] = v.x;
        lds[2 * e + 1] = v.y;
    }
    __syncthreads();
    const u64 *tw = (INV ? T.itw : T.tw) + (size_t)id * n;
    const u64 *tw_sh = (INV ? T.itw_sh : T.tw_sh) + (size_t)id * n;
    const int base0 = (int)(r1 + row0);
    lds_stages<INV>(lds, (int)rows, (int)T.log_r2, (int)r2, 1, false, tw, tw_sh, lc.q, lc.q2,
                    [base0](int g) { return base0 + g; });
    for (uint32_t e = threadIdx.x; e < tile / 2; e += NTT_THREADS) {
        ulong2 v;
        v.x = lds[2 * e];
        v.y = lds[2 * e + 1];
        if (!INV) {  // last pass of the forward transform: [0,8q) -> [0,q)
            v.x = canon8(v.x, lc.q, lc.q2);
            v.y = canon8(v.y, lc.q, lc.q2);
        }
        reinterpret_cast<ulong2 *>(dst)[e] = v;
    }
}

// =====================================================================================
// coefficient-wise kernels.  grid = (N / (2*256), slots, items); one modulus per block.
// =====================================================================================

constexpr int EW_THREADS = 256;

struct EwGeom {
    uint32_t n, nl, L;
};

#define EW_PROLOGUE(nslots_)                                                   \
    const uint32_t slot = blockIdx.y, item = blockIdx.z;                       \
    const uint32_t idx = (blockIdx.x * EW_THREADS + threadIdx.x) * 2;          \
    if (idx >= g.n) return;                                                    \
    (void)slot; (void)item;

__device__ __forceinline__ ulong2 ld2(const u64 *p) { return *reinterpret_cast<const ulong2 *>(p); }
__device__ __forceinline__ void st2(u64 *p, ulong2 v) { *reinterpret_cast<ulong2 *>(p) = v; }

// out = a + b over [items][slots][N]   (EvalAddCore)
__global__ void k_add(const u64 *a, const u64 *b, u64 *out, EwGeom g, const LimbConst *limb, uint32_t slots) {
    EW_PROLOGUE(slots)
    const u64 q = limb[limb_id_of(slot % g.nl, g.nl, g.L)].q;
    const size_t off = ((size_t)item * slots + slot) * g.n + idx;
    ulong2 x = ld2(a + off), y = ld2(b + off);
    x.x = add_mod(x.x, y.x, q);
    x.y = add_mod(x.y, y.y, q);
    st2(out + off, x);
}

// out[item][slot] = sum_k in[k][item][slot]  (n-ary EvalAdd; lazy u64 sum of < 2^61 terms, one reduction)
__global__ void k_sum(const u64 *in, u64 *out, EwGeom g, const LimbConst *limb, uint32_t slots,
                      uint32_t n_clients, size_t client_stride) {
    EW_PROLOGUE(slots)
    const LimbConst lc = limb[limb_id_of(slot % g.nl, g.nl, g.L)];
    const size_t off = ((size_t)item * slots + slot) * g.n + idx;
    u64 s0 = 0, s1 = 0;
    uint32_t pending = 0;
    for (uint32_t k = 0; k < n_clients; ++k) {
        const ulong2 v = ld2(in + (size_t)k * client_stride + off);
        s0 += v.x;
        s1 += v.y;
        if (++pending == 4) {  // 4 canonical terms + 1 reduced carry < 5 * 2^61 < 2^64
            s0 = reduce_word(s0, lc);
            s1 = reduce_word(s1, lc);
            pending = 1;
        }
    }
    ulong2 r;
    r.x = reduce_word(s0, lc);
    r.y = reduce_word(s1, lc);
    st2(out + off, r);
}

// out[slot] (+)= sum_{j < cnt} w[j][slot - slot0] * in[j][slot] over Q limbs slot0 + blockIdx.y (slot == limb id), one
// polynomial u64[nl][N] per input (combine_key_shares).  Weights: canonical residues by value in the kernel arguments,
// WSUM_IN inputs x WSUM_LIMBS limbs per launch (2 KiB); further inputs accumulate into `out`.  Every term is mul_mod
// of two canonical residues, summed canonically.  A thread reads its words of every input (and of `out` when it
// accumulates) before it writes them: out may be in[0].
constexpr uint32_t WSUM_IN = 16, WSUM_LIMBS = 16;
struct WsumTable {
    u64 w[WSUM_IN][WSUM_LIMBS];
};
__global__ void k_wsum(const u64 *in, u64 *out, EwGeom g, const LimbConst *limb, uint32_t slot0, uint32_t cnt,
                       size_t in_stride, int accumulate, WsumTable t) {
    const uint32_t ls = blockIdx.y, slot = slot0 + ls;
    const uint32_t idx = (blockIdx.x * EW_THREADS + threadIdx.x) * 2;
    if (idx >= g.n) return;
    const LimbConst lc = limb[slot];
    const size_t off = (size_t)slot * g.n + idx;
    ulong2 r{0, 0};
    if (accumulate) r = ld2(out + off);
    for (uint32_t j = 0; j < cnt; ++j) {
        const ulong2 v = ld2(in + (size_t)j * in_stride + off);
        const u64 w = t.w[j][ls];
        r.x = add_mod(r.x, mul_mod(v.x, w, lc), lc.q);
        r.y = add_mod(r.y, mul_mod(v.y, w, lc), lc.q);
    }
    st2(out + off, r);
}

// Weight tables of the weighted aggregation (Engine::weight_table): entry (k, limb id) = 4 words
// { M_k mod q, Shoup companion, [P M_k mod q] as a double, that / q } -- the doubles on fp64-class Q limbs only.
constexpr uint32_t WT_WORDS = 4;

// out[key][j][comp][limb] = (M_key mod m_limb) * in[key][j][comp][limb] on all D limbs of an eval key u64[beta][2][D][N]:
// grid (N / 512, D, n_keys * beta * 2), one limb per workgroup, streamed once (non-temporal both ways).
__global__ void k_scale_keys(const u64 *in, u64 *out, uint32_t n, uint32_t D, uint32_t polys_per_key, const LimbConst *limb,
                             const u64 *wt) {
    const uint32_t l = blockIdx.y, poly = blockIdx.z;
    const uint32_t idx = (blockIdx.x * EW_THREADS + threadIdx.x) * 2;
    if (idx >= n) return;
    const u64 q = limb[l].q;
    const u64 *w = wt + ((size_t)(poly / polys_per_key) * D + l) * WT_WORDS;
    const u64 f = w[0], f_sh = w[1];
    const size_t off = ((size_t)poly * D + l) * n + idx;
    ulong2 v = ld_stream2(reinterpret_cast<const ulong2 *>(in + off));
    v.x = shoup_mul(v.x, f, f_sh, q);
    v.y = shoup_mul(v.y, f, f_sh, q);
    st_stream2(reinterpret_cast<ulong2 *>(out + off), v);
}

// out[item] = (M mod q) * c0 of in[item], c1 copied: the input of the per-client weighted re-encryption on the shapes
// outside the merged flow.  in / out u64[items][2][nl][N]; w = the client's row of the weight table.
__global__ void k_scale_c0(const u64 *in, u64 *out, EwGeom g, const LimbConst *limb, const u64 *w) {
    EW_PROLOGUE(2 * g.nl)
    const size_t off = ((size_t)item * 2 * g.nl + slot) * g.n + idx;
    ulong2 v = ld_stream2(reinterpret_cast<const ulong2 *>(in + off));
    if (slot < g.nl) {
        const u64 q = limb[slot].q, f = w[slot * WT_WORDS], f_sh = w[slot * WT_WORDS + 1];
        v.x = shoup_mul(v.x, f, f_sh, q);
        v.y = shoup_mul(v.y, f, f_sh, q);
    }
    st2(out + off, v);
}

// out[item][slot] = sum_k (M_k mod q) * in[k][item][slot]: weighted n-ary EvalAdd, one pass over the n inputs and one
// write.  Every product is canonical (< q < 2^61), as is term 0 when it enters as it is (first_is_sum), so the u64 sums
// are reduced every 4 terms like k_sum's: 4 canonical terms + 1 reduced carry < 5 * 2^61 < 2^64.  A thread reads its
// words of every input before it writes them: out may be term 0.
__global__ void k_wsum_ct(const u64 *in, u64 *out, EwGeom g, const LimbConst *limb, uint32_t slots, uint32_t n_terms,
                          size_t term_stride, const u64 *wt, uint32_t wt_limbs, int first_is_sum) {
    EW_PROLOGUE(slots)
    const uint32_t l = slot % g.nl;
    const LimbConst lc = limb[l];
    const size_t off = ((size_t)item * slots + slot) * g.n + idx;
    u64 s0 = 0, s1 = 0;
    uint32_t pending = 0;
    for (uint32_t k = 0; k < n_terms; ++k) {
        ulong2 v = ld_stream2(reinterpret_cast<const ulong2 *>(in + (size_t)k * term_stride + off));
        if (k != 0 || !first_is_sum) {
            const u64 *w = wt + ((size_t)k * wt_limbs + l) * WT_WORDS;
            v.x = shoup_mul(v.x, w[0], w[1], lc.q);
            v.y = shoup_mul(v.y, w[0], w[1], lc.q);
        }
        s0 += v.x;
        s1 += v.y;
        if (++pending == 4) {
            s0 = reduce_word(s0, lc);
            s1 = reduce_word(s1, lc);
            pending = 1;
        }
    }
    ulong2 r;
    r.x = reduce_word(s0, lc);
    r.y = reduce_word(s1, lc);
    st_stream2(reinterpret_cast<ulong2 *>(out + off), r);
}

// in-place word-wise reduction after an integer-sum collective
__global__ void k_reduce(u64 *ct, EwGeom g, const LimbConst *limb, uint32_t slots) {
    EW_PROLOGUE(slots)
    const LimbConst lc = limb[limb_id_of(slot % g.nl, g.nl, g.L)];
    const size_t off = ((size_t)item * slots + slot) * g.n + idx;
    ulong2 v = ld2(ct + off);
    v.x = reduce_word(v.x, lc);
    v.y = reduce_word(v.y, lc);
    st2(ct + off, v);
}

// ct[item][slot] *= f[slot % nl]   (EvalMultCoreInPlace with a per-limb integer constant)
__global__ void k_mul_const(u64 *ct, EwGeom g, const LimbConst *limb, uint32_t slots, const u64 *f,
                            const u64 *f_sh) {
    EW_PROLOGUE(slots)
    const uint32_t l = slot % g.nl;
    const u64 q = limb[limb_id_of(l, g.nl, g.L)].q;
    const size_t off = ((size_t)item * slots + slot) * g.n + idx;
    ulong2 v = ld2(ct + off);
    v.x = shoup_mul(v.x, f[l], f_sh[l], q);
    v.y = shoup_mul(v.y, f[l], f_sh[l], q);
    st2(ct + off, v);
}

// out[item][k][l] = in[item][k][l] * pt[item % n_pt][l]   (EvalMult(ct, plaintext) core: the pointwise product of
// canonical residues, mul_mod in every arithmetic class; out may be in)
__global__ void k_mul_plain(const u64 *in, const u64 *pt, u64 *out, EwGeom g, const LimbConst *limb, uint32_t slots,
                            uint32_t n_pt) {
    EW_PROLOGUE(slots)
    const uint32_t l = slot % g.nl;
    const LimbConst lc = limb[limb_id_of(l, g.nl, g.L)];
    const size_t off = ((size_t)item * slots + slot) * g.n + idx;
    const ulong2 m = ld2(pt + ((size_t)(item % n_pt) * g.nl + l) * g.n + idx);
    ulong2 v = ld2(in + off);
    v.x = mul_mod(v.x, m.x, lc);
    v.y = mul_mod(v.y, m.y, lc);
    st2(out + off, v);
}

// NativeVectorT::SwitchModulus of the dropped limb (COEFFICIENT format) into limb `slot`:
// centred lift, v > floor(q_last/2) is negative.  last: [items][N]; out: [items][nl-1][N]
__global__ void k_switch_modulus(const u64 *last, u64 *out, EwGeom g, const LimbConst *limb, u64 q_last) {
    EW_PROLOGUE(g.nl - 1)
    const LimbConst lc = limb[slot];
    const u64 half = q_last >> 1;
    const u64 ql_mod = reduce_word(q_last, lc);
    const ulong2 v = ld2(last + (size_t)item * g.n + idx);
    ulong2 r;
    u64 a = reduce_word(v.x, lc);
    r.x = v.x > half ? sub_mod(a, ql_mod, lc.q) : a;
    a = reduce_word(v.y, lc);
    r.y = v.y > half ? sub_mod(a, ql_mod, lc.q) : a;
    st2(out + ((size_t)item * (g.nl - 1) + slot) * g.n + idx, r);
}

// DropLastElementAndScale tail: out[item][i] = (in[item][i] - tmp[item][i]) * c[i],
// c = q_last^-1 (times the EvalMult constant when the two are fused).  in: items in_ext slots apart (the first nl are
// this level's), tmp nl-1 slots; out nl-1 slots, item p at (p / group) * out_gstride + (p % group) * (nl-1) * N
// (group 0: packed).
__global__ void k_sub_mul(const u64 *in, uint32_t in_ext, const u64 *tmp, u64 *out, EwGeom g, const LimbConst *limb,
                          const u64 *c, const u64 *c_sh, uint32_t group, size_t out_gstride) {
    EW_PROLOGUE(g.nl - 1)
    const u64 q = limb[slot].q;
    const ulong2 x = ld2(in + ((size_t)item * in_ext + slot) * g.n + idx);
    const size_t off = ((size_t)item * (g.nl - 1) + slot) * g.n + idx;
    const ulong2 t = ld2(tmp + off);
    ulong2 r;
    r.x = shoup_mul(sub_mod(x.x, t.x, q), c[slot], c_sh[slot], q);
    r.y = shoup_mul(sub_mod(x.y, t.y, q), c[slot], c_sh[slot], q);
    const size_t o = group ? (size_t)(item / group) * out_gstride + ((size_t)(item % group) * (g.nl - 1) + slot) * g.n + idx : off;
    st2(out + o, r);
}

// ApproxModDown tail: out[item][i] = (in[item][i] - conv[item][i]) * Pinv[i] (+ add[item/2][i] on even items).
// in has ext = nl+K slots per item, conv/out have nl.
__global__ void k_moddown_tail(const u64 *in, const u64 *conv, u64 *out, EwGeom g, const LimbConst *limb,
                               uint32_t ext, const u64 *pinv, const u64 *pinv_sh, const u64 *add,
                               size_t add_stride, size_t out_item_stride, int accumulate) {
    EW_PROLOGUE(g.nl)
    const u64 q = limb[slot].q;
    const ulong2 x = ld2(in + ((size_t)item * ext + slot) * g.n + idx);
    const ulong2 t = ld2(conv + ((size_t)item * g.nl + slot) * g.n + idx);
    ulong2 r;
    r.x = shoup_mul(sub_mod(x.x, t.x, q), pinv[slot], pinv_sh[slot], q);
    r.y = shoup_mul(sub_mod(x.y, t.y, q), pinv[slot], pinv_sh[slot], q);
    if (add && (item & 1) == 0) {
        const ulong2 c = ld2(add + (size_t)(item >> 1) * add_stride + (size_t)slot * g.n + idx);
        r.x = add_mod(r.x, c.x, q);
        r.y = add_mod(r.y, c.y, q);
    }
    u64 *o = out + (size_t)item * out_item_stride + (size_t)slot * g.n + idx;
    if (accumulate) {
        const ulong2 a = ld2(o);
        r.x = add_mod(r.x, a.x, q);
        r.y = add_mod(r.y, a.y, q);
    }
    st2(o, r);
}

// copy selected limb slots between strided polynomial arrays
__global__ void k_copy_slots(const u64 *in, size_t in_stride, uint32_t in_slot0, u64 *out, size_t out_stride,
                             uint32_t out_slot0, uint32_t n) {
    const uint32_t slot = blockIdx.y, item = blockIdx.z;
    const uint32_t idx = (blockIdx.x * EW_THREADS + threadIdx.x) * 2;
    if (idx >= n) return;
    st2(out + (size_t)item * out_stride + (size_t)(out_slot0 + slot) * n + idx,
        ld2(in + (size_t)item * in_stride + (size_t)(in_slot0 + slot) * n + idx));
}

// =====================================================================================
// hybrid key switching kernels
// =====================================================================================

// ApproxSwitchCRTBasis: one thread per coefficient.  in: [items][*][N] COEFFICIENT, canonical.
template <int N_IN>
__global__ void k_baseconv(const u64 *in, size_t in_stride, u64 *out, size_t out_stride, DevConv cv,
                           const LimbConst *limb, uint32_t n, int prescaled) {
    const uint32_t idx = blockIdx.x * EW_THREADS + threadIdx.x;
    const uint32_t item = blockIdx.y;
    if (idx >= n) return;
    u64 t[N_IN];
#pragma unroll
    for (int i = 0; i < N_IN; ++i) {
        const u64 x = in[(size_t)item * in_stride + (size_t)cv.src_slot[i] * n + idx];
        // prescaled: the inverse transform already folded [(S/s_i)^-1]_{s_i} into its N^-1 scaling
        t[i] = prescaled ? x : shoup_mul(x, cv.hatinv[i], cv.hatinv_sh[i], limb[cv.src_id[i]].q);
    }
    for (uint32_t j = 0; j < cv.n_out; ++j) {
        u64 hi = 0, lo = 0;
#pragma unroll
        for (int i = 0; i < N_IN; ++i) mac128(hi, lo, t[i], cv.hat[i * cv.n_out + j]);
        out[(size_t)item * out_stride + (size_t)cv.dst_slot[j] * n + idx] = reduce_wide(hi, lo, limb[cv.dst_id[j]]);
    }
}

// EvalFastKeySwitchCoreExt, batch form: one workgroup owns a (limb, coefficient range) and keeps the eval-key
// words b_j, a_j of all NPARTS digits in registers while it walks the `items` ciphertexts of the batch, so the
// eval key is streamed from HBM once per launch instead of once per ciphertext.  The digit's own limbs are read
// straight from c1 (no copy into the digit buffer).
template <int NPARTS>
__global__ void k_inner_product_b(const u64 *digits, const u64 *c1, size_t c1_stride, const u64 *evk, u64 *ctilde,
                                  EwGeom g, const LimbConst *limb, uint32_t ext, uint32_t D, uint32_t alpha,
                                  uint32_t items, unsigned long long slot_mask) {
    const uint32_t slot = nth_set_bit(slot_mask, blockIdx.y);  // the slots this launch covers
    const uint32_t idx = (blockIdx.x * EW_THREADS + threadIdx.x) * 2;
    if (idx >= g.n) return;
    const uint32_t id = limb_id_of(slot, g.nl, g.L);
    const LimbConst lc = limb[id];
    const int own = slot < g.nl ? (int)(slot / alpha) : -1;
    ulong2 b[NPARTS], a[NPARTS];
#pragma unroll
    for (int j = 0; j < NPARTS; ++j) {
        b[j] = ld2(evk + (((size_t)j * 2 + 0) * D + id) * g.n + idx);
        a[j] = ld2(evk + (((size_t)j * 2 + 1) * D + id) * g.n + idx);
    }
    for (uint32_t item = 0; item < items; ++item) {
        u64 h0x = 0, l0x = 0, h0y = 0, l0y = 0, h1x = 0, l1x = 0, h1y = 0, l1y = 0;
#pragma unroll
        for (int j = 0; j < NPARTS; ++j) {
            const ulong2 d = (j == own) ? ld2(c1 + (size_t)item * c1_stride + (size_t)slot * g.n + idx)
                                        : ld2(digits + (((size_t)item * NPARTS + j) * ext + slot) * g.n + idx);
            mac128_split(h0x, l0x, d.x, b[j].x);
            mac128_split(h0y, l0y, d.y, b[j].y);
            mac128_split(h1x, l1x, d.x, a[j].x);
            mac128_split(h1y, l1y, d.y, a[j].y);
        }
        ulong2 r0, r1;
        if (NPARTS <= 4) {
            r0.x = reduce_sum4(h0x, l0x, lc);
            r0.y = reduce_sum4(h0y, l0y, lc);
            r1.x = reduce_sum4(h1x, l1x, lc);
            r1.y = reduce_sum4(h1y, l1y, lc);
        } else {
            r0.x = reduce_wide(h0x, l0x, lc);
            r0.y = reduce_wide(h0y, l0y, lc);
            r1.x = reduce_wide(h1x, l1x, lc);
            r1.y = reduce_wide(h1y, l1y, lc);
        }
        st2(ctilde + (((size_t)item * 2 + 0) * ext + slot) * g.n + idx, r0);
        st2(ctilde + (((size_t)item * 2 + 1) * ext + slot) * g.n + idx, r1);
    }
}

// =====================================================================================
// key generation / encryption / decryption kernels
// =====================================================================================

__device__ __forceinline__ u64 lift_value(int8_t v, const LimbConst &lc) {
    return v == 0 ? 0 : (v > 0 ? 1 : lc.q - 1);
}
__device__ __forceinline__ u64 lift_value(int32_t v, const LimbConst &lc) {
    const u64 m = reduce_word((u64)(v < 0 ? -(int64_t)v : (int64_t)v), lc);
    return (v < 0 && m != 0) ? lc.q - m : m;
}
__device__ __forceinline__ u64 lift_value(int64_t v, const LimbConst &lc) { return lift_signed(v, lc); }  // |v| < 2^63
// exact residue of round(x) for a double x (|x| < 2^120): mantissa * 2^e reduced in 128 bits
__device__ __forceinline__ u64 lift_value(double x, const LimbConst &lc) {
    const double r = round(x);
    const bool neg = r < 0;
    const double a = fabs(r);
    u64 m;
    if (a < 9223372036854775808.0) {
        m = reduce_word((u64)a, lc);
    } else {
        int e;
        const double f = frexp(a, &e);                 // a = f * 2^e, f in [0.5,1)
        const u64 mant = (u64)ldexp(f, 53);            // 53-bit integer mantissa
        const int sh = e - 53;                         // a = mant * 2^sh, 11 <= sh <= 67
        const u64 hi = sh >= 64 ? (mant << (sh - 64)) : (mant >> (64 - sh));
        const u64 lo = sh >= 64 ? 0 : (mant << sh);
        m = reduce_wide(hi, lo, lc);
    }
    return (neg && m != 0) ? lc.q - m : m;
}

// signed coefficient vectors -> residues: coef [items][N] -> out [items][ext][N]
template <typename T>
__global__ void k_lift(const T *coef, u64 *out, EwGeom g, const LimbConst *limb, uint32_t ext) {
    EW_PROLOGUE(ext)
    const LimbConst lc = limb[limb_id_of(slot, g.nl, g.L)];
    const T *c = coef + (size_t)item * g.n + idx;
    ulong2 r;
    r.x = lift_value(c[0], lc);
    r.y = lift_value(c[1], lc);
    st2(out + ((size_t)item * ext + slot) * g.n + idx, r);
}

// out = x*y + z (+ w*wc) over limb ids; every operand addressed by (base, item stride, slot->offset rule)
struct Opnd {
    const u64 *p;
    size_t item_stride;  // words between items (0 = broadcast)
    uint32_t by_id;      // 1: limb offset = limb id * N (keys over QP); 0: offset = slot * N
};
__device__ __forceinline__ ulong2 ld_op(const Opnd &o, uint32_t item, uint32_t slot, uint32_t id, uint32_t n,
                                        uint32_t idx) {
    return ld2(o.p + (size_t)item * o.item_stride + (size_t)(o.by_id ? id : slot) * n + idx);
}
__global__ void k_fma(Opnd x, Opnd y, Opnd z, Opnd w, const u64 *wc, int negate_xy, u64 *out,
                      size_t out_item_stride, uint32_t out_by_id, EwGeom g, const LimbConst *limb, uint32_t slots) {
    EW_PROLOGUE(slots)
    const uint32_t id = limb_id_of(slot, g.nl, g.L);
    const LimbConst lc = limb[id];
    const ulong2 a = ld_op(x, item, slot, id, g.n, idx), b = ld_op(y, item, slot, id, g.n, idx);
    ulong2 r;
    r.x = mul_mod(a.x, b.x, lc);
    r.y = mul_mod(a.y, b.y, lc);
    if (negate_xy) {
        r.x = r.x ? lc.q - r.x : 0;
        r.y = r.y ? lc.q - r.y : 0;
    }
    if (z.p) {
        const ulong2 c = ld_op(z, item, slot, id, g.n, idx);
        r.x = add_mod(r.x, c.x, lc.q);
        r.y = add_mod(r.y, c.y, lc.q);
    }
    if (w.p) {
        const ulong2 d = ld_op(w, item, slot, id, g.n, idx);
        const u64 k = wc ? wc[id] : 1;
        r.x = add_mod(r.x, wc ? mul_mod(d.x, k, lc) : d.x, lc.q);
        r.y = add_mod(r.y, wc ? mul_mod(d.y, k, lc) : d.y, lc.q);
    }
    st2(out + (size_t)item * out_item_stride + (size_t)(out_by_id ? id : slot) * g.n + idx, r);
}

// =====================================================================================
// Engine
// =====================================================================================

static int fast_log_h(uint32_t log_r, uint32_t other_extent);

// packed round-B twiddle table of the two-round row kernels (layout: NttTables::twb)
__global__ void k_pack_rowb(const u64 *tw, const u64 *tw_sh, u64 *out, uint32_t log_n, uint32_t log_r1, uint32_t log_h,
                            uint32_t limbs) {
    const uint32_t n = 1u << log_n, r1 = 1u << log_r1, H = 1u << log_h;
    const size_t total = (size_t)limbs * n, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // one (w, wp) pair each
    if (t >= total) return;
    const uint32_t j = (uint32_t)(t % H), i = (uint32_t)((t / H) % H), row = (uint32_t)((t / ((size_t)H * H)) % r1);
    const uint32_t limb = (uint32_t)(t / n);
    u64 w = 0, wp = 0;
    if (i < H - 1) {
        const uint32_t s = 31u - (uint32_t)__clz(i + 1), gq = i - ((1u << s) - 1);
        const uint32_t idx = ((((r1 + row) << log_h) + j) << s) + gq;
        w = tw[(size_t)limb * n + idx];
        wp = tw_sh[(size_t)limb * n + idx];
    }
    out[2 * t] = w;
    out[2 * t + 1] = wp;
}


static int fast_row(uint32_t log_r2, uint32_t rows);

static dim3 ew_grid(uint32_t n, uint32_t slots, uint32_t items) {
    return dim3((n / 2 + EW_THREADS - 1) / EW_THREADS, slots, items);
}

// "no HIP device" has one non-obvious cause worth naming: two copies of the HIP runtime in one process (PyTorch-ROCm
// ships its own libamdhip64 and loads it by path; this library links /opt/rocm's).  The copy initialised second finds no
// device.  /proc/self/maps tells.
static std::string hip_runtime_diagnosis() {
    std::vector<std::string> paths;
    if (FILE *f = std::fopen("/proc/self/maps", "r")) {
        char line[4096];
        while (std::fgets(line, sizeof line, f)) {
            const char *p = std::strstr(line, "libamdhip64");
            if (!p) continue;
            const char *start = std::strchr(line, '/');
            if (!start) continue;
            std::string path(start);
            while (!path.empty() && (path.back() == '\n' || path.back() == ' ')) path.pop_back();
            bool seen = false;
            for (const std::string &q : paths) seen = seen || q == path;
            if (!seen) paths.push_back(path);
        }
        std::fclose(f);
    }
    if (paths.size() < 2) return "";
    std::string msg = "; this process carries " + std::to_string(paths.size()) + " HIP runtimes (";
    for (size_t i = 0; i < paths.size(); ++i) msg += (i ? ", " : "") + paths[i];
    return msg + "): the one initialised second sees no device -- load the library that owns the device first (import torch "
                 "before libmkckks_hip.so, or link both against the same libamdhip64)";
}

// Switches are read ONCE, when a context is created (tests and A/B runs create a context under the switch).
static bool env_flag(const char *name, bool dflt) {
    const char *e = std::getenv(name);
    return e ? std::atoi(e) != 0 : dflt;
}
Knobs Knobs::from_env() {
    Knobs k;
    if (const char *e = std::getenv("MKCKKS_CHUNK")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= 64) k.chunk = (uint32_t)v;
    }
    if (const char *e = std::getenv("MKCKKS_QSUM_GROUP")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= 64) k.qsum_group = (uint32_t)v;
    }
    if (const char *e = std::getenv("MKCKKS_FANOUT_GROUP")) {
        const int v = std::atoi(e);
        if (v >= 1 && v <= 64) k.fanout_group = (uint32_t)v;
    }
    k.cu_affine = env_flag("MKCKKS_CU_AFFINE", k.cu_affine);
    k.generic_ntt = env_flag("MKCKKS_GENERIC_NTT", k.generic_ntt);
    k.no_pm = env_flag("MKCKKS_NO_PM", k.no_pm);
    k.no_fp64 = env_flag("MKCKKS_NO_FP64", k.no_fp64);
    if (const char *e = std::getenv("MKCKKS_Q0_WALK")) {
        if (!std::strcmp(e, "0")) k.q0_walk = 0;
        else if (!std::strcmp(e, "1")) k.q0_walk = 1;
    }
    if (const char *e = std::getenv("MKCKKS_PLAIN_FUSED")) {
        if (!std::strcmp(e, "0")) k.plain_fused = 0;
        else if (!std::strcmp(e, "1")) k.plain_fused = 1;
    }
    if (const char *e = std::getenv("MKCKKS_RELSHARE_FUSED")) {
        if (!std::strcmp(e, "0")) k.relshare_fused = 0;
        else if (!std::strcmp(e, "1")) k.relshare_fused = 1;
    }
    if (const char *e = std::getenv("MKCKKS_ICOL_CONV")) {
        if (e[0] >= '0' && e[0] <= '3' && !e[1]) k.icol_conv = e[0] - '0';
    }
    if (const char *e = std::getenv("MKCKKS_POLY_FUSED")) {
        if (!std::strcmp(e, "0")) k.poly_fused = 0;
        else if (!std::strcmp(e, "1")) k.poly_fused = 1;
    }
    if (const char *e = std::getenv("MKCKKS_CHEB_FUSED")) {
        if (!std::strcmp(e, "0")) k.cheb_fused = 0;
        else if (!std::strcmp(e, "1")) k.cheb_fused = 1;
    }
    if (const char *e = std::getenv("MKCKKS_LT_ORDER")) {
        if (e[0] >= '0' && e[0] <= '2' && !e[1]) k.lt_order = e[0] - '0';
    }
    if (const char *e = std::getenv("MKCKKS_BSGS_FUSED")) {
        if (!std::strcmp(e, "0")) k.bsgs_fused = 0;
        else if (!std::strcmp(e, "1")) k.bsgs_fused = 1;
    }
    if (const char *e = std::getenv("MKCKKS_BSGS_WS_MIB")) {
        const long v = std::atol(e);
        if (v >= 1 && v <= (1l << 20)) k.bsgs_ws_mib = (uint32_t)v;
    }
    return k;
}

Engine::Engine(const ParamSet &ps, int device) : ps_(ps), device_(device), knobs_(Knobs::from_env()) {
    if (device_ < 0) return;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= device_)
        throw NoDevice("no HIP device " + std::to_string(device_) + " (found " + std::to_string(count) + ")" +
                       hip_runtime_diagnosis());
    MK_HIP(hipSetDevice(device_));
    const uint32_t D = ps_.D, n = ps_.n;
    // N = R1 x R2 with R1 <= R2; even splits of even log N land on the radix-H kernels (16/64/256)
    tabs_.log_n = ps_.log_n;
    tabs_.log_r1 = (ps_.log_n % 2 == 0) ? ((ps_.log_n / 2) & ~1u) : ps_.log_n / 2;
    tabs_.log_r2 = ps_.log_n - tabs_.log_r1;
    if (knobs_.generic_ntt) { tabs_.log_r1 = ps_.log_n / 2; tabs_.log_r2 = ps_.log_n - tabs_.log_r1; }
    // fp64 limbs: only when BOTH passes run on the radix kernels (the generic LDS-stage kernels are integer-only)
    // and the modulus is below 1.25 * 2^50 (bounds in ntt_radix.hpp).  MKCKKS_NO_FP64=1 keeps everything integer.
    const bool radix_both = fast_log_h(tabs_.log_r1, 1u << tabs_.log_r2) && fast_row(tabs_.log_r2, 1u << tabs_.log_r1);
    const bool fp_ok = radix_both && !knobs_.no_fp64;
    tabs_.has_fp = 0;
    fp_of_.assign(D, 0);
    for (uint32_t i = 0; i < D; ++i) {
        ps_.limb[i].fp = (fp_ok && ps_.moduli[i] < (5ull << 48)) ? 1u : 0u;
        fp_of_[i] = (uint8_t)ps_.limb[i].fp;
        tabs_.has_fp |= ps_.limb[i].fp;
    }
    // integer limbs of the form 2^k - c (the 60-bit q_0 and P limbs OpenFHE generates): pseudo-Mersenne butterflies, if
    // EVERY integer limb of the context qualifies and both passes run on the radix kernels (the generic LDS-stage kernels
    // are Shoup-only) -- one integer arithmetic per context, chosen at launch (AR_PM / AR_INT kernel instances).
    // MKCKKS_NO_PM=1 keeps Shoup's.
    bool all_pm = radix_both && !knobs_.no_pm;
    for (uint32_t i = 0; i < D; ++i)
        if (!ps_.limb[i].fp && !pm_eligible(ps_.moduli[i])) all_pm = false;
    tabs_.int_pm = all_pm ? 1u : 0u;
    for (uint32_t i = 0; i < D; ++i) {
        const bool pm = all_pm && !ps_.limb[i].fp;
        ps_.limb[i].pm = pm ? 1u : 0u;
        ps_.limb[i].pm_c = pm ? (uint32_t)(((u64)1 << ps_.limb[i].k) - ps_.moduli[i]) : 0u;
    }
    tabs_.h_fp_of = fp_of_.data();
    tabs_.cu_affine = knobs_.cu_affine ? 1u : 0u;
    tabs_.stamps = nullptr;
    if (MK_STAMP && env_flag("MKCKKS_STAMPS", false)) {  // diagnostic build: phase stamps of the hot kernels (tools/stamps.py)
        MK_HIP(hipMalloc(&d_stamps_, (size_t)STAMP_REGIONS * STAMP_REGION * sizeof(unsigned long long)));
        MK_HIP(hipMemset(d_stamps_, 0, (size_t)STAMP_REGIONS * STAMP_REGION * sizeof(unsigned long long)));
        tabs_.stamps = d_stamps_;
    }
    MK_HIP(hipMalloc(&d_limb_, D * sizeof(LimbConst)));
    MK_HIP(hipMemcpy(d_limb_, ps_.limb.data(), D * sizeof(LimbConst), hipMemcpyHostToDevice));
    const size_t tbytes = (size_t)D * n * sizeof(u64);
    MK_HIP(hipMalloc(&d_tw_, tbytes));
    MK_HIP(hipMalloc(&d_tw_sh_, tbytes));
    MK_HIP(hipMalloc(&d_itw_, tbytes));
    MK_HIP(hipMalloc(&d_itw_sh_, tbytes));
    std::vector<u64> w, wsh;
    auto as_fp = [&](uint32_t i) {  // (w, Shoup companion) -> (double w, double w/q) bit patterns
        for (uint32_t k = 0; k < n; ++k) fp_table_entry(w[k], ps_.moduli[i], w[k], wsh[k]);
    };
    auto as_pm = [&](uint32_t i) {  // (w, Shoup companion) -> (w << t, (w * 2^32 mod q) << t), see pm_lazy
        for (uint32_t k = 0; k < n; ++k) pm_table_entry(w[k], ps_.limb[i], w[k], wsh[k]);
    };
    for (uint32_t i = 0; i < D; ++i) {
        ps_.twiddles(i, false, w, wsh);
        if (ps_.limb[i].fp) as_fp(i);
        if (ps_.limb[i].pm) as_pm(i);
        MK_HIP(hipMemcpy(d_tw_ + (size_t)i * n, w.data(), n * sizeof(u64), hipMemcpyHostToDevice));
        MK_HIP(hipMemcpy(d_tw_sh_ + (size_t)i * n, wsh.data(), n * sizeof(u64), hipMemcpyHostToDevice));
        ps_.twiddles(i, true, w, wsh);
        if (ps_.limb[i].fp) as_fp(i);
        if (ps_.limb[i].pm) as_pm(i);
        MK_HIP(hipMemcpy(d_itw_ + (size_t)i * n, w.data(), n * sizeof(u64), hipMemcpyHostToDevice));
        MK_HIP(hipMemcpy(d_itw_sh_ + (size_t)i * n, wsh.data(), n * sizeof(u64), hipMemcpyHostToDevice));
    }
    {   // encoding tables: rotation group 5^j mod 2N and the 2N-th roots of unity (fp64, computed on the host)
        const uint32_t slots = n / 2, M = 2 * n;
        std::vector<uint32_t> rot(slots);
        uint64_t pw = 1;
        for (uint32_t j = 0; j < slots; ++j) { rot[j] = (uint32_t)pw; pw = pw * 5 % M; }
        std::vector<double2> ksi(M + 1);
        const double pi = std::acos(-1.0);
        for (uint32_t k = 0; k <= M; ++k) {
            const double ang = 2.0 * pi * (double)k / (double)M;
            ksi[k] = double2{std::cos(ang), std::sin(ang)};
        }
        MK_HIP(hipMalloc(&d_rot_, slots * sizeof(uint32_t)));
        MK_HIP(hipMalloc(&d_ksi_, (M + 1) * sizeof(double2)));
        MK_HIP(hipMemcpy(d_rot_, rot.data(), slots * sizeof(uint32_t), hipMemcpyHostToDevice));
        MK_HIP(hipMemcpy(d_ksi_, ksi.data(), (M + 1) * sizeof(double2), hipMemcpyHostToDevice));
    }
    tabs_.twb = tabs_.itwb = nullptr;
    if (const int lh = fast_log_h(tabs_.log_r2, 1u << tabs_.log_r1)) {  // two-round row kernels: packed round-B tables
        MK_HIP(hipMalloc(&d_twb_, 2 * tbytes));
        MK_HIP(hipMalloc(&d_itwb_, 2 * tbytes));
        const size_t total = (size_t)D * n;
        const dim3 grid((unsigned)((total + 255) / 256));
        k_pack_rowb<<<grid, 256>>>(d_tw_, d_tw_sh_, d_twb_, ps_.log_n, tabs_.log_r1, (uint32_t)lh, D);
        k_pack_rowb<<<grid, 256>>>(d_itw_, d_itw_sh_, d_itwb_, ps_.log_n, tabs_.log_r1, (uint32_t)lh, D);
        MK_HIP(hipGetLastError());
        MK_HIP(hipDeviceSynchronize());
        tabs_.twb = d_twb_;
        tabs_.itwb = d_itwb_;
    }
    tabs_.limb = d_limb_;
    tabs_.tw = d_tw_; tabs_.tw_sh = d_tw_sh_; tabs_.itw = d_itw_; tabs_.itw_sh = d_itw_sh_;
    tabs_.L = ps_.L;
}

Engine::~Engine() {
    if (device_ < 0) return;
    (void)hipSetDevice(device_);
    (void)hipDeviceSynchronize();
    for (void *p : {(void *)d_limb_, (void *)d_tw_, (void *)d_tw_sh_, (void *)d_itw_, (void *)d_itw_sh_, (void *)ws_,
                    (void *)d_twb_, (void *)d_itwb_, (void *)d_stamps_,
                    (void *)d_rot_, (void *)d_ksi_, (void *)d_gal_s_, (void *)d_lt_g_})
        if (p) (void)hipFree(p);
    for (void *p : owned_) (void)hipFree(p);
    for (auto &kv : wt_cache_) (void)hipFree(kv.second);
    if (wtmp_) (void)hipFree(wtmp_);
    if (poly_buf_) (void)hipFree(poly_buf_);
    if (up_stream_) {
        (void)hipStreamDestroy(up_stream_);
        (void)hipStreamDestroy(down_stream_);
        for (uint32_t i = 0; i < COPY_RING; ++i) (void)hipEventDestroy(copy_ev_[i]);
        (void)hipEventDestroy(ev_fence_);
    }
}

void Engine::need_device() const {
    if (device_ < 0) throw NoDevice("host-only context: no device operations");
}

void Engine::sync() {
    need_device();
    MK_HIP(hipStreamSynchronize(stream_));
}
void *Engine::dev_alloc(size_t bytes) {
    need_device();
    void *p = nullptr;
    MK_HIP(hipMalloc(&p, bytes ? bytes : 8));
    return p;
}
void Engine::dev_free(void *p) {
    need_device();
    MK_HIP(hipStreamSynchronize(stream_));
    MK_HIP(hipFree(p));
}
void Engine::upload(void *d, const void *h, size_t bytes) {
    need_device();
    MK_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, stream_));
    MK_HIP(hipStreamSynchronize(stream_));
}
void Engine::download(void *h, const void *d, size_t bytes) {
    need_device();
    MK_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, stream_));
    MK_HIP(hipStreamSynchronize(stream_));
}

// ---- I/O pipeline -------------------------------------------------------------------
void Engine::copy_streams() {
    if (up_stream_) return;
    MK_HIP(hipStreamCreateWithFlags(&up_stream_, hipStreamNonBlocking));
    MK_HIP(hipStreamCreateWithFlags(&down_stream_, hipStreamNonBlocking));
    for (uint32_t i = 0; i < COPY_RING; ++i) MK_HIP(hipEventCreateWithFlags(&copy_ev_[i], hipEventDisableTiming));
    MK_HIP(hipEventCreateWithFlags(&ev_fence_, hipEventDisableTiming));
}
void *Engine::host_alloc(size_t bytes) {
    need_device();
    void *p = nullptr;
    MK_HIP(hipHostMalloc(&p, bytes ? bytes : 8, hipHostMallocDefault));
    return p;
}
void Engine::host_free(void *p) {
    need_device();
    if (p) MK_HIP(hipHostFree(p));
}
uint64_t Engine::enqueue_copy(void *dst, const void *src, size_t bytes, bool up) {
    need_device();
    copy_streams();
    const uint64_t t = next_ticket_;
    if (t > COPY_RING) {  // the ring slot's previous copy (ticket t - COPY_RING) must be over before its event is re-recorded
        MK_HIP(hipEventSynchronize(copy_ev_[t % COPY_RING]));
        done_ticket_ = std::max(done_ticket_, t - COPY_RING);
    }
    hipStream_t s = up ? up_stream_ : down_stream_;
    MK_HIP(hipMemcpyAsync(dst, src, bytes, up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, s));
    MK_HIP(hipEventRecord(copy_ev_[t % COPY_RING], s));
    ++next_ticket_;
    return t;
}
uint64_t Engine::upload_async(void *d, const void *h, size_t bytes) { return enqueue_copy(d, h, bytes, true); }
uint64_t Engine::download_async(void *h, const void *d, size_t bytes) { return enqueue_copy(h, d, bytes, false); }
bool Engine::copy_done(uint64_t ticket) {
    need_device();
    if (ticket == 0 || ticket >= next_ticket_) throw std::invalid_argument("unknown copy ticket");
    if (ticket <= done_ticket_ || ticket + COPY_RING < next_ticket_) return true;  // slot already recycled: waited for then
    const hipError_t e = hipEventQuery(copy_ev_[ticket % COPY_RING]);
    if (e == hipErrorNotReady) return false;
    MK_HIP(e);
    return true;
}
void Engine::copy_wait(uint64_t ticket) {
    need_device();
    if (ticket == 0 || ticket >= next_ticket_) throw std::invalid_argument("unknown copy ticket");
    if (ticket <= done_ticket_ || ticket + COPY_RING < next_ticket_) return;
    MK_HIP(hipEventSynchronize(copy_ev_[ticket % COPY_RING]));
}
void Engine::fence_uploads() {
    need_device();
    if (!up_stream_) return;
    MK_HIP(hipEventRecord(ev_fence_, up_stream_));
    MK_HIP(hipStreamWaitEvent(stream_, ev_fence_, 0));
}
void Engine::fence_compute() {
    need_device();
    copy_streams();
    MK_HIP(hipEventRecord(ev_fence_, stream_));
    MK_HIP(hipStreamWaitEvent(down_stream_, ev_fence_, 0));
}

// residues at or above their modulus, counted per workgroup and added to *bad (untrusted ciphertext files: the kernels
// assume canonical residues)
__global__ void k_count_noncanonical(const u64 *ct, EwGeom g, const LimbConst *limb, uint32_t slots, unsigned long long *bad) {
    EW_PROLOGUE(slots)
    const u64 q = limb[limb_id_of(slot % g.nl, g.nl, g.L)].q;
    const ulong2 v = ld2(ct + ((size_t)item * slots + slot) * g.n + idx);
    const unsigned long long wx = __ballot(v.x >= q), wy = __ballot(v.y >= q);  // one atomic per wave, and only for bad data
    if ((wx | wy) != 0 && (threadIdx.x & 63) == 0) atomicAdd(bad, (unsigned long long)(__popcll(wx) + __popcll(wy)));
}
uint64_t Engine::count_noncanonical(const u64 *ct, uint32_t n_ct, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!n_ct) return 0;
    unsigned long long *d_bad = reinterpret_cast<unsigned long long *>(workspace(1));
    MK_HIP(hipMemsetAsync(d_bad, 0, 8, stream_));
    EwGeom g{ps_.n, nl, ps_.L};
    k_count_noncanonical<<<ew_grid(ps_.n, 2 * nl, n_ct), EW_THREADS, 0, stream_>>>(ct, g, d_limb_, 2 * nl, d_bad);
    MK_HIP(hipGetLastError());
    unsigned long long h = 0;
    MK_HIP(hipMemcpyAsync(&h, d_bad, 8, hipMemcpyDeviceToHost, stream_));
    MK_HIP(hipStreamSynchronize(stream_));
    return h;
}

size_t Engine::debug_stamps(unsigned long long *h_out, uint32_t region) {
    need_device();
    if (!d_stamps_ || region >= STAMP_REGIONS) return 0;
    MK_HIP(hipDeviceSynchronize());
    MK_HIP(hipMemcpy(h_out, d_stamps_ + (size_t)region * STAMP_REGION, (size_t)STAMP_REGION * sizeof(unsigned long long),
                     hipMemcpyDeviceToHost));
    MK_HIP(hipMemset(d_stamps_ + (size_t)region * STAMP_REGION, 0, (size_t)STAMP_REGION * sizeof(unsigned long long)));
    return STAMP_REGION;
}

void Engine::check_nl(uint32_t nl) const {
    if (nl < 1 || nl > ps_.L) throw std::invalid_argument("nl out of range");
}

u64 *Engine::workspace(size_t words) {
    if (words > ws_words_) {
        MK_HIP(hipStreamSynchronize(stream_));
        if (ws_) MK_HIP(hipFree(ws_));
        ws_ = nullptr;
        ws_words_ = 0;
        MK_HIP(hipMalloc(&ws_, words * sizeof(u64)));
        ws_words_ = words;
    }
    return ws_;
}

u64 *Engine::chunk_buffer(size_t words) {
    if (words > wtmp_words_) {
        MK_HIP(hipStreamSynchronize(stream_));
        if (wtmp_) MK_HIP(hipFree(wtmp_));
        wtmp_ = nullptr;
        wtmp_words_ = 0;
        MK_HIP(hipMalloc(&wtmp_, words * sizeof(u64)));
        wtmp_words_ = words;
    }
    return wtmp_;
}

u64 *Engine::poly_buffer(size_t words) {
    if (words > poly_buf_words_) {
        MK_HIP(hipStreamSynchronize(stream_));
        if (poly_buf_) MK_HIP(hipFree(poly_buf_));
        poly_buf_ = nullptr;
        poly_buf_words_ = 0;
        MK_HIP(hipMalloc(&poly_buf_, words * sizeof(u64)));
        poly_buf_words_ = words;
    }
    return poly_buf_;
}

const u64 *Engine::limb_vector(const std::string &key, const std::vector<u64> &vals) {
    auto it = vec_cache_.find(key);
    if (it != vec_cache_.end()) return it->second;
    u64 *d = nullptr;
    MK_HIP(hipMalloc(&d, vals.size() * sizeof(u64)));
    MK_HIP(hipMemcpy(d, vals.data(), vals.size() * sizeof(u64), hipMemcpyHostToDevice));
    owned_.push_back(d);
    vec_cache_[key] = d;
    return d;
}

static DevConv to_dev(const BaseConvTable &t, const u64 *d_hat, const u64 *d_hat_fp) {
    if (t.src.size() > (size_t)MAX_CONV_IN || t.dst.size() > (size_t)MAX_CONV_OUT)
        throw std::invalid_argument("base conversion larger than supported");
    DevConv c{};
    c.n_in = (uint32_t)t.src.size();
    c.n_out = (uint32_t)t.dst.size();
    for (size_t i = 0; i < t.src.size(); ++i) {
        c.src_id[i] = t.src[i];
        c.hatinv[i] = t.hatinv[i];
        c.hatinv_sh[i] = t.hatinv_sh[i];
    }
    for (size_t j = 0; j < t.dst.size(); ++j) c.dst_id[j] = t.dst[j];
    c.hat = d_hat;
    c.hat_d = reinterpret_cast<const double *>(d_hat_fp);
    c.hatq_d = c.hat_d + t.hat.size();
    c.hat30_d = c.hatq_d + t.hat.size();
    return c;
}

const DevConv &Engine::modup_conv(uint32_t nl, uint32_t part, bool p_scaled) {
    auto key = std::make_pair(nl, part);
    auto &cache = p_scaled ? modup_ps_cache_ : modup_cache_;
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    BaseConvTable t = p_scaled ? ps_.modup_table_pscaled(nl, part) : ps_.modup_table(nl, part);
    const std::string tag = std::to_string(nl) + "_" + std::to_string(part) + (p_scaled ? "_ps" : "");
    const u64 *d_hat = limb_vector("modup_hat_" + tag, t.hat);
    DevConv c = to_dev(t, d_hat, limb_vector("modup_hatd_" + tag, hat_as_doubles(t, ps_.moduli)));
    const uint32_t lo = part * ps_.alpha;
    for (uint32_t i = 0; i < c.n_in; ++i) c.src_slot[i] = lo + i;  // slot inside the nl-limb input polynomial
    // targets: all slots of the extended polynomial except the digit's own
    uint32_t w = 0;
    for (uint32_t s = 0; s < nl + ps_.K; ++s)
        if (s < lo || s >= lo + c.n_in) c.dst_slot[w++] = s;
    return cache.emplace(key, c).first->second;
}

const DevConv &Engine::moddown_conv(uint32_t nl) {
    auto it = moddown_cache_.find(nl);
    if (it != moddown_cache_.end()) return it->second;
    BaseConvTable t = ps_.moddown_table(nl);
    const u64 *d_hat = limb_vector("moddown_hat_" + std::to_string(nl), t.hat);
    DevConv c = to_dev(t, d_hat, limb_vector("moddown_hatd_" + std::to_string(nl), hat_as_doubles(t, ps_.moduli)));
    for (uint32_t k = 0; k < c.n_in; ++k) c.src_slot[k] = k;
    for (uint32_t i = 0; i < c.n_out; ++i) c.dst_slot[i] = i;
    return moddown_cache_.emplace(nl, c).first->second;
}

// source-class pattern of a conversion for k_conv_col: 0 = all integer, 1 = all fp64, 2 = source 0 integer and
// the rest fp64; -1 = none of these (the caller then interchanges every source as packed 30-bit halves)
int Engine::conv_src_mode(const DevConv &cv) const {
    bool all_fp = true, all_int = true, rest_fp = true;
    for (uint32_t i = 0; i < cv.n_in; ++i) {
        const bool fp = fp_of_[cv.src_id[i]] != 0;
        all_fp = all_fp && fp;
        all_int = all_int && !fp;
        if (i > 0) rest_fp = rest_fp && fp;
    }
    if (all_int) return 0;
    if (all_fp) return 1;
    return (!fp_of_[cv.src_id[0]] && rest_fp) ? 2 : -1;
}

static void launch_baseconv(const u64 *in, size_t in_stride, u64 *out, size_t out_stride, const DevConv &cv,
                            const LimbConst *limb, uint32_t n, uint32_t items, int prescaled, hipStream_t s) {
    const dim3 grid((n + EW_THREADS - 1) / EW_THREADS, items);
    if (!dispatch<1, 2, 3, 4, 5, 6, 7, 8>(cv.n_in, [&](auto n_in) {
            k_baseconv<decltype(n_in)::value><<<grid, EW_THREADS, 0, s>>>(in, in_stride, out, out_stride, cv, limb, n, prescaled);
        }))
        throw std::invalid_argument("base conversion fan-in unsupported");
    MK_HIP(hipGetLastError());
}

// ---- transforms ---------------------------------------------------------------------

// radix-H register kernels exist for sub-transform sizes 16, 64, 256 (H = 4, 8, 16) and need at least
// S = 256/H columns (rows) for the column (row) pass; everything else takes the generic LDS-stage kernels.
static int fast_log_h(uint32_t log_r, uint32_t other_extent) {
    if (log_r != 4 && log_r != 6 && log_r != 8) return 0;
    const uint32_t h = 1u << (log_r / 2);
    return (256u / h) <= other_extent ? (int)(log_r / 2) : 0;
}
// row pass only: 512-point rows take the three-round radix-8 kernel (code 9)
static int fast_row(uint32_t log_r2, uint32_t rows) {
    if (log_r2 == 9 && rows >= 4) return 9;
    return fast_log_h(log_r2, rows);
}

// the integer instance of a radix kernel in the context's integer arithmetic: f(integral_constant<int, AR_PM | AR_INT>)
template <typename F>
static void with_int_arith(const NttTables &T, F &&f) {
    if (T.int_pm) f(std::integral_constant<int, AR_PM>{});
    else f(std::integral_constant<int, AR_INT>{});
}

// slots of `io` whose limb runs on the fp64 (want_fp) or the integer instance; fp_of: per-limb-id class (host copy)
static unsigned long long class_mask(const NttIo &io, const unsigned char *fp_of, uint32_t L, bool want_fp) {
    unsigned long long m = 0;
    for (uint32_t b = 0; b < io.nslots; ++b) {
        const uint32_t v = io.vslot0 + b, id = v < io.nl ? v : L + (v - io.nl);
        if ((fp_of[id] != 0) == want_fp) m |= 1ull << b;
    }
    return m;
}

// the slots of a pass (or the targets of a conversion) by arithmetic class
struct ClassMasks {
    unsigned long long integer = 0, fp = 0;
};
// classes: bit 0 keeps the integer limbs, bit 1 the fp64 limbs
static ClassMasks slot_classes(const NttIo &io, const NttTables &T, unsigned classes = 3) {
    ClassMasks m;
    if (classes & 1) m.integer = class_mask(io, T.h_fp_of, T.L, false);
    if (classes & 2) m.fp = class_mask(io, T.h_fp_of, T.L, true);
    return m;
}
// the first nl limbs of the chain
static ClassMasks limb_classes(uint32_t nl, const NttTables &T) {
    NttIo sel{};
    sel.nslots = sel.nl = nl;
    return slot_classes(sel, T);
}
static ClassMasks target_classes(const DevConv &cv, const NttTables &T, unsigned classes = 3) {
    ClassMasks m;
    for (uint32_t j = 0; j < cv.n_out; ++j) {
        const bool fp = T.h_fp_of[cv.dst_id[j]] != 0;
        if (fp && (classes & 2)) m.fp |= 1ull << j;
        if (!fp && (classes & 1)) m.integer |= 1ull << j;
    }
    return m;
}

// The integer and the fp64 instance of a pass touch disjoint limbs and are launched one after the other on the same
// stream (forking them onto two streams was measured slower: -5 %, event round trips): f(ar, mask, nsel) for each class
// that has slots, the integer class first; ar is integral_constant<int, AR_PM | AR_INT> or <int, AR_FP>
template <typename F>
static void for_each_class(const NttTables &T, const ClassMasks &m, F &&f) {
    if (m.integer) with_int_arith(T, [&](auto ar) { f(ar, m.integer, (uint32_t)__builtin_popcountll(m.integer)); });
    if (m.fp) f(std::integral_constant<int, AR_FP>{}, m.fp, (uint32_t)__builtin_popcountll(m.fp));
}

// workgroups along a pass of the radix-2^LOG_H kernels: one takes 256 >> LOG_H columns (rows)
template <int LOG_H>
static uint32_t col_tiles(const NttTables &T) { return (1u << T.log_r2) / (256u >> LOG_H); }
template <int LOG_H>
static uint32_t row_tiles(const NttTables &T) { return (1u << T.log_r1) / (256u >> LOG_H); }

template <bool INV>
static void launch_col(const NttIo &io0, const NttTables &T, uint32_t n_polys, const u64 *scale, const u64 *scale_sh,
                       hipStream_t s, int pack = 0, unsigned long long skip = 0) {  // skip: slots another kernel transforms
    const uint32_t r1 = 1u << T.log_r1, r2 = 1u << T.log_r2;
    const bool radix = dispatch<2, 3, 4>(fast_log_h(T.log_r1, r2), [&](auto log_h) {
        constexpr int LOG_H = decltype(log_h)::value;
        ClassMasks m = slot_classes(io0, T);
        m.integer &= ~skip;
        m.fp &= ~skip;
        for_each_class(T, m, [&](auto ar, unsigned long long mask, uint32_t nsel) {
            NttIo io = io0;
            io.slot_mask = mask;
            io.nsel = nsel;
            k_ntt_col_r<LOG_H, INV, decltype(ar)::value>
                <<<dim3(col_tiles<LOG_H>(T), n_polys * nsel), NTT_THREADS, 0, s>>>(io, T, scale, scale_sh, pack);
        });
    });
    if (radix) return;
    if (pack || skip) throw std::logic_error("packed output needs the radix column kernel");
    k_ntt_col<INV><<<dim3(r2 / NTT_COLS, n_polys * io0.nslots), NTT_THREADS, (size_t)r1 * NTT_COLS * sizeof(u64), s>>>(
        io0, T, scale, scale_sh);
}

static bool row_tail_supported(const NttTables &T) { return fast_row(T.log_r2, 1u << T.log_r1) != 0; }

template <bool INV>
static void launch_row(const NttIo &io0, const NttTables &T, uint32_t n_polys, const TailArgs &tail, hipStream_t s,
                       unsigned classes = 3) {  // bit 0: integer limbs, bit 1: fp64 limbs
    const uint32_t n = 1u << T.log_n, r1 = 1u << T.log_r1;
    const bool radix = dispatch<2, 3, 4, 9>(fast_row(T.log_r2, r1), [&](auto row_h) {
        constexpr int ROW_H = decltype(row_h)::value;
        for_each_class(T, slot_classes(io0, T, classes), [&](auto ar, unsigned long long mask, uint32_t nsel) {
            NttIo io = io0;
            io.slot_mask = mask;
            io.nsel = nsel;
            if constexpr (ROW_H == 9)
                k_ntt_row3<INV, decltype(ar)::value><<<dim3((r1 / 4) * n_polys * nsel), NTT_THREADS, 0, s>>>(io, T, tail);
            else
                k_ntt_row_r<ROW_H, INV, decltype(ar)::value>
                    <<<dim3(row_tiles<ROW_H>(T) * n_polys * nsel), NTT_THREADS, 0, s>>>(io, T, tail);
        });
    });
    if (radix) return;
    if (tail.enabled) throw std::logic_error("fused tail needs the radix row kernel");
    const uint32_t tile = n < (uint32_t)NTT_TILE ? n : (uint32_t)NTT_TILE;
    k_ntt_row<INV><<<dim3(n / tile, n_polys * io0.nslots), NTT_THREADS, (size_t)tile * sizeof(u64), s>>>(io0, T);
}

// two-pass launcher: reads `io.in`, leaves the result in `io.out` (may be the same buffer)
static void ntt_passes(NttIo io, const NttTables &T, uint32_t n_polys, bool inverse, const u64 *scale,
                       const u64 *scale_sh, hipStream_t s, int pack = 0, unsigned long long icol_skip = 0) {
    if (n_polys == 0 || io.nslots == 0) return;
    NttIo second = io;  // second pass runs in place on the output
    second.in_group = 0;
    second.in = io.out;
    second.in_stride = io.out_stride;
    second.in_slot0 = io.out_slot0;
    const TailArgs none{};
    if (!inverse) {
        launch_col<false>(io, T, n_polys, nullptr, nullptr, s);
        launch_row<false>(second, T, n_polys, none, s);
    } else {
        launch_row<true>(io, T, n_polys, none, s);
        launch_col<true>(second, T, n_polys, scale, scale_sh, s, pack, icol_skip);
    }
    MK_HIP(hipGetLastError());
}

// base conversion fused into the forward column pass of every converted limb (k_conv_col); false when the
// column pass of this ring size has no radix kernel (the caller then runs k_baseconv + a plain column pass)
template <int LOG_H, int N_IN, int SRCMODE>
static void launch_conv_col_n(const ConvIo &io0, const NttTables &T, const DevConv &cv, hipStream_t s, unsigned classes,
                              unsigned long long done) {
    ClassMasks m = target_classes(cv, T, classes);
    m.integer &= ~done;
    m.fp &= ~done;
    for_each_class(T, m, [&](auto ar, unsigned long long mask, uint32_t nsel) {
        ConvIo io = io0;
        io.target_mask = mask;
        io.nsel = nsel;
        if constexpr (LOG_H >= 3)
            // two targets of a class per workgroup (k_conv_col2): half the source traffic through each CU's L1; the last
            // workgroup of an odd target count carries one
            k_conv_col2<LOG_H, N_IN, decltype(ar)::value, DevConv, SRCMODE>
                <<<dim3(io.items * col_tiles<LOG_H>(T) * ((nsel + 1) / 2)), NTT_THREADS, 0, s>>>(io, T, cv);
        else
            k_conv_col<LOG_H, N_IN, decltype(ar)::value, DevConv, SRCMODE>
                <<<dim3(io.items * col_tiles<LOG_H>(T) * nsel), NTT_THREADS, 0, s>>>(io, T, cv);
    });
}
template <int LOG_H, int N_IN>
static void launch_conv_col_m(const ConvIo &io, const NttTables &T, const DevConv &cv, hipStream_t s, int srcmode,
                              unsigned classes, unsigned long long done) {
    if constexpr (N_IN <= 4 && LOG_H >= 3) {
        if (srcmode == 1) return launch_conv_col_n<LOG_H, N_IN, 1>(io, T, cv, s, classes, done);
        if (srcmode == 2) return launch_conv_col_n<LOG_H, N_IN, (N_IN > 1 ? 2 : 0)>(io, T, cv, s, classes, done);
    }
    if (srcmode != 0) throw std::logic_error("double conversion sources: unsupported shape");
    launch_conv_col_n<LOG_H, N_IN, 0>(io, T, cv, s, classes, done);
}
// srcmode: form of the sources in io.in (see src_is_double): 0 = packed 30-bit halves, 1 / 2 = doubles
// classes: bit 0 integer-class targets, bit 1 fp64-class targets; done: targets (indices into cv.dst_*) already written
static bool launch_conv_col(const ConvIo &io, const NttTables &T, const DevConv &cv, hipStream_t s, int srcmode = 0,
                            unsigned classes = 3, unsigned long long done = 0) {
    const bool radix = dispatch<2, 3, 4>(fast_log_h(T.log_r1, 1u << T.log_r2), [&](auto log_h) {
        if (!dispatch<1, 2, 3, 4, 5, 6, 7, 8>(cv.n_in, [&](auto n_in) {
                launch_conv_col_m<decltype(log_h)::value, decltype(n_in)::value>(io, T, cv, s, srcmode, classes, done);
            }))
            throw std::invalid_argument("base conversion fan-in unsupported");
    });
    if (radix) MK_HIP(hipGetLastError());
    return radix;
}
// the inverse column pass of every fp64-class limb of c1 in one launch, digit by digit, with up to `nt_max` fp64-class
// targets of a digit converted on the way (k_icol_conv; io.job[])
static void launch_icol_conv(const IcolConvIo &io, const NttTables &T, uint32_t nt_max, const u64 *scale, const u64 *scale_sh,
                             hipStream_t s) {
    if (!dispatch<3, 4>(fast_log_h(T.log_r1, 1u << T.log_r2), [&](auto log_h) {
            constexpr int LOG_H = decltype(log_h)::value;
            if (!dispatch<1, 2, 3>(nt_max, [&](auto nt_c) {
                    k_icol_conv<LOG_H, decltype(nt_c)::value>
                        <<<dim3(io.njobs * io.items * col_tiles<LOG_H>(T)), NTT_THREADS, 0, s>>>(io, T, scale, scale_sh);
                }))
                throw std::logic_error("k_icol_conv takes 1 to 3 targets");
        }))
        throw std::logic_error("k_icol_conv needs 64- or 256-point columns");
    MK_HIP(hipGetLastError());
}
// the group's ONE ModDown conversion (k_conv_col_psum), one instance per arithmetic class of the targets
template <int LOG_H, int N_IN>
static void launch_conv_col_psum_n(const ConvIo &io0, const NttTables &T, const DevConv &cv, hipStream_t s) {
    for_each_class(T, target_classes(cv, T), [&](auto ar, unsigned long long mask, uint32_t nsel) {
        ConvIo io = io0;
        io.target_mask = mask;
        io.nsel = nsel;
        if constexpr (decltype(ar)::value == AR_FP)
            // fp64-class targets two per workgroup (+0.2 % on the step at C3, +0.9 % at N = 2^17, L = 20)
            k_conv_col_psum2<LOG_H, N_IN, DevConv>
                <<<dim3(io.items * col_tiles<LOG_H>(T) * ((nsel + 1) / 2)), NTT_THREADS, 0, s>>>(io, T, cv);
        else
            k_conv_col_psum<LOG_H, N_IN, decltype(ar)::value, DevConv>
                <<<dim3(io.items * col_tiles<LOG_H>(T) * nsel), NTT_THREADS, 0, s>>>(io, T, cv);
    });
}
static void launch_conv_col_psum(const ConvIo &io, const NttTables &T, const DevConv &cv, hipStream_t s) {
    if (!dispatch<3, 4>(fast_log_h(T.log_r1, 1u << T.log_r2), [&](auto log_h) {
            if (!dispatch<1, 2, 3, 4, 5, 6, 7, 8>(cv.n_in, [&](auto n_in) {
                    launch_conv_col_psum_n<decltype(log_h)::value, decltype(n_in)::value>(io, T, cv, s);
                }))
                throw std::invalid_argument("base conversion fan-in unsupported");
        }))
        throw std::logic_error("summed conversion needs 64- or 256-point columns");
    MK_HIP(hipGetLastError());
}
// inverse column pass of the P limbs of every client of a group, summed over the clients as integers (k_icol_sum)
static void launch_icol_sum(const u64 *pc, u64 *psum, const NttTables &T, uint32_t K, uint32_t n_polys, uint32_t n_clients,
                            size_t in_cstride, hipStream_t s) {
    if (!dispatch<3, 4>(fast_log_h(T.log_r1, 1u << T.log_r2), [&](auto log_h) {
            constexpr int LOG_H = decltype(log_h)::value;
            with_int_arith(T, [&](auto ar) {
                k_icol_sum<LOG_H, decltype(ar)::value><<<dim3(col_tiles<LOG_H>(T), n_polys * K), NTT_THREADS, 0, s>>>(
                    pc, psum, T, K, n_clients, in_cstride);
            });
        }))
        throw std::logic_error("summed conversion needs 64- or 256-point columns");
    MK_HIP(hipGetLastError());
}

void Engine::ntt_launch(u64 *d, uint32_t n_polys, uint32_t nl, uint32_t ext, bool inverse, const u64 *scale,
                        const u64 *scale_sh) {
    NttIo io{d, d, (size_t)ext * ps_.n, (size_t)ext * ps_.n, 0, 0, 0, ext, nl};
    ntt_passes(io, tabs_, n_polys, inverse, scale, scale_sh, stream_);
}

void Engine::ntt_forward(u64 *d, uint32_t n_polys, uint32_t nl, bool with_p) {
    need_device();
    if (nl > ps_.L || (nl == 0 && !with_p)) throw std::invalid_argument("nl out of range");
    ntt_launch(d, n_polys, nl, nl + (with_p ? ps_.K : 0), false, nullptr, nullptr);
}
void Engine::ntt_inverse(u64 *d, uint32_t n_polys, uint32_t nl, bool with_p) {
    need_device();
    if (nl > ps_.L || (nl == 0 && !with_p)) throw std::invalid_argument("nl out of range");
    ntt_launch(d, n_polys, nl, nl + (with_p ? ps_.K : 0), true, nullptr, nullptr);
}

// ---- aggregation --------------------------------------------------------------------

void Engine::eval_add(const u64 *a, const u64 *b, u64 *out, uint32_t n_ct, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!n_ct) return;
    EwGeom g{ps_.n, nl, ps_.L};
    k_add<<<ew_grid(ps_.n, 2 * nl, n_ct), EW_THREADS, 0, stream_>>>(a, b, out, g, d_limb_, 2 * nl);
    MK_HIP(hipGetLastError());
}

void Engine::eval_sum(const u64 *in, u64 *out, uint32_t n_clients, uint32_t n_ct, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!n_ct || !n_clients) return;
    EwGeom g{ps_.n, nl, ps_.L};
    k_sum<<<ew_grid(ps_.n, 2 * nl, n_ct), EW_THREADS, 0, stream_>>>(in, out, g, d_limb_, 2 * nl, n_clients,
                                                                 (size_t)n_ct * 2 * nl * ps_.n);
    MK_HIP(hipGetLastError());
}

void Engine::reduce_mod(u64 *ct, uint32_t n_ct, uint32_t nl, uint32_t n_terms) {
    need_device();
    check_nl(nl);
    if (n_terms > 8) throw std::invalid_argument("integer-sum collective supports at most 8 terms (q < 2^61)");
    if (!n_ct) return;
    EwGeom g{ps_.n, nl, ps_.L};
    k_reduce<<<ew_grid(ps_.n, 2 * nl, n_ct), EW_THREADS, 0, stream_>>>(ct, g, d_limb_, 2 * nl);
    MK_HIP(hipGetLastError());
}

void Engine::reduce_scatter_sum_mod(void *comm, const u64 *partial, u64 *shard, uint32_t n_ct_shard, uint32_t nl,
                                    uint32_t n_ranks) {
    need_device();
    check_nl(nl);
    if (n_ranks < 1 || n_ranks > 8) throw std::invalid_argument("integer-sum collective supports 1..8 ranks (q < 2^61)");
    if (!n_ct_shard) return;
    comm_reduce_scatter_u64(comm, partial, shard, (size_t)n_ct_shard * 2 * nl * ps_.n, stream_);
    reduce_mod(shard, n_ct_shard, nl, n_ranks);
}

void Engine::mult_const(u64 *ct, uint32_t n_ct, uint32_t nl, const std::vector<u64> &factors) {
    need_device();
    check_nl(nl);
    if (!n_ct) return;
    std::vector<u64> both(factors);
    for (uint32_t i = 0; i < nl; ++i) both.push_back(h_shoup(factors[i], ps_.moduli[i]));
    u64 *d_f = workspace(2 * nl);
    MK_HIP(hipMemcpyAsync(d_f, both.data(), both.size() * sizeof(u64), hipMemcpyHostToDevice, stream_));
    MK_HIP(hipStreamSynchronize(stream_));  // `both` is a stack-local staging buffer
    EwGeom g{ps_.n, nl, ps_.L};
    k_mul_const<<<ew_grid(ps_.n, 2 * nl, n_ct), EW_THREADS, 0, stream_>>>(ct, g, d_limb_, 2 * nl, d_f, d_f + nl);
    MK_HIP(hipGetLastError());
}

template <int LOG_H>
static void launch_switch_col(const u64 *last, u64 *out, const NttTables &T, uint32_t n_targets, uint32_t items, u64 q_last,
                              hipStream_t s) {
    for_each_class(T, limb_classes(n_targets, T), [&](auto ar, unsigned long long mask, uint32_t nsel) {
        k_switch_col<LOG_H, decltype(ar)::value>
            <<<dim3(col_tiles<LOG_H>(T), nsel, items), NTT_THREADS, 0, s>>>(last, out, T, n_targets, q_last, mask);
    });
}

const u64 *Engine::rescale_consts(uint32_t nl, const std::vector<u64> *factors) {
    // constants c_i = q_last^-1 (* EvalMult constant) mod q_i, cached on the device per (level, constant): no host
    // synchronisation inside a server step
    const uint32_t last = nl - 1;
    std::string key = "resc_" + std::to_string(nl);
    if (factors)
        for (uint32_t i = 0; i < last; ++i) key += "_" + std::to_string((*factors)[i]);
    auto it = vec_cache_.find(key);
    if (it != vec_cache_.end()) return it->second;
    std::vector<u64> c(2 * last);
    for (uint32_t i = 0; i < last; ++i) {
        u64 v = ps_.q_inv_mod(last, i);
        if (factors) v = h_mulmod(v, (*factors)[i], ps_.moduli[i]);
        c[i] = v;
        c[last + i] = h_shoup(v, ps_.moduli[i]);
    }
    if (vec_cache_.size() > 4096) throw std::runtime_error("too many distinct rescale constants cached");
    return limb_vector(key, c);
}

void Engine::rescale_core(const u64 *in, uint32_t in_limbs, u64 *out, uint32_t items, uint32_t nl, const u64 *d_c, u64 *d_last,
                          u64 *d_tmp, uint32_t group, size_t out_gstride) {
    const uint32_t n = ps_.n, last = nl - 1;
    // 1. dropped limb -> COEFFICIENT format
    NttIo io{in, d_last, (size_t)in_limbs * n, (size_t)n, last, 0, last, 1, nl};
    ntt_passes(io, tabs_, items, true, nullptr, nullptr, stream_);
    const int col_h = fast_log_h(tabs_.log_r1, 1u << tabs_.log_r2);
    if (col_h >= 2 && row_tail_supported(tabs_)) {
        // 2. centred switch of modulus fused into the forward column pass of every remaining limb; 3. row pass with
        // 4. (c_i - tmp_i) * q_last^-1 [* constant] in its copy-out (the ModDown tail with til = the input ciphertext)
        if (!dispatch<2, 3, 4>(col_h, [&](auto log_h) {
                launch_switch_col<decltype(log_h)::value>(d_last, d_tmp, tabs_, last, items, ps_.moduli[last], stream_);
            }))
            throw std::logic_error("fused rescale: no switch kernel for this column radix");
        MK_HIP(hipGetLastError());
        NttIo row{d_tmp, out, (size_t)last * n, (size_t)last * n, 0, 0, 0, last, last};
        TailArgs tail{in, nullptr, d_c, d_c + last, 0, in_limbs, 1, 0u, group, out_gstride};
        launch_row<false>(row, tabs_, items, tail, stream_);
        MK_HIP(hipGetLastError());
        return;
    }
    // ring sizes without the radix kernels: the four steps as separate kernels
    EwGeom g{n, nl, ps_.L};
    k_switch_modulus<<<ew_grid(n, last, items), EW_THREADS, 0, stream_>>>(d_last, d_tmp, g, d_limb_, ps_.moduli[last]);
    MK_HIP(hipGetLastError());
    ntt_launch(d_tmp, items, last, last, false, nullptr, nullptr);
    k_sub_mul<<<ew_grid(n, last, items), EW_THREADS, 0, stream_>>>(in, in_limbs, d_tmp, out, g, d_limb_, d_c, d_c + last, group,
                                                                out_gstride);
    MK_HIP(hipGetLastError());
}

void Engine::rescale(const u64 *in, u64 *out, uint32_t n_ct, uint32_t nl, const std::vector<u64> *factors) {
    need_device();
    check_nl(nl);
    if (nl < 2) throw std::invalid_argument("rescale needs at least 2 limbs");
    if (!n_ct) return;
    const uint32_t n = ps_.n, last = nl - 1, items = 2 * n_ct;
    const u64 *d_c = rescale_consts(nl, factors);
    const size_t w_last = (size_t)items * n, w_tmp = (size_t)items * last * n;
    u64 *ws = workspace(w_last + w_tmp);
    rescale_core(in, nl, out, items, nl, d_c, ws, ws + w_last, 0, 0);
}

static bool ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
    const uintptr_t a_lo = (uintptr_t)a, b_lo = (uintptr_t)b;
    return a_lo < b_lo + b_bytes && b_lo < a_lo + a_bytes;
}

// Rescale(prefix(in, nl_out + 1)): the rescale launches on the first nl_out + 1 limbs of ciphertexts nl_in limbs wide,
// read where they are (a polynomial of the prefix is a polynomial of the input at stride nl_in)
void Engine::compress(const u64 *in, u64 *out, uint32_t n_ct, uint32_t nl_in, uint32_t nl_out) {
    need_device();
    check_nl(nl_in);
    if (nl_out < 1 || nl_out >= nl_in) throw std::invalid_argument("compress needs 1 <= nl_out < nl_in");
    if (!n_ct) return;
    const uint32_t n = ps_.n, nl = nl_out + 1, items = 2 * n_ct;
    if (ranges_overlap(in, (size_t)items * nl_in * n * sizeof(u64), out, (size_t)items * nl_out * n * sizeof(u64)))
        throw std::invalid_argument("compress cannot write over its input");
    const u64 *d_c = rescale_consts(nl, nullptr);
    const size_t w_last = (size_t)items * n, w_tmp = (size_t)items * nl_out * n;
    u64 *ws = workspace(w_last + w_tmp);
    rescale_core(in, nl_in, out, items, nl, d_c, ws, ws + w_last, 0, 0);
}

// ---- EvalMult(ct, plaintext): per-slot aggregation weights ------------------------------

static void check_plain_counts(uint32_t n_ct, uint32_t n_pt) {
    if (n_pt != 1 && n_pt != n_ct) throw std::invalid_argument("n_pt must be 1 or n_ct");
}

void Engine::mult_plain(u64 *ct, const u64 *pt, uint32_t n_ct, uint32_t n_pt, uint32_t nl) {
    need_device();
    check_nl(nl);
    check_plain_counts(n_ct, n_pt);
    if (!n_ct) return;
    EwGeom g{ps_.n, nl, ps_.L};
    k_mul_plain<<<ew_grid(ps_.n, 2 * nl, n_ct), EW_THREADS, 0, stream_>>>(ct, pt, ct, g, d_limb_, 2 * nl, n_pt);
    MK_HIP(hipGetLastError());
}

// the two row kernels of the fused form, in the arithmetic class of their limbs
static void launch_ptmul_irow(const PtmulArgs &a, const NttTables &T, uint32_t polys, hipStream_t s) {
    const uint32_t r1 = 1u << T.log_r1;
    ClassMasks m;  // the dropped limb alone
    (T.h_fp_of[a.nl - 1] ? m.fp : m.integer) = 1ull;
    if (!dispatch<2, 3, 4, 9>(fast_row(T.log_r2, r1), [&](auto row_h) {
            constexpr int ROW_H = decltype(row_h)::value;
            for_each_class(T, m, [&](auto ar, unsigned long long, uint32_t) {
                if constexpr (ROW_H == 9)
                    k_ptmul_irow3<decltype(ar)::value><<<dim3((r1 / 4) * polys), NTT_THREADS, 0, s>>>(a, T);
                else
                    k_ptmul_irow<ROW_H, decltype(ar)::value><<<dim3(row_tiles<ROW_H>(T) * polys), NTT_THREADS, 0, s>>>(a, T);
            });
        }))
        throw std::logic_error("fused plaintext product: no row kernel for this row length");
}
static void launch_ptresc_row(const PtmulArgs &a0, const NttTables &T, uint32_t polys, hipStream_t s) {
    const uint32_t r1 = 1u << T.log_r1;
    if (!dispatch<2, 3, 4, 9>(fast_row(T.log_r2, r1), [&](auto row_h) {
            constexpr int ROW_H = decltype(row_h)::value;
            for_each_class(T, limb_classes(a0.nl - 1, T), [&](auto ar, unsigned long long mask, uint32_t nsel) {
                PtmulArgs a = a0;
                a.slot_mask = mask;
                a.nsel = nsel;
                if constexpr (ROW_H == 9)
                    k_ptresc_row3<decltype(ar)::value><<<dim3((r1 / 4) * polys * nsel), NTT_THREADS, 0, s>>>(a, T);
                else
                    k_ptresc_row<ROW_H, decltype(ar)::value>
                        <<<dim3(row_tiles<ROW_H>(T) * polys * nsel), NTT_THREADS, 0, s>>>(a, T);
            });
        }))
        throw std::logic_error("fused plaintext product: no row kernel for this row length");
}

// DropLastElementAndScale(in * pt).  Fused (the ring sizes whose plain rescale is fused): the product of the dropped limb
// inside its inverse row pass, the products of the remaining limbs inside the forward row pass of the switched limb;
// otherwise, and under MKCKKS_PLAIN_FUSED=0, the composition k_mul_plain into a workspace + rescale_core, chunk by chunk.
void Engine::mult_plain_rescale(const u64 *in, const u64 *pt, u64 *out, uint32_t n_ct, uint32_t n_pt, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (nl < 2) throw std::invalid_argument("rescale needs at least 2 limbs");
    check_plain_counts(n_ct, n_pt);
    if (!n_ct) return;
    const uint32_t n = ps_.n, last = nl - 1;
    if (ranges_overlap(in, (size_t)n_ct * 2 * nl * n * sizeof(u64), out, (size_t)n_ct * 2 * last * n * sizeof(u64)))
        throw std::invalid_argument("mult_plain_rescale cannot write over its input");
    const u64 *d_c = rescale_consts(nl, nullptr);
    const int col_h = fast_log_h(tabs_.log_r1, 1u << tabs_.log_r2);
    const bool fused = col_h >= 2 && row_tail_supported(tabs_) && knobs_.plain_fused != 0;
    if (fused) {
        const uint32_t items = 2 * n_ct;
        const size_t w_last = (size_t)items * n;
        u64 *d_last = workspace(w_last + (size_t)items * last * n), *d_tmp = d_last + w_last;
        PtmulArgs a{in, pt, d_tmp, d_last, d_c, d_c + last, nl, n_pt == 1 ? 1u : 0u, 0, 0};
        launch_ptmul_irow(a, tabs_, items, stream_);
        NttIo col{d_last, d_last, (size_t)n, (size_t)n, 0, 0, last, 1, nl};
        launch_col<true>(col, tabs_, items, nullptr, nullptr, stream_);
        if (!dispatch<2, 3, 4>(col_h, [&](auto log_h) {
                launch_switch_col<decltype(log_h)::value>(d_last, d_tmp, tabs_, last, items, ps_.moduli[last], stream_);
            }))
            throw std::logic_error("fused rescale: no switch kernel for this column radix");
        a.out = out;
        launch_ptresc_row(a, tabs_, items, stream_);
        MK_HIP(hipGetLastError());
        return;
    }
    const uint32_t chunk = n_ct < knobs_.chunk ? n_ct : knobs_.chunk;
    const size_t w_prod = (size_t)chunk * 2 * nl * n, w_last = (size_t)chunk * 2 * n;
    u64 *prod = workspace(w_prod + w_last + (size_t)chunk * 2 * last * n);
    EwGeom g{n, nl, ps_.L};
    for (uint32_t b0 = 0; b0 < n_ct; b0 += chunk) {
        const uint32_t cnt = n_ct - b0 < chunk ? n_ct - b0 : chunk;
        const u64 *ptb = n_pt == 1 ? pt : pt + (size_t)b0 * nl * n;
        k_mul_plain<<<ew_grid(n, 2 * nl, cnt), EW_THREADS, 0, stream_>>>(in + (size_t)b0 * 2 * nl * n, ptb, prod, g, d_limb_, 2 * nl,
                                                                        n_pt == 1 ? 1u : cnt);
        MK_HIP(hipGetLastError());
        rescale_core(prod, nl, out + (size_t)b0 * 2 * last * n, 2 * cnt, nl, d_c, prod + w_prod, prod + w_prod + w_last, 0, 0);
    }
}

// ---- hybrid key switching -----------------------------------------------------------

// N^-1 * [(Q_j/q_i)^-1]_{q_i} per Q limb (its digit at this level) and N^-1 * [(P/p_k)^-1]_{p_k} per P limb:
// the inverse transforms ahead of ModUp / ModDown scale by these, so the conversions take their inputs as is.
const u64 *Engine::folded_scale(uint32_t nl) {
    const std::string key = "fold_" + std::to_string(nl);
    auto it = vec_cache_.find(key);
    if (it != vec_cache_.end()) return it->second;
    const uint32_t D = ps_.D;
    std::vector<u64> v(2 * D, 0);
    auto put = [&](uint32_t id, u64 hatinv) {
        const u64 q = ps_.moduli[id];
        const u64 c = h_mulmod(ps_.limb[id].ninv, hatinv, q);
        if (ps_.limb[id].fp) {  // the inverse column pass of an fp limb scales with (double c, double c/q)
            const double cd = (double)c, cq = (double)((long double)c / (long double)q);
            std::memcpy(&v[id], &cd, 8);
            std::memcpy(&v[D + id], &cq, 8);
        } else {
            v[id] = c;
            v[D + id] = h_shoup(c, q);
        }
    };
    for (uint32_t part = 0; part < ps_.num_parts(nl); ++part) {
        BaseConvTable t = ps_.modup_table(nl, part);
        for (size_t i = 0; i < t.src.size(); ++i) put(t.src[i], t.hatinv[i]);
    }
    BaseConvTable t = ps_.moddown_table(nl);
    for (size_t i = 0; i < t.src.size(); ++i) put(t.src[i], t.hatinv[i]);
    return limb_vector(key, v);
}

const u64 *Engine::p_inverse(uint32_t nl) {
    const std::string key = "pinv_" + std::to_string(nl);
    auto it = vec_cache_.find(key);
    if (it != vec_cache_.end()) return it->second;
    std::vector<u64> pinv(2 * nl);
    for (uint32_t i = 0; i < nl; ++i) {
        pinv[i] = ps_.p_inv_mod(i);
        pinv[nl + i] = h_shoup(pinv[i], ps_.moduli[i]);
    }
    return limb_vector(key, pinv);
}

// EvalKeySwitchPrecomputeCore on `cnt` polynomials c1 (items ct_stride apart): fills the converted limbs of
// dig[item][part][ext][N] in EVALUATION format; the digits' own limbs are NOT copied (readers take them from c1).
// p_scaled (the merged n-client flow only): convert with the P-scaled tables, so the P limbs of the digits hold
// N^-1 [(P/p_k)^-1]_{p_k} d_j and the flow's inverse transform of the P limbs does not scale (k_icol_sum).
void Engine::modup_core(const u64 *c1, size_t c1_stride, u64 *coef, u64 *dig, uint32_t cnt, uint32_t nl,
                        bool rows_int_only, uint32_t in_group, size_t in_gstride, bool p_scaled) {
    const uint32_t n = ps_.n, ext = nl + ps_.K, nparts = ps_.num_parts(nl), D = ps_.D;
    const u64 *fold = folded_scale(nl);
    // the fused conversion kernel exists when the column pass has a radix kernel; it reads packed 30-bit halves
    bool fused = fast_log_h(tabs_.log_r1, 1u << tabs_.log_r2) != 0;
    // S1: c1 -> COEFFICIENT format, scaled by N^-1 * Qhat_inv
    NttIo s1{c1, coef, c1_stride, (size_t)nl * n, 0, 0, 0, nl, nl};
    s1.in_group = in_group;  // n-client flow: polynomial p is c1 of cts[p / in_group][p % in_group]
    s1.in_gstride = in_gstride;
    const size_t dstride = (size_t)nparts * ext * n;
    // interchange format of the coefficient-form digits: fp64-class limbs as canonical doubles when every digit is
    // "all fp64-class" or "q_0 first, then fp64-class" (k_conv_col's SRCMODE 1 / 2), else packed halves throughout
    bool doubles = fused && tabs_.has_fp && fast_log_h(tabs_.log_r1, 1u << tabs_.log_r2) >= 3;
    for (uint32_t part = 0; part < nparts && doubles; ++part) {
        const DevConv &cv = modup_conv(nl, part, p_scaled);
        if (conv_src_mode(cv) < 0 || (conv_src_mode(cv) != 0 && cv.n_in > 4)) doubles = false;
    }
    // digits whose sources are all fp64-class: their inverse column pass converts some of their fp64-class targets on the
    // way (how many: icol_conv_targets).  Where a digit takes part, ONE launch of k_icol_conv runs the inverse column pass
    // of every fp64-class limb (a job per digit, the longest first) and the fp64 instance of the plain pass is not launched
    std::vector<unsigned long long> icol_done(nparts, 0);  // per digit: the targets k_icol_conv writes
    IcolConvIo icol{coef, dig, (size_t)nl * n, dstride, cnt, 0, {}};
    uint32_t icol_nt_max = 0;
    unsigned long long icol_slots = 0;
    if (doubles && knobs_.icol_conv != 0 && nparts <= (uint32_t)ICOL_MAX_JOBS) {
        std::vector<unsigned long long> fp_targets(nparts, 0);
        uint32_t eligible = 0;
        for (uint32_t part = 0; part < nparts; ++part) {
            const DevConv &cv = modup_conv(nl, part, p_scaled);
            if (conv_src_mode(cv) != 1) continue;
            fp_targets[part] = target_classes(cv, tabs_, 2).fp;
            eligible += fp_targets[part] != 0;
        }
        const uint64_t grid = (uint64_t)cnt * eligible * ((1u << tabs_.log_r2) / (256u >> (tabs_.log_r1 / 2)));
        std::vector<IcolJob> jobs;
        for (uint32_t part = 0; part < nparts; ++part) {
            const DevConv &cv = modup_conv(nl, part, p_scaled);
            IcolJob jb{};
            uint32_t first_fp = 0;  // index in cv of the job's first source: its rows of the constant tables start there
            for (uint32_t i = 0; i < cv.n_in; ++i)
                if (fp_of_[cv.src_id[i]]) {
                    if (!jb.n_in) first_fp = i;
                    jb.src_id[jb.n_in] = cv.src_id[i];
                    jb.src_slot[jb.n_in++] = cv.src_slot[i];
                    icol_slots |= 1ull << cv.src_slot[i];
                }
            if (!jb.n_in) continue;
            unsigned long long m = fp_targets[part];
            uint32_t nt = icol_conv_targets((uint32_t)__builtin_popcountll(m), grid, knobs_.icol_conv);
            for (; nt; --nt, m &= m - 1) icol_done[part] |= m & (~m + 1);  // the first nt of them
            for (unsigned long long d = icol_done[part]; d; d &= d - 1) {
                const uint32_t t = (uint32_t)__builtin_ctzll(d);
                jb.dst_id[jb.nt] = cv.dst_id[t];
                jb.dst_slot[jb.nt] = cv.dst_slot[t];
                jb.hat_d[jb.nt] = cv.hat_d + t;
                jb.hatq_d[jb.nt++] = cv.hatq_d + t;
            }
            for (uint32_t t = jb.nt; t < 3; ++t) {  // the kernel loads every target's constants: valid ones, sums dropped
                jb.dst_id[t] = jb.src_id[0];
                jb.hat_d[t] = cv.hat_d + (size_t)first_fp * cv.n_out;
                jb.hatq_d[t] = cv.hatq_d + (size_t)first_fp * cv.n_out;
            }
            jb.hat_stride = cv.n_out;
            jb.dig_off = (size_t)part * ext * n;
            icol_nt_max = std::max(icol_nt_max, jb.nt);
            jobs.push_back(jb);
        }
        if (icol_nt_max) {
            std::stable_sort(jobs.begin(), jobs.end(),
                             [](const IcolJob &a, const IcolJob &b) { return a.n_in + a.nt > b.n_in + b.nt; });
            for (const IcolJob &jb : jobs) icol.job[icol.njobs++] = jb;
        } else {
            icol_slots = 0;
        }
    }
    ntt_passes(s1, tabs_, cnt, true, fold, fold + D, stream_, fused ? (doubles ? 2 : 1) : 0, icol_slots);
    if (icol_slots) launch_icol_conv(icol, tabs_, icol_nt_max, fold, fold + D, stream_);
    for (uint32_t part = 0; part < nparts && fused; ++part) {
        // S2+S3a: base conversion fused into the column pass of each complement limb
        ConvIo io{coef, dig + (size_t)part * ext * n, (size_t)nl * n, dstride, cnt, 0, 0};
        const DevConv &cv = modup_conv(nl, part, p_scaled);
        launch_conv_col(io, tabs_, cv, stream_, doubles ? conv_src_mode(cv) : 0, 3, icol_done[part]);
    }
    if (fused) {
        // S3b: one row pass over every converted limb of every digit (own limbs skipped)
        NttIo row{dig, dig, (size_t)ext * n, (size_t)ext * n, 0, 0, 0, ext, nl, nparts, ps_.alpha};
        // (rows_int_only: the fp64 limbs finish their transform inside the fused inner-product kernel)
        if (!skip_rows_) launch_row<false>(row, tabs_, cnt * nparts, TailArgs{}, stream_, rows_int_only ? 1u : 3u);
        MK_HIP(hipGetLastError());
        return;
    }
    if (rows_int_only || p_scaled) throw std::logic_error("fused inner product needs the radix kernels");
    for (uint32_t part = 0; part < nparts; ++part) {  // ring sizes without a radix column kernel
        const DevConv &cv = modup_conv(nl, part);
        const uint32_t lo = part * ps_.alpha, hi = lo + cv.n_in;
        u64 *d = dig + (size_t)part * ext * n;
        launch_baseconv(coef, (size_t)nl * n, d, dstride, cv, d_limb_, n, cnt, 1, stream_);
        if (lo > 0) {
            NttIo a{d, d, dstride, dstride, 0, 0, 0, lo, nl};
            ntt_passes(a, tabs_, cnt, false, nullptr, nullptr, stream_);
        }
        if (hi < ext) {
            NttIo b{d, d, dstride, dstride, hi, hi, hi, ext - hi, nl};
            ntt_passes(b, tabs_, cnt, false, nullptr, nullptr, stream_);
        }
    }
}

// first half of ApproxModDown on `cnt` polynomials: INTT of the P limbs of til (scaled by N^-1 * Phat^-1), conversion
// P -> Q_l, forward column pass of the converted limbs -> conv [cnt][nl][N] (the row pass + tail follow).  pc is the
// scratch of the P limbs between the passes; with rows_done the inverse ROW pass already happened inside the fused
// inner-product kernel and pc holds its output.
void Engine::moddown_convert(const u64 *til, u64 *pc, u64 *conv, uint32_t cnt, uint32_t nl, bool rows_done) {
    const uint32_t n = ps_.n, K = ps_.K, ext = nl + K, D = ps_.D;
    const u64 *fold = folded_scale(nl);
    NttIo s5{til, pc, (size_t)ext * n, (size_t)K * n, nl, 0, nl, K, nl};
    const DevConv &cv = moddown_conv(nl);
    if (!rows_done) {
        ntt_passes(s5, tabs_, cnt, true, fold, fold + D, stream_, 1);
    } else {
        NttIo second = s5;
        second.in = s5.out;
        second.in_stride = s5.out_stride;
        second.in_slot0 = s5.out_slot0;
        launch_col<true>(second, tabs_, cnt, fold, fold + D, stream_, 1);
        MK_HIP(hipGetLastError());
    }
    ConvIo io{pc, conv, (size_t)K * n, (size_t)nl * n, cnt, 0, 0};
    launch_conv_col(io, tabs_, cv, stream_);
}

// ApproxModDown on `cnt` polynomials til[item][ext][N] -> out[item] (items out_stride apart, nl limbs each);
// add (optional): ciphertext array whose c0 is added on even items (KeySwitchInPlace: c0 += ...).
void Engine::moddown_core(const u64 *til, u64 *pc, u64 *conv, u64 *out, size_t out_stride, const u64 *add,
                          size_t add_stride, uint32_t cnt, uint32_t nl, bool accumulate, bool p_rows_done, uint32_t group,
                          size_t out_gstride) {
    const uint32_t n = ps_.n, K = ps_.K, ext = nl + K, D = ps_.D;
    const u64 *fold = folded_scale(nl), *pinv = p_inverse(nl);
    const bool conv_fused = fast_log_h(tabs_.log_r1, 1u << tabs_.log_r2) != 0;  // conversion inside the column pass
    const bool tail_fused = conv_fused && row_tail_supported(tabs_);               // tail inside the row pass
    const DevConv &cv = moddown_conv(nl);
    EwGeom g{n, nl, ps_.L};
    if (tail_fused) {
        moddown_convert(til, pc, conv, cnt, nl, p_rows_done);
        // row pass of the converted limbs with the (ctilde_Q - conv) * P^-1 (+ c0) tail in its copy-out
        NttIo row{conv, out, (size_t)nl * n, out_stride, 0, 0, 0, nl, nl};
        TailArgs tail{til, add, pinv, pinv + nl, add_stride, ext, 1, accumulate ? 1u : 0u, group, out_gstride};
        launch_row<false>(row, tabs_, cnt, tail, stream_);
        MK_HIP(hipGetLastError());
        return;
    }
    if (group) throw std::logic_error("grouped ModDown needs the fused tail");
    if (conv_fused) {  // fused conversion + column pass, plain row pass, tail as its own kernel
        moddown_convert(til, pc, conv, cnt, nl, p_rows_done);
        NttIo row{conv, conv, (size_t)nl * n, (size_t)nl * n, 0, 0, 0, nl, nl};
        launch_row<false>(row, tabs_, cnt, TailArgs{}, stream_);
    } else {
        if (p_rows_done) throw std::logic_error("fused P-limb inverse needs the radix kernels");
        NttIo s5{til, pc, (size_t)ext * n, (size_t)K * n, nl, 0, nl, K, nl};
        ntt_passes(s5, tabs_, cnt, true, fold, fold + D, stream_, 0);
        launch_baseconv(pc, (size_t)K * n, conv, (size_t)nl * n, cv, d_limb_, n, cnt, 1, stream_);
        ntt_launch(conv, cnt, nl, nl, false, nullptr, nullptr);
    }
    k_moddown_tail<<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(til, conv, out, g, d_limb_, ext, pinv, pinv + nl,
                                                                 add, add_stride, out_stride, accumulate ? 1 : 0);
    MK_HIP(hipGetLastError());
}

void Engine::modup(const u64 *c1, u64 *digits, uint32_t cnt, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!cnt) return;
    const uint32_t n = ps_.n, ext = nl + ps_.K, nparts = ps_.num_parts(nl);
    u64 *coef = workspace((size_t)cnt * nl * n);
    modup_core(c1, (size_t)nl * n, coef, digits, cnt, nl);
    // the public digit layout carries the own limbs too (EvalKeySwitchPrecomputeCore's partsCtExt)
    const size_t dstride = (size_t)nparts * ext * n;
    for (uint32_t part = 0; part < nparts; ++part) {
        const uint32_t lo = part * ps_.alpha, hi = std::min(nl, lo + ps_.alpha);
        k_copy_slots<<<ew_grid(n, hi - lo, cnt), EW_THREADS, 0, stream_>>>(c1, (size_t)nl * n, lo,
                                                                         digits + (size_t)part * ext * n, dstride, lo, n);
    }
    MK_HIP(hipGetLastError());
}

void Engine::moddown(const u64 *in, u64 *out, uint32_t cnt, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!cnt) return;
    const uint32_t n = ps_.n, K = ps_.K;
    const size_t w_pc = (size_t)cnt * K * n, w_conv = (size_t)cnt * nl * n;
    u64 *ws = workspace(w_pc + w_conv);
    moddown_core(in, ws, ws + w_pc, out, (size_t)nl * n, nullptr, 0, cnt, nl, false);
}

template <int NPARTS>
static void launch_inner(const u64 *dig, const u64 *c1, size_t c1_stride, const u64 *evk, u64 *til, EwGeom g,
                         const LimbConst *limb, uint32_t ext, uint32_t D, uint32_t alpha, uint32_t items,
                         unsigned long long slot_mask, hipStream_t s) {
    const uint32_t nsel = (uint32_t)__builtin_popcountll(slot_mask);
    if (!nsel) return;
    k_inner_product_b<NPARTS><<<dim3((g.n / 2 + EW_THREADS - 1) / EW_THREADS, nsel), EW_THREADS, 0, s>>>(
        dig, c1, c1_stride, evk, til, g, limb, ext, D, alpha, items, slot_mask);
}

template <int LOG_H, int NPARTS>
static void launch_row_inner_fp(const InnerArgs &a, const NttTables &T, hipStream_t s) {
    const uint32_t tiles = (1u << T.log_r1) / (256u >> LOG_H);
    // 2 waves per SIMD: 196 VGPRs, no spills; measured 18.35 k ct/s against 17.9 k at 3 waves (168 VGPRs, 28 spilled)
    const dim3 grid(tiles * a.nsel * a.items);
    k_row_inner_fp<LOG_H, NPARTS, 2><<<grid, NTT_THREADS, 0, s>>>(a, T);
}
template <int LOG_H>
static void launch_row_inner_fp_n(const InnerArgs &a, const NttTables &T, uint32_t nparts, hipStream_t s) {
    if (!dispatch<1, 2, 3, 4, 5, 6>(nparts, [&](auto np) { launch_row_inner_fp<LOG_H, decltype(np)::value>(a, T, s); }))
        throw std::invalid_argument("more than 6 key-switch digits unsupported");
}

// 256-point rows have two implementations of the fused kernels: two rounds of radix 16 (16 words per thread, 2 waves
// per SIMD) and three rounds 8 x 8 x 4 (8 words per thread, 3 waves per SIMD); Knobs::row3x picks

template <int LOGC>
static void launch_row3_inner_fp_n(const InnerArgs &a, const NttTables &T, uint32_t nparts, hipStream_t s) {
    const dim3 grid(((1u << T.log_r1) / RowT<LOGC>::ROWS) * a.nsel * a.items);
    if (!dispatch<1, 2, 3, 4, 5, 6>(nparts, [&](auto np) {
            k_row3_inner_fp<decltype(np)::value, LOGC><<<grid, NTT_THREADS, 0, s>>>(a, T);
        }))
        throw std::invalid_argument("more than 6 key-switch digits unsupported");
}

template <int LOGC, bool INVP>
static void launch_row3_inner_int_k(const InnerArgs &a, const NttTables &T, uint32_t nparts, uint32_t L, u64 *pc,
                                    uint32_t K, hipStream_t s) {
    if (!a.nsel || !a.items) return;
    // a workgroup walks up to inner_walk_len(nparts) ciphertext indices of one client
    const dim3 grid(((1u << T.log_r1) / RowT<LOGC>::ROWS) * a.nsel * inner_walks(a, nparts));
    if (!dispatch<1, 2, 3, 4, 5, 6>(nparts, [&](auto np) {
            with_int_arith(T, [&](auto ar) {
                k_row3_inner_int<decltype(np)::value, LOGC, INVP, decltype(ar)::value>
                    <<<grid, NTT_THREADS, 0, s>>>(a, T, L, pc, K);
            });
        }))
        throw std::invalid_argument("more than 6 key-switch digits unsupported");
}
// integer slots of the extended basis: Q slots (q0) keep their accumulators in til; P slots continue into the inverse
// row pass when `pc` is given (its own kernel instance: different epilogue, different register budget)
template <int LOGC>
static void launch_row3_inner_int_n(const InnerArgs &a, const NttTables &T, uint32_t nparts, uint32_t L, u64 *pc,
                                    uint32_t K, hipStream_t s) {
    if (!pc) {
        launch_row3_inner_int_k<LOGC, false>(a, T, nparts, L, nullptr, K, s);
        return;
    }
    const unsigned long long q_slots = a.nl >= 64 ? ~0ull : ((1ull << a.nl) - 1);
    InnerArgs aq = a, ap = a;
    aq.slot_mask = a.slot_mask & q_slots;
    ap.slot_mask = a.slot_mask & ~q_slots;
    aq.nsel = (uint32_t)__builtin_popcountll(aq.slot_mask);
    ap.nsel = (uint32_t)__builtin_popcountll(ap.slot_mask);
    launch_row3_inner_int_k<LOGC, true>(ap, T, nparts, L, pc, K, s);
    launch_row3_inner_int_k<LOGC, false>(aq, T, nparts, L, nullptr, K, s);
}

// S1-S4 of the hybrid key switch for `cnt` ciphertexts: ModUp digits of c1 (EvalKeySwitchPrecomputeCore) and their
// inner product with the eval key over Q_l P (EvalFastKeySwitchCoreExt) -> til [cnt][2][ext][N].
// With the radix kernels the fp64 Q limbs finish their forward transform inside k_row_inner_fp (digits stay on chip);
// integer limbs (q0, P) take k_row3_inner_int, or the row pass + k_inner_product_b on ring sizes without it.
bool Engine::keyswitch_digits(const u64 *c1, size_t ct_stride, const u64 *evk, u64 *coef, u64 *dig, u64 *til, u64 *pc,
                              uint32_t cnt, uint32_t nl) {
    const uint32_t ext = nl + ps_.K, nparts = ps_.num_parts(nl), D = ps_.D;
    const int row_h = fast_row(tabs_.log_r2, 1u << tabs_.log_r1);
    unsigned long long fp_mask = 0, all_mask = ext >= 64 ? ~0ull : ((1ull << ext) - 1);
    for (uint32_t i = 0; i < nl; ++i)
        if (tabs_.h_fp_of[i]) fp_mask |= 1ull << i;
    // fp64-class P limbs (aux_bits <= 50) are in neither fused kernel: k_row_inner_fp covers the Q slots of fp_mask only
    // and the integer kernels cannot read their tables, so such a context takes the full row pass + k_inner_product_b
    // (the condition of qsum_ok and fanout_fused)
    bool p_fp = false;
    for (uint32_t k = 0; k < ps_.K; ++k)
        if (tabs_.h_fp_of[ps_.L + k]) p_fp = true;
    const bool fuse = fp_mask != 0 && !p_fp && (row_h == 3 || row_h == 4 || row_h == 9) &&
                      fast_log_h(tabs_.log_r1, 1u << tabs_.log_r2) != 0;
    const bool fuse_int = fuse && (row_h == 4 || row_h == 9);  // +1.3 % at C3
    {
        struct Reset {  // cleared on every exit path: the public ModUp entry point must never inherit it
            bool &flag;
            ~Reset() { flag = false; }
        } reset{skip_rows_};
        skip_rows_ = fuse_int;  // no separate row pass at all: both classes finish inside the fused kernels
        modup_core(c1, ct_stride, coef, dig, cnt, nl, fuse);
    }
    if (fuse) {
        InnerArgs a{dig, c1, evk, til, ct_stride, nl, ext, D, ps_.alpha, cnt, fp_mask,
                    (uint32_t)__builtin_popcountll(fp_mask)};
        if (!dispatch<3, 4, 9>(row_h, [&](auto rh) {
                if constexpr (decltype(rh)::value == 9) launch_row3_inner_fp_n<3>(a, tabs_, nparts, stream_);
                else launch_row_inner_fp_n<decltype(rh)::value>(a, tabs_, nparts, stream_);
            }))
            throw std::logic_error("fused fp64 inner product: no kernel for this row radix");
    }
    const unsigned long long mask = fuse ? (all_mask & ~fp_mask) : all_mask;
    if (fuse_int) {  // integer limbs: row pass + inner product in one three-round kernel as well
        InnerArgs a{dig, c1, evk, til, ct_stride, nl, ext, D, ps_.alpha, cnt, mask, (uint32_t)__builtin_popcountll(mask)};
        u64 *pc_fused = pc;
        // 256-point rows: 8 x 8 x 4 (LOGC 2); 512-point rows: 8 x 8 x 8 (LOGC 3)
        if (!dispatch<4, 9>(row_h, [&](auto rh) {
                launch_row3_inner_int_n<decltype(rh)::value == 9 ? 3 : 2>(a, tabs_, nparts, ps_.L, pc_fused, ps_.K, stream_);
            }))
            throw std::logic_error("fused integer inner product: no kernel for this row radix");
        MK_HIP(hipGetLastError());
        return pc_fused != nullptr;
    }
    inner_product_all(c1, ct_stride, evk, dig, til, cnt, nl, mask);
    return false;
}

// EvalFastKeySwitchCoreExt on fully transformed digits (k_inner_product_b) over the slots of `mask`
void Engine::inner_product_all(const u64 *c1, size_t ct_stride, const u64 *evk, const u64 *dig, u64 *til, uint32_t cnt,
                               uint32_t nl, unsigned long long mask) {
    const uint32_t n = ps_.n, ext = nl + ps_.K, nparts = ps_.num_parts(nl), D = ps_.D;
    EwGeom g{n, nl, ps_.L};
    if (!dispatch<1, 2, 3, 4, 5, 6>(nparts, [&](auto np) {
            launch_inner<decltype(np)::value>(dig, c1, ct_stride, evk, til, g, d_limb_, ext, D, ps_.alpha, cnt, mask, stream_);
        }))
        throw std::invalid_argument("more than 6 key-switch digits unsupported");
    MK_HIP(hipGetLastError());
}

void Engine::reencrypt_chunk(const u64 *ct, const u64 *evk, u64 *out, uint32_t cnt, uint32_t nl, bool accumulate) {
    const uint32_t n = ps_.n, K = ps_.K, ext = nl + K, nparts = ps_.num_parts(nl);
    const size_t ct_stride = (size_t)2 * nl * n;
    const size_t w_coef = (size_t)cnt * nl * n, w_dig = (size_t)cnt * nparts * ext * n;
    const size_t w_til = (size_t)cnt * 2 * ext * n, w_pc = (size_t)cnt * 2 * K * n, w_conv = (size_t)cnt * 2 * nl * n;
    u64 *ws = workspace(w_coef + w_dig + w_til + w_pc + w_conv);
    u64 *coef = ws, *dig = coef + w_coef, *til = dig + w_dig, *pc = til + w_til, *conv = pc + w_pc;
    const u64 *c1 = ct + (size_t)nl * n;  // component 1 of item 0; items are ct_stride apart

    // S1-S4: ModUp digits of c1 and their inner product with the eval key
    const bool p_rows = keyswitch_digits(c1, ct_stride, evk, coef, dig, til, pc, cnt, nl);
    // S5: ApproxModDown of both components (2*cnt polynomials of ext limbs), + c0 on component 0
    moddown_core(til, pc, conv, out, (size_t)nl * n, ct, ct_stride, 2 * cnt, nl, accumulate, p_rows);
}

template <int LOGC, int MINW, bool W = false>
static void launch_qsum3_fp(const QSumArgs &a, const NttTables &T, uint32_t nparts, hipStream_t s) {
    const uint32_t tiles = (1u << T.log_r1) / RowT<LOGC>::ROWS;
    const dim3 grid(tiles * a.nsel * a.cnt);
    if (!dispatch<1, 2, 3, 4, 5, 6>(nparts, [&](auto np) {
            k_qsum3_fp<decltype(np)::value, LOGC, MINW, W><<<grid, NTT_THREADS, 0, s>>>(a, T);
        }))
        throw std::invalid_argument("more than 6 key-switch digits unsupported");
}

// the integer-class Q limbs (a.slot_mask) in the same shape; two digits at least (a single-digit context keeps the
// two-kernel form, whose q_0 instance runs 3 waves per SIMD)
template <int LOGC, bool W>
static void launch_qsum3_int(const QSumArgs &a, const NttTables &T, uint32_t nparts, hipStream_t s) {
    const uint32_t tiles = (1u << T.log_r1) / RowT<LOGC>::ROWS;
    const dim3 grid(tiles * a.nsel * a.cnt);
    if (!dispatch<2, 3, 4, 5, 6>(nparts, [&](auto np) {
            with_int_arith(T, [&](auto ar) {
                k_qsum3_int<decltype(np)::value, LOGC, decltype(ar)::value, W><<<grid, NTT_THREADS, 0, s>>>(a, T);
            });
        }))
        throw std::invalid_argument("k_qsum3_int: 2 to 6 key-switch digits");
}

// per Q limb: P mod q, (P mod q)/q, P^-1 mod q, (P^-1 mod q)/q as doubles (fp64-class limbs; zeros elsewhere)
const u64 *Engine::p_doubles() {
    auto it = vec_cache_.find("p_doubles");
    if (it != vec_cache_.end()) return it->second;
    std::vector<u64> v(4 * (size_t)ps_.L, 0);
    for (uint32_t i = 0; i < ps_.L; ++i) {
        if (!ps_.limb[i].fp) continue;
        const long double q = (long double)ps_.moduli[i];
        const u64 pm = ps_.p_mod(i), pi = ps_.p_inv_mod(i);
        const double d[4] = {(double)pm, (double)((long double)pm / q), (double)pi, (double)((long double)pi / q)};
        std::memcpy(&v[4 * (size_t)i], d, sizeof(d));
    }
    return limb_vector("p_doubles", v);
}

// the merged n-client flow needs: radix column kernels (64- or 256-point columns), 256- or 512-point rows (k_qsum3_fp,
// k_row3_inner_int and the fused tail + sum kernels exist for them), fp64-class Q limbs, integer-class P limbs
bool Engine::qsum_ok(uint32_t nl) const {
    const int row_h = fast_row(tabs_.log_r2, 1u << tabs_.log_r1);
    if ((row_h != 4 && row_h != 9) || fast_log_h(tabs_.log_r1, 1u << tabs_.log_r2) < 3) return false;
    for (uint32_t k = 0; k < ps_.K; ++k)
        if (tabs_.h_fp_of[ps_.L + k]) return false;  // k_icol_sum sums the P-limb coefficients as 64-bit integers
    for (uint32_t i = 0; i < nl; ++i)
        if (tabs_.h_fp_of[i]) return true;
    return false;
}

// sum over clients of ReEncrypt(ct_c[b], evk_c).  Merged flow (N = 2^14, 2^16 with fp64-class limbs): per chunk of
// ciphertext indices and group of clients, every phase is ONE launch over all (client, index) items:
//   ModUp of c1 -> converted digits (column-passed)                          modup_core
//   P limbs: row pass + eval-key inner product + inverse row pass            k_row3_inner_int<.., true>
//   ApproxModDown's conversion P -> Q_l (column-passed)                      moddown_convert
//   integer-class Q limbs (q_0): everything that is left, summed over clients  k_qsum3_int
//     calls whose grid cannot fill the chip (q0_walk_fused) and single-digit contexts: inner product through a compact
//     til, then row pass + tail + sum                                        k_row3_inner_int<.., false>, k_row3_tail_once
//   fp64-class Q limbs: everything that is left, summed over clients        k_qsum3_fp
void Engine::reencrypt_sum_merged(const u64 *cts, const u64 *evks, u64 *out, uint32_t n_clients, uint32_t n_ct,
                                  uint32_t nl, const u64 *wt) {
    const uint32_t n = ps_.n, K = ps_.K, ext = nl + K, nparts = ps_.num_parts(nl), D = ps_.D;
    const size_t ct_words = (size_t)2 * nl * n, evk_words = (size_t)ps_.beta * 2 * D * n;
    const u64 *pinv = p_inverse(nl), *pq = p_doubles();
    unsigned long long fp_mask = 0, intq_mask = 0, p_mask = 0;
    for (uint32_t i = 0; i < nl; ++i) (tabs_.h_fp_of[i] ? fp_mask : intq_mask) |= 1ull << i;
    for (uint32_t i = nl; i < ext; ++i) p_mask |= 1ull << i;
    const uint32_t n_intq = (uint32_t)__builtin_popcountll(intq_mask);
    // clients per pass: the group's P-limb coefficients are summed as 64-bit integers (k_icol_sum), so a group holds at
    // most floor((2^64 - 1) / max p_k) clients (15 for 60-bit P limbs)
    u64 max_p = 1;
    for (uint32_t k = 0; k < K; ++k) max_p = std::max(max_p, ps_.moduli[ps_.L + k]);
    const uint32_t group = std::min({n_clients, knobs_.qsum_group, (uint32_t)std::min<u64>(64, ~0ull / max_p)});
    const bool wide_rows = fast_row(tabs_.log_r2, 1u << tabs_.log_r1) == 9;  // N = 2^17: 512-point rows, three-round kernels
    // the kernel instances of this call, f(lc, w): LOGC 2 (256-point rows) or 3 (512-point), w = std::bool_constant<weighted>
    auto with_rows_and_weight = [&](auto &&f) {
        dispatch<2, 3>(wide_rows ? 3 : 2, [&](auto lc) {
            dispatch<0, 1>(wt ? 1 : 0, [&](auto w) { f(lc, std::bool_constant<decltype(w)::value != 0>{}); });
        });
    };
    // One stream: running the memory-bound sums of group g on a second stream beside the multiply-bound phases of group
    // g+1 was measured neutral to slightly negative (20.47 k against 20.59 k ct/s at groups of 4): both kinds of kernel
    // fill the register file of a CU, so the hardware time-slices them instead of co-scheduling.
    const uint32_t max_items = group * std::min(knobs_.chunk, n_ct);
    const size_t w_coef = (size_t)max_items * nl * n, w_dig = (size_t)max_items * nparts * ext * n;
    const size_t w_pc = (size_t)max_items * 2 * K * n;
    // q_0 in one kernel or in two, per chunk (the last chunk of a call may be shorter and take the other form)
    const uint32_t q0_tiles = (1u << tabs_.log_r1) / (wide_rows ? RowT<3>::ROWS : RowT<2>::ROWS);
    auto q0_fused = [&](uint32_t cnt) {
        return n_intq != 0 && nparts >= 2 && q0_walk_fused(q0_tiles, n_intq, cnt, knobs_.q0_walk);
    };
    const uint32_t cnt_full = std::min(knobs_.chunk, n_ct), cnt_last = n_ct % knobs_.chunk ? n_ct % knobs_.chunk : cnt_full;
    // the compact til exists only for the two-kernel form
    const bool any_til = n_intq != 0 && (!q0_fused(cnt_full) || !q0_fused(cnt_last));
    const size_t w_til = any_til ? (size_t)max_items * 2 * n_intq * n : 0;
    const size_t w_csum = (size_t)std::min(knobs_.chunk, n_ct) * 2 * nl * n;  // conversions summed over a group's clients
    const size_t w_psum = (size_t)std::min(knobs_.chunk, n_ct) * 2 * K * n;   // P-limb coefficients summed over a group's clients
    u64 *ws = workspace(w_coef + w_dig + w_pc + w_til + w_csum + w_psum);
    hipStream_t main = stream_;
    for (uint32_t b0 = 0; b0 < n_ct; b0 += knobs_.chunk) {
        const uint32_t cnt = std::min(knobs_.chunk, n_ct - b0);
        for (uint32_t g0 = 0; g0 < n_clients; g0 += group) {
            const uint32_t gc = std::min(group, n_clients - g0), items = gc * cnt;
            u64 *coef = ws, *dig = coef + w_coef, *pc = dig + w_dig, *til = pc + w_pc, *convsum = til + w_til;
            u64 *psum = convsum + w_csum;
            const u64 *ct0 = cts + ((size_t)g0 * n_ct + b0) * ct_words;  // client g0, index b0
            const u64 *c1 = ct0 + (size_t)nl * n, *evk0 = evks + (size_t)g0 * evk_words;
            const size_t ct_cstride = (size_t)n_ct * ct_words;
            {   // ModUp of every item's c1: column-passed converted limbs; the row passes happen in the consumers
                struct Reset {
                    bool &flag;
                    ~Reset() { flag = false; }
                } reset{skip_rows_};
                skip_rows_ = true;
                // P-scaled tables: the converted P limbs hold sc_k d_j, so k_icol_sum's outputs need no scaling
                modup_core(c1, ct_words, coef, dig, items, nl, true, cnt, ct_cstride, true);
            }
            InnerArgs ia{dig, c1, evk0, til, ct_words, nl, ext, D, ps_.alpha, items, 0, 0};
            ia.ipc = cnt;
            ia.c1_gstride = ct_cstride;
            ia.evk_cstride = evk_words;
            {   // P limbs: accumulators straight through the inverse row pass into pc
                InnerArgs ap = ia;
                ap.slot_mask = p_mask;
                ap.nsel = K;
                if (wide_rows) launch_row3_inner_int_k<3, true>(ap, tabs_, nparts, ps_.L, pc, K, main);
                else launch_row3_inner_int_k<2, true>(ap, tabs_, nparts, ps_.L, pc, K, main);
            }
            {   // ApproxModDown: inverse column pass of every item's P limbs, summed over the group's clients as integers
                // (k_icol_sum), then ONE conversion P -> Q_l and forward column pass per (index, component, target limb)
                launch_icol_sum(pc, psum, tabs_, K, 2 * cnt, gc, (size_t)cnt * 2 * K * n, main);
                ConvIo cs{psum, convsum, (size_t)K * n, (size_t)nl * n, 2 * cnt, 0, 0};
                launch_conv_col_psum(cs, tabs_, moddown_conv(nl), main);
            }
            const bool fused_q0 = q0_fused(cnt);
            if (n_intq && !fused_q0) {  // integer-class Q limbs: accumulators through a compact til
                InnerArgs aq = ia;
                aq.slot_mask = intq_mask;
                aq.nsel = n_intq;
                aq.til_compact = 1;
                if (wide_rows) launch_row3_inner_int_k<3, false>(aq, tabs_, nparts, ps_.L, nullptr, K, main);
                else launch_row3_inner_int_k<2, false>(aq, tabs_, nparts, ps_.L, nullptr, K, main);
            }
            MK_HIP(hipGetLastError());
            if (fused_q0) {  // q_0: inner products, sum over the group's clients, summed conversion and tail in one kernel
                QSumArgs qi{dig, convsum, ct0, evk0, out + (size_t)b0 * ct_words, pq, ct_cstride, ct_words, evk_words, ct_words,
                            gc, cnt, nl, ext, D, ps_.alpha, intq_mask, n_intq, g0 != 0 ? 1u : 0u,
                            wt ? wt + (size_t)g0 * D * WT_WORDS : nullptr, pinv, pinv + nl};
                with_rows_and_weight([&](auto lc, auto w) {
                    launch_qsum3_int<decltype(lc)::value, decltype(w)::value>(qi, tabs_, nparts, main);
                });
            } else if (n_intq) {  // q_0: row pass of the summed conversion, tail, sum over the group's clients
                TailOnceArgs ta{convsum, til, ct0, out + (size_t)b0 * ct_words, pinv, pinv + nl,
                                (size_t)cnt * 2 * n_intq * n, ct_cstride, ct_words, gc, nl, 2 * cnt, intq_mask, n_intq,
                                g0 != 0 ? 1u : 0u, wt ? wt + (size_t)g0 * D * WT_WORDS : nullptr, D};
                with_rows_and_weight([&](auto lc, auto w) {  // weighted: M_c * c0 per client
                    constexpr int LOGC = decltype(lc)::value;
                    const dim3 grid(((1u << tabs_.log_r1) / RowT<LOGC>::ROWS) * n_intq * 2 * cnt);
                    with_int_arith(tabs_, [&](auto ar) {
                        k_row3_tail_once<LOGC, decltype(ar)::value, decltype(w)::value>
                            <<<grid, NTT_THREADS, 0, main>>>(ta, tabs_);
                    });
                });
            }
            QSumArgs qa{dig, convsum, ct0, evk0, out + (size_t)b0 * ct_words, pq, ct_cstride, ct_words, evk_words, ct_words,
                        gc, cnt, nl, ext, D, ps_.alpha, fp_mask, (uint32_t)__builtin_popcountll(fp_mask), g0 != 0 ? 1u : 0u,
                        wt ? wt + (size_t)g0 * D * WT_WORDS : nullptr};
            // 256-point rows: 2 workgroups per CU -- at N = 2^16, L = 12 the kernel's 5 632 workgroups then fill the 512 resident
            // slots exactly 11 times (7.33 times 768 at 3 per CU: a last round a third full) and nothing is parked in scratch;
            // +0.45 % on the step after the eval-key bursts (it was +-0 before them)
            with_rows_and_weight([&](auto lc, auto w) {  // MINW = LOGC: the two pairs the kernel exists for
                launch_qsum3_fp<decltype(lc)::value, decltype(lc)::value, decltype(w)::value>(qa, tabs_, nparts, main);
            });
            MK_HIP(hipGetLastError());
        }
    }
}

void Engine::reencrypt_sum(const u64 *cts, const u64 *evks, u64 *out, uint32_t n_clients, uint32_t n_ct, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!n_clients || !n_ct) return;
    const size_t ct_words = (size_t)2 * nl * ps_.n, evk_words = (size_t)ps_.beta * 2 * ps_.D * ps_.n;
    if (qsum_ok(nl)) {  // N = 2^14, 2^16, 2^17 with fp64-class Q limbs: every phase one launch over all (client, index) items
        reencrypt_sum_merged(cts, evks, out, n_clients, n_ct, nl, nullptr);
        return;
    }
    // other ring sizes / arithmetic classes: one re-encryption per client with the accumulating tail
    for (uint32_t c = 0; c < n_clients; ++c)
        reencrypt(cts + (size_t)c * n_ct * ct_words, evks + (size_t)c * evk_words, out, n_ct, nl, c != 0);
}

void Engine::reencrypt(const u64 *ct, const u64 *evk, u64 *out, uint32_t n_ct, uint32_t nl, bool accumulate) {
    need_device();
    check_nl(nl);
    if (accumulate && ct == out) throw std::invalid_argument("accumulating re-encryption cannot run in place");
    const size_t ct_stride = (size_t)2 * nl * ps_.n;
    for (uint32_t done = 0; done < n_ct; done += knobs_.chunk) {
        const uint32_t cnt = n_ct - done < knobs_.chunk ? n_ct - done : knobs_.chunk;
        reencrypt_chunk(ct + done * ct_stride, evk, out + done * ct_stride, cnt, nl, accumulate);
    }
}

// ---- weighted aggregation ("weighted aggregation") -------------------------------------------------------

// Device table of the constants M_k = trunc(w_k * sf(sf_level) + 0.5) over all D limbs, WT_WORDS words per (k, limb).
// Cached per (sf_level, weights) like rescale_consts, so a server step that repeats its weights uploads nothing and no
// call synchronises per chunk; the cache is small and emptied (after one stream synchronisation) when it is full, since
// a long-running server sees new weights every round.
const u64 *Engine::weight_table(const double *w, uint32_t n, uint32_t sf_level) {
    if (!w) throw std::invalid_argument("null weights");
    std::string key((const char *)w, (size_t)n * sizeof(double));
    key += "@" + std::to_string(sf_level);
    auto it = wt_cache_.find(key);
    if (it != wt_cache_.end()) return it->second;
    const uint32_t D = ps_.D;
    std::vector<u64> t((size_t)n * D * WT_WORDS, 0);
    for (uint32_t k = 0; k < n; ++k) {
        const std::vector<u64> f = ps_.const_factors_qp(sf_level, w[k]);  // throws on a weight that does not fit
        for (uint32_t i = 0; i < D; ++i) {
            u64 *e = &t[((size_t)k * D + i) * WT_WORDS];
            const u64 q = ps_.moduli[i];
            e[0] = f[i];
            e[1] = h_shoup(f[i], q);
            if (i < ps_.L && ps_.limb[i].fp) {
                const u64 pmw = h_mulmod(ps_.p_mod(i), f[i], q);
                const double d[2] = {(double)pmw, (double)((long double)pmw / (long double)q)};
                std::memcpy(e + 2, d, sizeof(d));
            }
        }
    }
    return cache_table(key, t);
}

void Engine::scale_evk(const u64 *in, u64 *out, uint32_t n_keys, const double *w, uint32_t sf_level) {
    need_device();
    if (!n_keys) return;
    const uint32_t n = ps_.n, D = ps_.D, polys_per_key = 2 * ps_.beta;
    const size_t bytes = (size_t)n_keys * polys_per_key * D * n * sizeof(u64);
    if (ranges_overlap(in, bytes, out, bytes)) throw std::invalid_argument("output overlaps input");
    if ((size_t)n_keys * polys_per_key > 65535) throw std::invalid_argument("too many keys in one call");
    const u64 *wt = weight_table(w, n_keys, sf_level);
    k_scale_keys<<<dim3((n / 2 + EW_THREADS - 1) / EW_THREADS, D, n_keys * polys_per_key), EW_THREADS, 0, stream_>>>(
        in, out, n, D, polys_per_key, d_limb_, wt);
    MK_HIP(hipGetLastError());
}

// sum over clients of ReEncrypt((M_c * c0_c[b], c1_c[b]), evk'_c) with evk'_c = M_c * evk_c made by scale_evk from the
// same weights and level
void Engine::reencrypt_wsum(const u64 *cts, const u64 *evks_scaled, u64 *out, uint32_t n_clients, uint32_t n_ct, uint32_t nl,
                            const double *w, uint32_t sf_level) {
    need_device();
    check_nl(nl);
    if (!n_clients || !n_ct) return;
    const size_t ct_words = (size_t)2 * nl * ps_.n, evk_words = (size_t)ps_.beta * 2 * ps_.D * ps_.n;
    if (ranges_overlap(cts, (size_t)n_clients * n_ct * ct_words * sizeof(u64), out, (size_t)n_ct * ct_words * sizeof(u64)))
        throw std::invalid_argument("output overlaps input");
    const u64 *wt = weight_table(w, n_clients, sf_level);
    if (qsum_ok(nl)) {
        reencrypt_sum_merged(cts, evks_scaled, out, n_clients, n_ct, nl, wt);
        return;
    }
    // other ring sizes / arithmetic classes: the composition, chunk by chunk -- c0 scaled into a buffer of its own (the
    // re-encryption owns the workspace), then the accumulating re-encryption with the scaled key
    const uint32_t chunk = std::min(knobs_.chunk, n_ct);
    u64 *scaled = chunk_buffer((size_t)chunk * ct_words);
    EwGeom g{ps_.n, nl, ps_.L};
    for (uint32_t c = 0; c < n_clients; ++c)
        for (uint32_t b0 = 0; b0 < n_ct; b0 += chunk) {
            const uint32_t cnt = std::min(chunk, n_ct - b0);
            k_scale_c0<<<ew_grid(ps_.n, 2 * nl, cnt), EW_THREADS, 0, stream_>>>(
                cts + ((size_t)c * n_ct + b0) * ct_words, scaled, g, d_limb_, wt + (size_t)c * ps_.D * WT_WORDS);
            MK_HIP(hipGetLastError());
            reencrypt_chunk(scaled, evks_scaled + (size_t)c * evk_words, out + (size_t)b0 * ct_words, cnt, nl, c != 0);
        }
}

void Engine::eval_wsum(const u64 *in, u64 *out, uint32_t n_terms, uint32_t n_ct, uint32_t nl, const double *w,
                       uint32_t sf_level, bool first_is_sum) {
    need_device();
    check_nl(nl);
    if (!n_terms || !n_ct) return;
    const size_t term_words = (size_t)n_ct * 2 * nl * ps_.n;
    // a thread reads its words of every term before it writes them, so out may be term 0 itself; any other overlap is a race
    if (out != in && ranges_overlap(in, (size_t)n_terms * term_words * sizeof(u64), out, term_words * sizeof(u64)))
        throw std::invalid_argument("output overlaps input (it may only be term 0 itself)");
    std::vector<double> ww(w, w + n_terms);
    if (first_is_sum) ww[0] = 1.0;  // ignored by the kernel; keeps the cache key and the range check independent of it
    const u64 *wt = weight_table(ww.data(), n_terms, sf_level);
    EwGeom g{ps_.n, nl, ps_.L};
    k_wsum_ct<<<ew_grid(ps_.n, 2 * nl, n_ct), EW_THREADS, 0, stream_>>>(in, out, g, d_limb_, 2 * nl, n_terms, term_words, wt,
                                                                      ps_.D, first_is_sum ? 1 : 0);
    MK_HIP(hipGetLastError());
}

// the three instances of the fused fan-out kernels over one chunk of ciphertexts and one group of keys
template <int NPARTS, int LOGC>
static void launch_fan3(const FanArgs &a0, const NttTables &T, uint32_t L, unsigned long long fp_mask,
                        unsigned long long intq_mask, unsigned long long p_mask, hipStream_t s) {
    const uint32_t tiles = (1u << T.log_r1) / RowT<LOGC>::ROWS;
    auto select = [&](unsigned long long m) {
        FanArgs a = a0;
        a.slot_mask = m;
        a.nsel = (uint32_t)__builtin_popcountll(m);
        return a;
    };
    if (p_mask) {  // first: ModDown starts from their output
        const FanArgs a = select(p_mask);
        with_int_arith(T, [&](auto ar) {
            k_fan3_inner_int<NPARTS, LOGC, true, decltype(ar)::value>
                <<<dim3(tiles * a.nsel * a.items), NTT_THREADS, 0, s>>>(a, T, L);
        });
    }
    if (intq_mask) {
        const FanArgs a = select(intq_mask);
        with_int_arith(T, [&](auto ar) {
            k_fan3_inner_int<NPARTS, LOGC, false, decltype(ar)::value>
                <<<dim3(tiles * a.nsel * a.items), NTT_THREADS, 0, s>>>(a, T, L);
        });
    }
    if (fp_mask) {
        const FanArgs a = select(fp_mask);
        k_fan3_inner_fp<NPARTS, LOGC><<<dim3(tiles * a.nsel * a.items), NTT_THREADS, 0, s>>>(a, T);
    }
}
template <int LOGC>
static void launch_fan3_n(const FanArgs &a, const NttTables &T, uint32_t nparts, uint32_t L, unsigned long long fp_mask,
                          unsigned long long intq_mask, unsigned long long p_mask, hipStream_t s) {
    if (!dispatch<1, 2, 3, 4, 5, 6>(nparts, [&](auto np) {
            launch_fan3<decltype(np)::value, LOGC>(a, T, L, fp_mask, intq_mask, p_mask, s);
        }))
        throw std::invalid_argument("more than 6 key-switch digits unsupported");
}

// the fused fan-out kernels need what keyswitch_digits needs for its fully fused form: radix column kernels, 256- or
// 512-point rows, fp64-class Q limbs; and integer-class P limbs (their accumulators run through row3_inverse_int)
bool Engine::fanout_fused(uint32_t nl) const {
    const int row_h = fast_row(tabs_.log_r2, 1u << tabs_.log_r1);
    if ((row_h != 4 && row_h != 9) || fast_log_h(tabs_.log_r1, 1u << tabs_.log_r2) == 0) return false;
    for (uint32_t k = 0; k < ps_.K; ++k)
        if (tabs_.h_fp_of[ps_.L + k]) return false;
    for (uint32_t i = 0; i < nl; ++i)
        if (tabs_.h_fp_of[i]) return true;
    return false;
}

// out[k][b] = ReEncrypt(ct[b], evks[k]).  Per chunk of ciphertexts the key-independent half of the key switch runs
// once: INTT of c1 + ModUp conversions + forward column pass (modup_core).  Fused path (N = 2^14, 2^16, 2^17 with
// fp64-class Q limbs), per group of keys:
//   row pass of every converted digit once per (ciphertext, limb, row tile), then per key the inner product
//   (+ inverse row pass on the P limbs)                                        k_fan3_inner_fp, k_fan3_inner_int
//   ApproxModDown of all (key, ciphertext, component) polynomials at once      moddown_core (grouped tail)
// Other ring sizes / arithmetic classes: ModUp with its row pass once, then k_inner_product_b + ModDown per key.
void Engine::reencrypt_fanout(const u64 *ct, const u64 *evks, u64 *out, uint32_t n_keys, uint32_t n_ct, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!n_keys || !n_ct) return;
    const size_t ct_bytes = (size_t)n_ct * 2 * nl * ps_.n * sizeof(u64);
    if (ranges_overlap(ct, ct_bytes, out, n_keys * ct_bytes))
        throw std::invalid_argument("fan-out re-encryption cannot write over its input");
    fanout_core(ct, nl, evks, out, n_keys, n_ct, nl, false);
}

// out[k][b] = Rescale(ReEncrypt(prefix(ct[b], nl_out + 1), evks[k])): the fan-out at nl = nl_out + 1 limbs on the
// aggregate's prefix, read in place, with the closing rescale of every (key, ciphertext, component) polynomial of a
// group as one pass into the compact layout
void Engine::reencrypt_fanout_compact(const u64 *ct, const u64 *evks, u64 *out, uint32_t n_keys, uint32_t n_ct, uint32_t nl_in,
                                      uint32_t nl_out) {
    need_device();
    check_nl(nl_in);
    if (nl_out < 1 || nl_out >= nl_in) throw std::invalid_argument("compact fan-out needs 1 <= nl_out < nl_in");
    if (!n_keys || !n_ct) return;
    const size_t poly_bytes = (size_t)n_ct * 2 * ps_.n * sizeof(u64);
    if (ranges_overlap(ct, poly_bytes * nl_in, out, n_keys * poly_bytes * nl_out))
        throw std::invalid_argument("fan-out re-encryption cannot write over its input");
    fanout_core(ct, nl_in, evks, out, n_keys, n_ct, nl_out + 1, true);
}

void Engine::fanout_core(const u64 *ct, uint32_t in_limbs, const u64 *evks, u64 *out, uint32_t n_keys, uint32_t n_ct, uint32_t nl,
                         bool compact) {
    const uint32_t n = ps_.n, K = ps_.K, ext = nl + K, nparts = ps_.num_parts(nl), D = ps_.D;
    // input ciphertexts are in_limbs wide (the kernels take the stride and the c0 / c1 pointers apart from nl); the
    // key-switched ciphertexts have nl limbs, the outputs of the compact form nl - 1
    const size_t ct_words = (size_t)2 * in_limbs * n, ks_words = (size_t)2 * nl * n, evk_words = (size_t)ps_.beta * 2 * D * n;
    const size_t out_words = compact ? (size_t)2 * (nl - 1) * n : ks_words;
    const bool fused = fanout_fused(nl);
    unsigned long long fp_mask = 0, intq_mask = 0, p_mask = 0, all_mask = ext >= 64 ? ~0ull : ((1ull << ext) - 1);
    for (uint32_t i = 0; i < nl; ++i) (tabs_.h_fp_of[i] ? fp_mask : intq_mask) |= 1ull << i;
    for (uint32_t i = nl; i < ext; ++i) p_mask |= 1ull << i;
    const uint32_t chunk = std::min(knobs_.chunk, n_ct), group = fused ? std::min(knobs_.fanout_group, n_keys) : 1u;
    const size_t w_coef = (size_t)chunk * nl * n, w_dig = (size_t)chunk * nparts * ext * n;
    const size_t w_til = (size_t)group * chunk * 2 * ext * n, w_pc = (size_t)group * chunk * 2 * K * n;
    const size_t w_conv = (size_t)group * chunk * 2 * nl * n;
    const size_t w_ks = compact ? (size_t)group * chunk * ks_words : 0;  // key-switched group ahead of its rescale
    const u64 *d_c = compact ? rescale_consts(nl, nullptr) : nullptr;
    u64 *ws = workspace(w_coef + w_dig + w_til + w_pc + w_conv + w_ks);
    u64 *coef = ws, *dig = coef + w_coef, *til = dig + w_dig, *pc = til + w_til, *conv = pc + w_pc, *ks = conv + w_conv;
    const bool wide_rows = fast_row(tabs_.log_r2, 1u << tabs_.log_r1) == 9;
    for (uint32_t b0 = 0; b0 < n_ct; b0 += chunk) {
        const uint32_t cnt = std::min(chunk, n_ct - b0);
        const u64 *ct0 = ct + (size_t)b0 * ct_words, *c1 = ct0 + (size_t)in_limbs * n;
        {   // the shared half; on the fused path the row passes are left to the fan-out kernels
            struct Reset {
                bool &flag;
                ~Reset() { flag = false; }
            } reset{skip_rows_};
            skip_rows_ = fused;
            modup_core(c1, ct_words, coef, dig, cnt, nl, fused);
        }
        for (uint32_t k0 = 0; k0 < n_keys; k0 += group) {
            const uint32_t gk = std::min(group, n_keys - k0);
            const u64 *evk0 = evks + (size_t)k0 * evk_words;
            u64 *out0 = out + ((size_t)k0 * n_ct + b0) * out_words;
            // compact: the group's key-switched ciphertexts go to ks [key][cnt][2][nl][N]
            u64 *sw0 = compact ? ks : out0;
            const size_t sw_gstride = compact ? (size_t)cnt * ks_words : (size_t)n_ct * ks_words;
            if (fused) {
                FanArgs a{dig, c1, evk0, til, pc, ct_words, evk_words, nl, ext, D, ps_.alpha, cnt, gk, K, 0, 0};
                if (wide_rows) launch_fan3_n<3>(a, tabs_, nparts, ps_.L, fp_mask, intq_mask, p_mask, stream_);
                else launch_fan3_n<2>(a, tabs_, nparts, ps_.L, fp_mask, intq_mask, p_mask, stream_);
                MK_HIP(hipGetLastError());
                // polynomial p = (key * cnt + b) * 2 + comp: c0 of ciphertext b, output of key k0 + key
                moddown_core(til, pc, conv, sw0, (size_t)nl * n, ct0, ct_words, gk * 2 * cnt, nl, false, true, 2 * cnt, sw_gstride);
            } else {
                inner_product_all(c1, ct_words, evk0, dig, til, cnt, nl, all_mask);
                moddown_core(til, pc, conv, sw0, (size_t)nl * n, ct0, ct_words, 2 * cnt, nl, false, false);
            }
            if (compact) {
                // the closing rescale of all gk * 2 * cnt polynomials at once; til is free again and holds its scratch
                // (ext words per polynomial against the 1 + (nl - 1) needed)
                const uint32_t polys = gk * 2 * cnt;
                rescale_core(ks, nl, out0, polys, nl, d_c, til, til + (size_t)polys * n, fused ? 2 * cnt : 0,
                             (size_t)n_ct * out_words);
            }
        }
    }
}

// ---- keys / client endpoints --------------------------------------------------------

void Engine::keygen(const int8_t *s, const u64 *a, const int32_t *e, u64 *pk, u64 *sk) {
    need_device();
    const uint32_t n = ps_.n, D = ps_.D, L = ps_.L;
    u64 *ee = workspace((size_t)D * n);
    EwGeom g{n, L, L};
    k_lift<int8_t><<<ew_grid(n, D, 1), EW_THREADS, 0, stream_>>>(s, sk, g, d_limb_, D);
    k_lift<int32_t><<<ew_grid(n, D, 1), EW_THREADS, 0, stream_>>>(e, ee, g, d_limb_, D);
    MK_HIP(hipGetLastError());
    ntt_launch(sk, 1, L, D, false, nullptr, nullptr);
    ntt_launch(ee, 1, L, D, false, nullptr, nullptr);
    // b = e - a*s ; a copied
    Opnd x{a, 0, 0}, y{sk, 0, 0}, z{ee, 0, 0}, none{nullptr, 0, 0};
    k_fma<<<ew_grid(n, D, 1), EW_THREADS, 0, stream_>>>(x, y, z, none, nullptr, 1, pk, 0, 0, g, d_limb_, D);
    MK_HIP(hipGetLastError());
    MK_HIP(hipMemcpyAsync(pk + (size_t)D * n, a, (size_t)D * n * sizeof(u64), hipMemcpyDeviceToDevice, stream_));
}

// the source key's transform se u64[D][N] lives at the head of the key generators' workspace
u64 *Engine::rekey_workspace() {
    return workspace((size_t)ps_.D * ps_.n * (1 + 3 * (size_t)ps_.beta) + ps_.D);
}

void Engine::rekeygen(const int8_t *s_old, const u64 *pk_new, const int8_t *u, const int32_t *e0,
                      const int32_t *e1, u64 *evk) {
    need_device();
    const uint32_t n = ps_.n, D = ps_.D, L = ps_.L;
    u64 *se = rekey_workspace();
    EwGeom g{n, L, L};
    k_lift<int8_t><<<ew_grid(n, D, 1), EW_THREADS, 0, stream_>>>(s_old, se, g, d_limb_, D);
    MK_HIP(hipGetLastError());
    ntt_launch(se, 1, L, D, false, nullptr, nullptr);
    rekeygen_from(pk_new, u, e0, e1, evk);
}

// KeySwitchGenInternal after the source key's transform: evk[j] = (pk0 u_j + e0_j + (P mod q_i) se on digit j's own
// limbs, pk1 u_j + e1_j) with se u64[D][N], EVALUATION, canonical, at the head of rekey_workspace().  Shared by
// rekeygen (se = NTT(s_old)), galois_keygen (through rekeygen) and relin_keygen (se = NTT(s)^2).
void Engine::rekeygen_from(const u64 *pk_new, const int8_t *u, const int32_t *e0, const int32_t *e1, u64 *evk) {
    const uint32_t n = ps_.n, D = ps_.D, L = ps_.L, beta = ps_.beta;
    const size_t poly = (size_t)D * n;
    u64 *ws = rekey_workspace();
    u64 *se = ws, *ue = se + poly, *e0e = ue + poly * beta, *e1e = e0e + poly * beta, *d_gadget = e1e + poly * beta;
    EwGeom g{n, L, L};
    k_lift<int8_t><<<ew_grid(n, D, beta), EW_THREADS, 0, stream_>>>(u, ue, g, d_limb_, D);
    k_lift<int32_t><<<ew_grid(n, D, beta), EW_THREADS, 0, stream_>>>(e0, e0e, g, d_limb_, D);
    k_lift<int32_t><<<ew_grid(n, D, beta), EW_THREADS, 0, stream_>>>(e1, e1e, g, d_limb_, D);
    MK_HIP(hipGetLastError());
    ntt_launch(ue, 3 * beta, L, D, false, nullptr, nullptr);  // ue, e0e, e1e are contiguous
    for (uint32_t part = 0; part < beta; ++part) {
        // gadget P mod q_i on the digit's own limbs, 0 elsewhere (KeySwitchGenInternal)
        std::vector<u64> gad(D, 0);
        const uint32_t lo = part * ps_.alpha, hi = std::min(L, lo + ps_.alpha);
        for (uint32_t i = lo; i < hi; ++i) gad[i] = ps_.p_mod(i);
        MK_HIP(hipMemcpyAsync(d_gadget, gad.data(), D * sizeof(u64), hipMemcpyHostToDevice, stream_));
        MK_HIP(hipStreamSynchronize(stream_));
        Opnd p0{pk_new, 0, 0}, p1{pk_new + poly, 0, 0}, uu{ue + part * poly, 0, 0};
        Opnd z0{e0e + part * poly, 0, 0}, z1{e1e + part * poly, 0, 0}, w{se, 0, 0}, none{nullptr, 0, 0};
        k_fma<<<ew_grid(n, D, 1), EW_THREADS, 0, stream_>>>(p0, uu, z0, w, d_gadget, 0, evk + (size_t)(part * 2 + 0) * poly,
                                                         0, 0, g, d_limb_, D);
        k_fma<<<ew_grid(n, D, 1), EW_THREADS, 0, stream_>>>(p1, uu, z1, none, nullptr, 0, evk + (size_t)(part * 2 + 1) * poly,
                                                         0, 0, g, d_limb_, D);
        MK_HIP(hipGetLastError());
        MK_HIP(hipStreamSynchronize(stream_));  // d_gadget is rewritten next iteration
    }
}

// ---- slot rotations ("rotations and slot sums"); overlaps and the span are refused in capi.cpp ---------------

// rows = (polynomial, limb) pairs, N words apart in both buffers
void Engine::launch_automorph(const u64 *in, u64 *out, size_t rows, uint32_t g) {
    if (!galois_valid(g, ps_.log_n)) throw std::invalid_argument("Galois element must be odd and below 2N");
    if (((uintptr_t)in | (uintptr_t)out) & 15) throw std::invalid_argument("polynomials must be 16-byte aligned");
    const uint32_t log_t = std::min(ps_.log_n, AUTO_LOG_TILE);
    const size_t blocks = rows << (ps_.log_n - log_t);
    if (blocks > 0x7fffffffu) throw std::invalid_argument("batch too large for one launch");
    if (!blocks) return;
    k_automorph<<<dim3((unsigned)blocks), AUTO_THREADS, 0, stream_>>>(in, out, g, ps_.log_n, log_t);
    MK_HIP(hipGetLastError());
}

void Engine::automorphism(const u64 *in, u64 *out, uint32_t n_polys, uint32_t nl, uint32_t g) {
    need_device();
    check_nl(nl);
    launch_automorph(in, out, (size_t)n_polys * nl, g);
}

void Engine::automorphism_secret(const int8_t *s, int8_t *out, uint32_t g) {
    need_device();
    if (!galois_valid(g, ps_.log_n)) throw std::invalid_argument("Galois element must be odd and below 2N");
    k_automorph_s8<<<(ps_.n + 255) / 256, 256, 0, stream_>>>(s, out, g, ps_.log_n);
    MK_HIP(hipGetLastError());
}

// the re-encryption key from sigma_g(s) to s: a ciphertext permuted by sigma_g decrypts under sigma_g(s)
void Engine::galois_keygen(const int8_t *s, const u64 *pk, const int8_t *u, const int32_t *e0, const int32_t *e1, uint32_t g,
                           u64 *evk) {
    need_device();
    if (!d_gal_s_) MK_HIP(hipMalloc(&d_gal_s_, ps_.n));
    automorphism_secret(s, d_gal_s_, g);
    rekeygen(d_gal_s_, pk, u, e0, e1, evk);
}

// Both components are permuted straight into `out`, where the key switch then runs in place: sigma_g(c1) exists once in
// HBM, as the source of the INTT and as the digits' own limbs, and sigma_g(c0) sits where the ModDown tail adds it.
// One read and one write of the ciphertext on top of reencrypt.
void Engine::rotate(const u64 *ct, const u64 *evk, u64 *out, uint32_t n_ct, uint32_t nl, uint32_t g) {
    need_device();
    check_nl(nl);
    const size_t ct_words = (size_t)2 * nl * ps_.n;
    for (uint32_t done = 0; done < n_ct; done += knobs_.chunk) {
        const uint32_t cnt = std::min(knobs_.chunk, n_ct - done);
        launch_automorph(ct + done * ct_words, out + done * ct_words, (size_t)cnt * 2 * nl, g);
        reencrypt_chunk(out + done * ct_words, evk, out + done * ct_words, cnt, nl, false);
    }
}

// out = ct; step k: out += ReEncrypt(sigma_g(out), evks[k]) with g = 5^(2^k): the permuted chunk goes to the chunk
// buffer, the accumulating ModDown tail adds the rotation to the running sum
void Engine::slot_sum(const u64 *ct, const u64 *evks, u64 *out, uint32_t n_ct, uint32_t nl, uint32_t span) {
    need_device();
    check_nl(nl);
    const size_t ct_words = (size_t)2 * nl * ps_.n, evk_words = (size_t)ps_.beta * 2 * ps_.D * ps_.n;
    if (!n_ct) return;
    const uint32_t chunk = std::min(knobs_.chunk, n_ct);
    u64 *perm = span > 1 ? chunk_buffer((size_t)chunk * ct_words) : nullptr;
    for (uint32_t done = 0; done < n_ct; done += chunk) {
        const uint32_t cnt = std::min(chunk, n_ct - done);
        u64 *acc = out + done * ct_words;
        MK_HIP(hipMemcpyAsync(acc, ct + done * ct_words, cnt * ct_words * sizeof(u64), hipMemcpyDeviceToDevice, stream_));
        for (uint32_t k = 0; (1u << k) < span; ++k) {
            launch_automorph(acc, perm, (size_t)cnt * 2 * nl, galois_element((int32_t)(1u << k), ps_.log_n));
            reencrypt_chunk(perm, evks + k * evk_words, acc, cnt, nl, true);
        }
    }
}

// ---- linear transforms ("linear transforms"); refusals of the arguments are decided in capi.cpp -------------

// EvalLinearTransform's shape with EvalFastRotation's hoisting, both hoists: per chunk one ModUp of c1 (modup_core, the
// digits of mkckks_modup_batch), one launch of k_lt_accum over the extended basis (every rotation an eval-key inner product
// on permuted digits, the plaintext diagonal multiplied in before the sum leaves Q_l P), one ModDown of both components
// (moddown_core, the words of mkckks_moddown_batch).
void Engine::linear_transform(const u64 *ct, const u64 *evks, const u64 *pts, const uint32_t *h_g, u64 *out, uint32_t n_rot,
                              uint32_t n_ct, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!n_rot || !n_ct) return;
    const uint32_t n = ps_.n, K = ps_.K, ext = nl + K, nparts = ps_.num_parts(nl);
    for (uint32_t r = 0; r < n_rot; ++r)
        if (!galois_valid(h_g[r], ps_.log_n)) throw std::invalid_argument("Galois element must be odd and below 2N");
    if (nparts > 6) throw std::invalid_argument("more than 6 key-switch digits unsupported");
    if (n_rot > lt_g_cap_) {
        MK_HIP(hipStreamSynchronize(stream_));
        if (d_lt_g_) MK_HIP(hipFree(d_lt_g_));
        d_lt_g_ = nullptr;
        lt_g_cap_ = 0;
        MK_HIP(hipMalloc(&d_lt_g_, (size_t)n_rot * sizeof(uint32_t)));
        lt_g_cap_ = n_rot;
    }
    // stream-ordered behind the previous call's kernel; the wait keeps the caller's array free to change on return
    MK_HIP(hipMemcpyAsync(d_lt_g_, h_g, (size_t)n_rot * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
    MK_HIP(hipStreamSynchronize(stream_));
    std::vector<u64> pm(nl);
    for (uint32_t i = 0; i < nl; ++i) pm[i] = ps_.p_mod(i);
    const u64 *pmod = limb_vector("pmod_" + std::to_string(nl), pm);

    const uint32_t log_t = std::min(ps_.log_n, LT_LOG_TILE);
    const size_t ct_words = (size_t)2 * nl * n;
    const uint32_t chunk = std::min(knobs_.chunk, n_ct);
    const size_t w_coef = (size_t)chunk * nl * n, w_dig = (size_t)chunk * nparts * ext * n;
    const size_t w_til = (size_t)chunk * 2 * ext * n, w_pc = (size_t)chunk * 2 * K * n, w_conv = (size_t)chunk * 2 * nl * n;
    u64 *ws = workspace(w_coef + w_dig + w_til + w_pc + w_conv);
    u64 *coef = ws, *dig = coef + w_coef, *til = dig + w_dig, *pc = til + w_til, *conv = pc + w_pc;
    for (uint32_t done = 0; done < n_ct; done += chunk) {
        const uint32_t cnt = std::min(chunk, n_ct - done);
        const u64 *c = ct + done * ct_words;
        modup_core(c + (size_t)nl * n, ct_words, coef, dig, cnt, nl);
        LtArgs a{c, dig, evks, pts, d_lt_g_, pmod, til, (size_t)ps_.beta * 2 * ps_.D * n,
                 n_rot, cnt, nl, ext, ps_.L, ps_.D, ps_.alpha, ps_.log_n, log_t,
                 ext << (ps_.log_n - log_t), knobs_.lt_order == 1 ? 1u : cnt, knobs_.lt_order == 1 ? 1u : 0u,
                 knobs_.lt_order == 2 ? 0u : 1u};
        const uint64_t blocks = (uint64_t)((a.groups + LT_XCDS - 1) / LT_XCDS * LT_XCDS) * a.members;
        if (blocks > 0x7fffffffu) throw std::invalid_argument("batch too large for one launch");
        dispatch<1, 2, 3, 4, 5, 6>(nparts, [&](auto np) {
            k_lt_accum<decltype(np)::value><<<dim3((unsigned)blocks), LT_THREADS, 0, stream_>>>(a, d_limb_);
        });
        MK_HIP(hipGetLastError());
        moddown_core(til, pc, conv, out + done * ct_words, (size_t)nl * n, nullptr, 0, 2 * cnt, nl, false);
    }
}

// The baby-step giant-step form (definition: include/mkckks.h; kernels: bsgs_kernels.hpp).  The plan is compacted on the
// host first: a baby whose column has no present entry and a giant whose row has none are dropped (they cost nothing,
// their ModDown and ModUp included), the giants with a key come first so that their Ua_t are one contiguous batch.
// Per chunk: modup_core(c1); k_bsgs_baby; k_bsgs_inner; ONE moddown_core and ONE modup_core over the keyed giants of
// every ciphertext of the chunk; k_bsgs_giant; moddown_core of both components.
// Workspace: babies, inner sums and giant digits are per ciphertext (words per ciphertext below); the chunk is
// min(knobs.chunk, max(1, cap / that)), cap = Knobs::bsgs_ws_mib (2 GiB; MKCKKS_BSGS_WS_MIB).  Every word of the result is
// a function of its own ciphertext alone, so the bits do not depend on the chunk.
void Engine::linear_transform_bsgs(const u64 *ct, const u64 *bkeys, const uint32_t *h_gb, uint32_t n1, const u64 *gkeys,
                                   const uint32_t *h_gg, uint32_t n2, const u64 *pts, const uint8_t *h_present, u64 *out,
                                   uint32_t n_ct, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!n1 || !n2 || n1 > BSGS_MAX || n2 > BSGS_MAX) throw std::invalid_argument("n1 and n2 must be in [1, 64]");
    const uint32_t n = ps_.n, K = ps_.K, ext = nl + K, nparts = ps_.num_parts(nl);
    for (uint32_t b = 0; b < n1; ++b)
        if (!galois_valid(h_gb[b], ps_.log_n)) throw std::invalid_argument("Galois element must be odd and below 2N");
    for (uint32_t t = 0; t < n2; ++t)
        if (!galois_valid(h_gg[t], ps_.log_n)) throw std::invalid_argument("Galois element must be odd and below 2N");
    if (nparts > 6) throw std::invalid_argument("more than 6 key-switch digits unsupported");
    if (!n_ct) return;
    // the compacted plan
    std::vector<uint32_t> babies, giants;
    for (uint32_t b = 0; b < n1; ++b)
        for (uint32_t t = 0; t < n2; ++t)
            if (h_present[(size_t)t * n1 + b]) {
                babies.push_back(b);
                break;
            }
    for (int keyed = 1; keyed >= 0; --keyed)
        for (uint32_t t = 0; t < n2; ++t) {
            if ((h_gg[t] != 1u) != (keyed == 1)) continue;
            for (uint32_t b = 0; b < n1; ++b)
                if (h_present[(size_t)t * n1 + b]) {
                    giants.push_back(t);
                    break;
                }
        }
    if (babies.empty()) return;
    const uint32_t n1c = (uint32_t)babies.size(), n2c = (uint32_t)giants.size();
    uint32_t nk = 0;
    for (uint32_t t : giants) nk += h_gg[t] != 1u;
    // device copy of the plan: bg[n1c] bk[n1c] gg[n2c] gk[n2c] ptidx[n2c][n1c]
    std::vector<uint32_t> meta;
    for (uint32_t b : babies) meta.push_back(h_gb[b]);
    for (uint32_t b : babies) meta.push_back(b);
    for (uint32_t t : giants) meta.push_back(h_gg[t]);
    for (uint32_t t : giants) meta.push_back(t);
    for (uint32_t t : giants)
        for (uint32_t b : babies) meta.push_back(h_present[(size_t)t * n1 + b] ? t * n1 + b : BSGS_ABSENT);
    if (meta.size() > lt_g_cap_) {
        MK_HIP(hipStreamSynchronize(stream_));
        if (d_lt_g_) MK_HIP(hipFree(d_lt_g_));
        d_lt_g_ = nullptr;
        lt_g_cap_ = 0;
        MK_HIP(hipMalloc(&d_lt_g_, meta.size() * sizeof(uint32_t)));
        lt_g_cap_ = meta.size();
    }
    MK_HIP(hipMemcpyAsync(d_lt_g_, meta.data(), meta.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
    MK_HIP(hipStreamSynchronize(stream_));
    const uint32_t *d_bg = d_lt_g_, *d_bk = d_bg + n1c, *d_gg = d_bk + n1c, *d_gk = d_gg + n2c, *d_ptidx = d_gk + n2c;
    std::vector<u64> pm(nl);
    for (uint32_t i = 0; i < nl; ++i) pm[i] = ps_.p_mod(i);
    const u64 *pmod = limb_vector("pmod_" + std::to_string(nl), pm);

    const uint32_t log_t = std::min(ps_.log_n, LT_LOG_TILE);
    const size_t ct_words = (size_t)2 * nl * n, qw = (size_t)nl * n, ew = (size_t)ext * n, kw = (size_t)K * n;
    const uint32_t nmd = std::max(nk, 2u);  // polynomials per ciphertext of the larger ModDown
    // words per ciphertext: c1's coefficients and digits, the babies, the inner sums, per keyed giant v_t, its coefficients
    // and its digits, the accumulators, the scratch of the larger ModDown
    // (the composition arm: a ciphertext (0, v_t), one key-switched giant and one permuted Ub_t more)
    const bool fused = knobs_.bsgs_fused != 0;
    const size_t w_comp = fused ? 0 : 2 * qw + 3 * ew;
    const size_t per_ct = qw + nparts * ew + (size_t)n1c * 2 * ew + (size_t)n2c * 2 * ew + (size_t)nk * (2 * qw + nparts * ew) +
                          2 * ew + (size_t)nmd * (kw + qw) + w_comp;
    const size_t cap_words = (size_t)knobs_.bsgs_ws_mib * (1u << 20) / sizeof(u64);
    const uint32_t chunk = (uint32_t)std::min<size_t>(std::min(knobs_.chunk, n_ct), std::max<size_t>(1, cap_words / per_ct));
    u64 *ws = workspace(per_ct * chunk);
    u64 *coef = ws, *dig = coef + chunk * qw, *bab = dig + (size_t)chunk * nparts * ew, *ub = bab + (size_t)chunk * n1c * 2 * ew;
    u64 *ua = ub + (size_t)chunk * n2c * ew, *v = ua + (size_t)chunk * n2c * ew, *coef2 = v + (size_t)chunk * nk * qw;
    u64 *dig2 = coef2 + (size_t)chunk * nk * qw, *til = dig2 + (size_t)chunk * nk * nparts * ew, *pc = til + (size_t)chunk * 2 * ew;
    u64 *conv = pc + (size_t)chunk * nmd * kw, *ctg = conv + (size_t)chunk * nmd * qw, *tmp_t = ctg + (size_t)chunk * 2 * qw;
    u64 *tmp_u = tmp_t + (size_t)chunk * 2 * ew;
    const size_t evk_words = (size_t)ps_.beta * 2 * ps_.D * n;
    const u64 *ones = fused ? nullptr : limb_vector("ones_" + std::to_string(ext), std::vector<u64>(ew, 1));
    for (uint32_t done = 0; done < n_ct; done += chunk) {
        const uint32_t cnt = std::min(chunk, n_ct - done);
        const u64 *c = ct + done * ct_words;
        modup_core(c + qw, ct_words, coef, dig, cnt, nl);
        const uint32_t groups = ext << (ps_.log_n - log_t);
        if (!fused) {
            // MKCKKS_BSGS_FUSED=0: the same sums from the kernels the direct transform has.  k_lt_accum with ONE rotation
            // and an all-ones plaintext is a baby (and the key-switched part of a giant, on the ciphertext (0, v_t));
            // k_fma multiplies and adds over the extended basis; k_automorph permutes Ub_t.  Every step stores canonical
            // residues of exact sums, so the bits are those of the fused kernels.  Layouts: babies [n1c][cnt][2][ext][N].
            const EwGeom eg{n, nl, ps_.L};
            const Opnd none{nullptr, 0, 0}, one{ones, 0, 0};
            auto accum1 = [&](const u64 *cts, const u64 *digs, const u64 *key, const uint32_t *d_g, u64 *dst) {
                LtArgs a{cts, digs, key, ones, d_g, pmod, dst, evk_words, 1, cnt, nl, ext, ps_.L, ps_.D, ps_.alpha, ps_.log_n, log_t,
                         groups, cnt, 0u, 1u};
                const uint64_t blocks = (uint64_t)((groups + LT_XCDS - 1) / LT_XCDS * LT_XCDS) * cnt;
                if (blocks > 0x7fffffffu) throw std::invalid_argument("batch too large for one launch");
                dispatch<1, 2, 3, 4, 5, 6>(nparts, [&](auto np) {
                    k_lt_accum<decltype(np)::value><<<dim3((unsigned)blocks), LT_THREADS, 0, stream_>>>(a, d_limb_);
                });
                MK_HIP(hipGetLastError());
            };
            // out = x y + z (+ w) over `polys` polynomials of ext slots
            auto fma = [&](Opnd x, Opnd y, Opnd z, Opnd w, u64 *o, size_t o_stride, uint32_t polys) {
                k_fma<<<ew_grid(n, ext, polys), EW_THREADS, 0, stream_>>>(x, y, z, w, nullptr, 0, o, o_stride, 0, eg, d_limb_, ext);
                MK_HIP(hipGetLastError());
            };
            for (uint32_t b = 0; b < n1c; ++b)
                accum1(c, dig, h_gb[babies[b]] != 1u ? bkeys + (size_t)babies[b] * evk_words : nullptr, d_bg + b,
                       bab + (size_t)b * cnt * 2 * ew);
            for (uint32_t t = 0; t < n2c; ++t) {
                bool first = true;
                for (uint32_t b = 0; b < n1c; ++b) {
                    const uint32_t idx = meta[2 * n1c + 2 * n2c + (size_t)t * n1c + b];
                    if (idx == BSGS_ABSENT) continue;
                    const Opnd pt{pts + (size_t)idx * ew, 0, 0};
                    for (uint32_t k = 0; k < 2; ++k) {
                        u64 *u = (k ? ua : ub) + (size_t)t * cnt * ew;
                        fma(Opnd{bab + ((size_t)b * cnt * 2 + k) * ew, 2 * ew, 0}, pt, first ? none : Opnd{u, ew, 0}, none, u, ew, cnt);
                    }
                    first = false;
                }
            }
            if (nk) {
                moddown_core(ua, pc, conv, v, qw, nullptr, 0, nk * cnt, nl, false);
                modup_core(v, qw, coef2, dig2, nk * cnt, nl);
                MK_HIP(hipMemsetAsync(ctg, 0, (size_t)cnt * 2 * qw * sizeof(u64), stream_));
            }
            for (uint32_t t = 0; t < n2c; ++t) {
                const u64 *ubt = ub + (size_t)t * cnt * ew, *uat = ua + (size_t)t * cnt * ew;
                const Opnd zb = t ? Opnd{til, 2 * ew, 0} : none, za = t ? Opnd{til + ew, 2 * ew, 0} : none;
                if (t < nk) {
                    k_copy_slots<<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(v + (size_t)t * cnt * qw, qw, 0, ctg + qw, 2 * qw, 0, n);
                    MK_HIP(hipGetLastError());
                    accum1(ctg, dig2 + (size_t)t * cnt * nparts * ew, gkeys + (size_t)giants[t] * evk_words, d_gg + t, tmp_t);
                    launch_automorph(ubt, tmp_u, (size_t)cnt * ext, h_gg[giants[t]]);
                    fma(Opnd{tmp_t, 2 * ew, 0}, one, zb, Opnd{tmp_u, ew, 0}, til, 2 * ew, cnt);
                    fma(Opnd{tmp_t + ew, 2 * ew, 0}, one, za, none, til + ew, 2 * ew, cnt);
                } else {
                    fma(Opnd{ubt, ew, 0}, one, zb, none, til, 2 * ew, cnt);
                    fma(Opnd{uat, ew, 0}, one, za, none, til + ew, 2 * ew, cnt);
                }
            }
            moddown_core(til, pc, conv, out + done * ct_words, qw, nullptr, 0, 2 * cnt, nl, false);
            continue;
        }
        BsgsArgs a{};
        a.ct = c; a.dig = dig; a.evks = bkeys; a.pts = nullptr; a.g = d_bg; a.pmod = pmod; a.til = bab;
        a.evk_words = evk_words;
        a.n_rot = n1c; a.cnt = cnt; a.nl = nl; a.ext = ext; a.L = ps_.L; a.D = ps_.D; a.alpha = ps_.alpha;
        a.log_n = ps_.log_n; a.log_t = log_t; a.groups = groups; a.members = cnt; a.walk = 0; a.xcd_order = 1;
        a.kidx = d_bk;
        const uint64_t blocks = (uint64_t)((groups + LT_XCDS - 1) / LT_XCDS * LT_XCDS) * cnt;
        if (blocks > 0x7fffffffu) throw std::invalid_argument("batch too large for one launch");
        dispatch<1, 2, 3, 4, 5, 6>(nparts, [&](auto np) {
            k_bsgs_baby<decltype(np)::value><<<dim3((unsigned)blocks), LT_THREADS, 0, stream_>>>(a, d_limb_);
        });
        MK_HIP(hipGetLastError());
        BsgsInnerArgs in{bab, pts, d_ptidx, ub, ua, n1c, n2c, cnt, nl, ext, ps_.L, ps_.log_n, log_t, groups, cnt, 1u};
        k_bsgs_inner<<<dim3((unsigned)blocks), LT_THREADS, 0, stream_>>>(in, d_limb_);
        MK_HIP(hipGetLastError());
        if (nk) {  // the keyed giants are giants [0, nk): Ua_t of all of them, one batch
            moddown_core(ua, pc, conv, v, qw, nullptr, 0, nk * cnt, nl, false);
            modup_core(v, qw, coef2, dig2, nk * cnt, nl);
        }
        BsgsArgs gi = a;
        gi.ct = nullptr; gi.dig = dig2; gi.evks = gkeys; gi.g = d_gg; gi.til = til; gi.n_rot = nk; gi.kidx = d_gk;
        gi.v = v; gi.ub = ub; gi.ua = ua; gi.n_all = n2c;
        dispatch<1, 2, 3, 4, 5, 6>(nparts, [&](auto np) {
            k_bsgs_giant<decltype(np)::value><<<dim3((unsigned)blocks), LT_THREADS, 0, stream_>>>(gi, d_limb_);
        });
        MK_HIP(hipGetLastError());
        moddown_core(til, pc, conv, out + done * ct_words, qw, nullptr, 0, 2 * cnt, nl, false);
    }
}

// ---- ciphertext products ("ciphertext products"); overlaps and alignment are refused in capi.cpp ------------

// the relinearisation key: the re-encryption key from s^2 to s, i.e. rekeygen with NTT(s_old) replaced by NTT(s)^2
void Engine::relin_keygen(const int8_t *s, const u64 *pk, const int8_t *u, const int32_t *e0, const int32_t *e1, u64 *evk) {
    need_device();
    const uint32_t n = ps_.n, D = ps_.D, L = ps_.L;
    u64 *se = rekey_workspace();
    EwGeom g{n, L, L};
    k_lift<int8_t><<<ew_grid(n, D, 1), EW_THREADS, 0, stream_>>>(s, se, g, d_limb_, D);
    MK_HIP(hipGetLastError());
    ntt_launch(se, 1, L, D, false, nullptr, nullptr);
    Opnd x{se, 0, 0}, none{nullptr, 0, 0};
    k_fma<<<ew_grid(n, D, 1), EW_THREADS, 0, stream_>>>(x, x, none, none, nullptr, 0, se, 0, 0, g, d_limb_, D);
    MK_HIP(hipGetLastError());
    rekeygen_from(pk, u, e0, e1, evk);
}

// one k_tensor launch over `cnt` items; a == b takes the square instance
void Engine::launch_tensor(const u64 *a, const u64 *b, size_t term_stride, uint32_t n_terms, u64 *o01, size_t o01_stride,
                           u64 *o2, size_t o2_stride, uint32_t cnt, uint32_t nl) {
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)o01 | (uintptr_t)o2) & 15)
        throw std::invalid_argument("ciphertext arrays must be 16-byte aligned");
    if (!cnt) return;
    const TensorArgs t{a, b, o01, o2, term_stride, o01_stride, o2_stride, n_terms, ps_.n, nl};
    const dim3 grid((ps_.n / 2 + TENSOR_THREADS - 1) / TENSOR_THREADS, nl, cnt);
    if (a == b) k_tensor<true><<<grid, TENSOR_THREADS, 0, stream_>>>(t, d_limb_);
    else k_tensor<false><<<grid, TENSOR_THREADS, 0, stream_>>>(t, d_limb_);
    MK_HIP(hipGetLastError());
}

void Engine::tensor_sum(const u64 *a, const u64 *b, u64 *out3, uint32_t n_terms, uint32_t n_ct, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!n_terms) throw std::invalid_argument("n_terms must be at least 1");
    const size_t poly = (size_t)nl * ps_.n;
    constexpr uint32_t MAX_ITEMS = 32768;  // grid.z
    for (uint32_t done = 0; done < n_ct; done += MAX_ITEMS) {
        const uint32_t cnt = std::min(MAX_ITEMS, n_ct - done);
        const size_t in_off = (size_t)done * 2 * poly, out_off = (size_t)done * 3 * poly;
        launch_tensor(a + in_off, b + in_off, (size_t)n_ct * 2 * poly, n_terms, out3 + out_off, 3 * poly,
                      out3 + out_off + 2 * poly, 3 * poly, cnt, nl);
    }
}

// out[item] += KeySwitch(d2[item], rlk) for `cnt` items, d2 items d2_stride words apart: the hybrid key switch of
// reencrypt_chunk with d2 in the place of c1 and nothing in the place of c0; the accumulating tail adds onto (d0, d1)
void Engine::relin_chunk(const u64 *d2, size_t d2_stride, const u64 *rlk, u64 *out, uint32_t cnt, uint32_t nl) {
    const uint32_t n = ps_.n, K = ps_.K, ext = nl + K, nparts = ps_.num_parts(nl);
    const size_t w_coef = (size_t)cnt * nl * n, w_dig = (size_t)cnt * nparts * ext * n;
    const size_t w_til = (size_t)cnt * 2 * ext * n, w_pc = (size_t)cnt * 2 * K * n, w_conv = (size_t)cnt * 2 * nl * n;
    u64 *ws = workspace(w_coef + w_dig + w_til + w_pc + w_conv);
    u64 *coef = ws, *dig = coef + w_coef, *til = dig + w_dig, *pc = til + w_til, *conv = pc + w_pc;
    const bool p_rows = keyswitch_digits(d2, d2_stride, rlk, coef, dig, til, pc, cnt, nl);
    moddown_core(til, pc, conv, out, (size_t)nl * n, nullptr, 0, 2 * cnt, nl, true, p_rows);
}

void Engine::relinearize(const u64 *in3, const u64 *rlk, u64 *out, uint32_t n_ct, uint32_t nl) {
    need_device();
    check_nl(nl);
    const uint32_t n = ps_.n;
    const size_t poly = (size_t)nl * n;
    for (uint32_t done = 0; done < n_ct; done += knobs_.chunk) {
        const uint32_t cnt = std::min(knobs_.chunk, n_ct - done);
        const u64 *src = in3 + (size_t)done * 3 * poly;
        u64 *dst = out + (size_t)done * 2 * poly;
        k_copy_slots<<<ew_grid(n, 2 * nl, cnt), EW_THREADS, 0, stream_>>>(src, 3 * poly, 0, dst, 2 * poly, 0, n);
        MK_HIP(hipGetLastError());
        relin_chunk(src + 2 * poly, 3 * poly, rlk, dst, cnt, nl);
    }
}

// per chunk: k_tensor writes d0, d1 straight into `out` (which may be a or b: it touches a thread's own words only) and
// d2 into the chunk buffer, the only place it ever exists; the key switch of d2 accumulates onto out
void Engine::mult_relin(const u64 *a, const u64 *b, const u64 *rlk, u64 *out, uint32_t n_ct, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!n_ct) return;
    const size_t poly = (size_t)nl * ps_.n;
    const uint32_t chunk = std::min(knobs_.chunk, n_ct);
    u64 *d2 = chunk_buffer((size_t)chunk * poly);
    for (uint32_t done = 0; done < n_ct; done += chunk) {
        const uint32_t cnt = std::min(chunk, n_ct - done);
        const size_t off = (size_t)done * 2 * poly;
        u64 *dst = out + off;
        launch_tensor(a + off, b + off, 0, 1, dst, 2 * poly, d2, poly, cnt, nl);
        relin_chunk(d2, poly, rlk, dst, cnt, nl);
    }
}

// ---- polynomial evaluation ("polynomial evaluation"); overlaps and alignment are refused in capi.cpp -----------

// the composition's constant column and closing row (MKCKKS_POLY_FUSED=0 only)
// ct[item][0][l] += f[l]: the constant M_{j,0} enters component 0 of Q_j, i.e. Q_j + M_{j,0} (1, 0)
__global__ void k_poly_add_const(u64 *ct, EwGeom g, const LimbConst *limb, const u64 *f) {
    EW_PROLOGUE(g.nl)
    const u64 q = limb[slot].q, c = f[slot];
    const size_t off = ((size_t)item * 2 * g.nl + slot) * g.n + idx;
    ulong2 v = ld2(ct + off);
    v.x = add_mod(v.x, c, q);
    v.y = add_mod(v.y, c, q);
    st2(ct + off, v);
}
// out3[item][c][l] += q0[item][c][l] for c < 2: (Q'_0, 0) onto the tensor sum; grid.y = 2 * nl
__global__ void k_poly_add_row(u64 *out3, const u64 *q0, EwGeom g, const LimbConst *limb) {
    EW_PROLOGUE(2 * g.nl)
    const u64 q = limb[slot % g.nl].q;
    const size_t in = ((size_t)item * 2 * g.nl + slot) * g.n + idx, out = ((size_t)item * 3 * g.nl + slot) * g.n + idx;
    ulong2 v = ld2(out3 + out);
    const ulong2 a = ld2(q0 + in);
    v.x = add_mod(v.x, a.x, q);
    v.y = add_mod(v.y, a.y, q);
    st2(out3 + out, v);
}

// Device table of a call's constants, cached per (weights, B, G, nl_T) like weight_table and in the same cache:
// M u64[G][B][nl_T] (k_poly_tensor), then the same constants as weight-table entries [G][B][nl_T][WT_WORDS] (k_wsum_ct of
// the composition reads M and its Shoup companion)
const u64 *Engine::poly_table(const double *w, uint32_t B, uint32_t G, uint32_t nl_T) {
    std::string key((const char *)w, (size_t)B * G * sizeof(double));
    key += "@poly" + std::to_string(B) + "," + std::to_string(G) + "," + std::to_string(nl_T);
    auto it = wt_cache_.find(key);
    if (it != wt_cache_.end()) return it->second;
    const std::vector<u64> m = ps_.poly_constants(w, B * G, nl_T);  // throws on a weight that does not fit
    std::vector<u64> t(m.size() * (1 + WT_WORDS), 0);
    std::copy(m.begin(), m.end(), t.begin());
    for (size_t e = 0; e < m.size(); ++e) {
        u64 *wt = &t[m.size() + e * WT_WORDS];
        wt[0] = m[e];
        wt[1] = h_shoup(m[e], ps_.moduli[e % nl_T]);
    }
    return cache_table(key, t);
}

// words of scratch poly_tensor_core needs: none for the kernel; the composition packs the operands' prefixes and keeps
// every Q_j
size_t Engine::poly_tensor_scratch(uint32_t B, uint32_t G, uint32_t cnt, uint32_t nl_T) const {
    if (poly_tensor_fused(B, G, knobs_.poly_fused)) return 0;
    return (size_t)(B - 1 + G - 1 + G) * cnt * 2 * nl_T * ps_.n;
}

void Engine::poly_tensor_core(const PolyOpnd *baby, const PolyOpnd *giant, const u64 *table, u64 *out3, uint32_t B, uint32_t G,
                              uint32_t cnt, uint32_t nl_T, u64 *scratch) {
    const uint32_t n = ps_.n;
    if (!cnt) return;
    if (poly_tensor_fused(B, G, knobs_.poly_fused)) {
        PolyArgs t{};
        for (uint32_t i = 0; i + 1 < B; ++i) t.baby[i] = baby[i];
        for (uint32_t j = 0; j + 1 < G; ++j) t.giant[j] = giant[j];
        t.m = table;
        t.out3 = out3;
        t.G = G;
        t.n = n;
        t.nl_T = nl_T;
        const dim3 grid((n / 2 + POLY_THREADS - 1) / POLY_THREADS, nl_T, cnt);
        if (!dispatch<2, 4, 8>(B, [&](auto b) {
                k_poly_tensor<decltype(b)::value><<<grid, POLY_THREADS, 0, stream_>>>(t, d_limb_);
            }))
            throw std::invalid_argument("B must be 2, 4 or 8");
        MK_HIP(hipGetLastError());
        return;
    }
    // the composition: packed prefix copies, eval_wsum's kernel per giant index, the constant column, tensor_sum's kernel
    // over the giants, the closing row
    const size_t poly = (size_t)nl_T * n, term = (size_t)cnt * 2 * poly;
    u64 *bp = scratch, *gp = bp + (B - 1) * term, *qs = gp + (G - 1) * term;  // qs[0] = Q'_0, qs[j] = Q'_j
    for (uint32_t i = 0; i + 1 < B; ++i)
        k_copy_slots<<<ew_grid(n, nl_T, 2 * cnt), EW_THREADS, 0, stream_>>>(baby[i].p, (size_t)baby[i].nl * n, 0, bp + i * term,
                                                                             poly, 0, n);
    for (uint32_t j = 0; j + 1 < G; ++j)
        k_copy_slots<<<ew_grid(n, nl_T, 2 * cnt), EW_THREADS, 0, stream_>>>(giant[j].p, (size_t)giant[j].nl * n, 0,
                                                                             gp + j * term, poly, 0, n);
    MK_HIP(hipGetLastError());
    const size_t m_words = (size_t)G * B * nl_T;
    EwGeom g{n, nl_T, ps_.L};
    for (uint32_t j = 0; j < G; ++j) {
        const u64 *wt = table + m_words + ((size_t)j * B + 1) * nl_T * WT_WORDS;  // terms i = 1 .. B - 1 of row j
        k_wsum_ct<<<ew_grid(n, 2 * nl_T, cnt), EW_THREADS, 0, stream_>>>(bp, qs + j * term, g, d_limb_, 2 * nl_T, B - 1, term, wt,
                                                                          nl_T, 0);
        k_poly_add_const<<<ew_grid(n, nl_T, cnt), EW_THREADS, 0, stream_>>>(qs + j * term, g, d_limb_,
                                                                             table + (size_t)j * B * nl_T);
    }
    MK_HIP(hipGetLastError());
    launch_tensor(qs + term, gp, term, G - 1, out3, 3 * poly, out3 + 2 * poly, 3 * poly, cnt, nl_T);
    k_poly_add_row<<<ew_grid(n, 2 * nl_T, cnt), EW_THREADS, 0, stream_>>>(out3, qs, g, d_limb_);
    MK_HIP(hipGetLastError());
}

void Engine::poly_tensor(const u64 *baby, const uint32_t *baby_nl, const u64 *giant, const uint32_t *giant_nl, const double *w,
                         u64 *out3, uint32_t B, uint32_t G, uint32_t n_ct, uint32_t nl_T) {
    need_device();
    check_nl(nl_T);
    if (!n_ct) return;
    const uint32_t n = ps_.n;
    const u64 *table = poly_table(w, B, G, nl_T);
    constexpr uint32_t MAX_ITEMS = 32768;  // grid.z
    const uint32_t step = std::min(n_ct, MAX_ITEMS);
    const size_t scratch_words = poly_tensor_scratch(B, G, step, nl_T);
    u64 *scratch = scratch_words ? poly_buffer(scratch_words) : nullptr;
    for (uint32_t done = 0; done < n_ct; done += step) {
        const uint32_t cnt = std::min(step, n_ct - done);
        PolyOpnd bo[POLY_MAX_B - 1] = {}, go[POLY_MAX_B - 1] = {};
        size_t off = 0;  // power k of a packed array starts behind the n_ct items of power k - 1
        for (uint32_t i = 0; i + 1 < B; ++i) {
            bo[i] = PolyOpnd{baby + off + (size_t)done * 2 * baby_nl[i] * n, baby_nl[i], 0};
            off += (size_t)n_ct * 2 * baby_nl[i] * n;
        }
        off = 0;
        for (uint32_t j = 0; j + 1 < G; ++j) {
            go[j] = PolyOpnd{giant + off + (size_t)done * 2 * giant_nl[j] * n, giant_nl[j], 0};
            off += (size_t)n_ct * 2 * giant_nl[j] * n;
        }
        poly_tensor_core(bo, go, table, out3 + (size_t)done * 3 * nl_T * n, B, G, cnt, nl_T, scratch);
    }
}

void Engine::power_ladder_core(u64 *const *pw, const uint32_t *nlk, const u64 *rlk, uint32_t cnt, uint32_t n_pow, u64 *scratch) {
    const uint32_t n = ps_.n;
    u64 *pre = scratch, *prod = scratch + (size_t)cnt * 2 * nlk[1] * n;
    for (uint32_t k = 2; k <= n_pow; ++k) {
        const uint32_t i = (k + 1) / 2, j = k - i, nli = nlk[i];
        const u64 *b = pw[j];
        if (nlk[j] != nli) {  // the level cut: the first nl_i limbs of both components, packed
            k_copy_slots<<<ew_grid(n, nli, 2 * cnt), EW_THREADS, 0, stream_>>>(pw[j], (size_t)nlk[j] * n, 0, pre, (size_t)nli * n, 0,
                                                                             n);
            MK_HIP(hipGetLastError());
            b = pre;
        }
        mult_relin(pw[i], b, rlk, prod, cnt, nli);
        rescale(prod, pw[k], cnt, nli, nullptr);
    }
}

void Engine::powers(const u64 *z, const u64 *rlk, u64 *out, uint32_t n_ct, uint32_t nl, uint32_t n_pow) {
    need_device();
    check_nl(nl);
    std::vector<uint32_t> nlk(n_pow + 1);
    ps_.power_ladder(nl, n_pow, 1.0, nlk.data() + 1, nullptr);
    if (!n_ct) return;
    const uint32_t n = ps_.n;
    MK_HIP(hipMemcpyAsync(out, z, (size_t)n_ct * 2 * nl * n * sizeof(u64), hipMemcpyDeviceToDevice, stream_));
    if (n_pow < 2) return;
    const uint32_t chunk = std::min(knobs_.chunk, n_ct);
    u64 *scratch = poly_buffer((size_t)2 * chunk * 2 * nl * n);
    std::vector<size_t> off(n_pow + 1, 0);
    for (uint32_t k = 2; k <= n_pow; ++k) off[k] = off[k - 1] + (size_t)n_ct * 2 * nlk[k - 1] * n;
    std::vector<u64 *> pw(n_pow + 1, nullptr);
    for (uint32_t done = 0; done < n_ct; done += chunk) {
        const uint32_t cnt = std::min(chunk, n_ct - done);
        for (uint32_t k = 1; k <= n_pow; ++k) pw[k] = out + off[k] + (size_t)done * 2 * nlk[k] * n;
        power_ladder_core(pw.data(), nlk.data(), rlk, cnt, n_pow, scratch);
    }
}

// per chunk, everything but the input and the output in the poly buffer: x^2 .. x^B (= y), y^2 .. y^(G-1), the ladder's
// scratch, the outer sum, its relinearisation and the first rescale.  x^1 is the input where it is
void Engine::poly_eval(const u64 *ct, const u64 *rlk, const double *coef, uint32_t degree, u64 *out, uint32_t n_ct, uint32_t nl,
                       double scale_in) {
    need_device();
    const PolyPlan p = ps_.poly_plan(degree, nl);
    std::vector<double> w((size_t)p.B * p.G);
    ps_.poly_weights(coef, degree, nl, scale_in, w.data());
    if (!n_ct) return;
    const uint32_t n = ps_.n, B = p.B, G = p.G, nl_T = p.nl_T;
    uint32_t nlx[POLY_MAX_B + 1] = {}, nly[POLY_MAX_B] = {};
    ps_.power_ladder(nl, B, 1.0, nlx + 1, nullptr);
    ps_.power_ladder(nlx[B], G - 1, 1.0, nly + 1, nullptr);
    const u64 *table = poly_table(w.data(), B, G, nl_T);
    const uint32_t chunk = std::min(knobs_.chunk, n_ct);
    const size_t ctw = (size_t)chunk * 2 * n;  // words of a chunk's ciphertexts per limb
    size_t words = 0, off_x[POLY_MAX_B + 1] = {}, off_y[POLY_MAX_B] = {};
    for (uint32_t k = 2; k <= B; ++k) {
        off_x[k] = words;
        words += ctw * nlx[k];
    }
    for (uint32_t k = 2; k < G; ++k) {
        off_y[k] = words;
        words += ctw * nly[k];
    }
    const size_t off_ladder = words;
    words += 2 * ctw * nl;
    const size_t off_out3 = words;
    words += (size_t)chunk * 3 * nl_T * n;
    const size_t off_relin = words;
    words += ctw * nl_T;
    const size_t off_resc = words;
    words += ctw * (nl_T - 1);
    const size_t off_comp = words;
    words += poly_tensor_scratch(B, G, chunk, nl_T);
    u64 *buf = poly_buffer(words);
    for (uint32_t done = 0; done < n_ct; done += chunk) {
        const uint32_t cnt = std::min(chunk, n_ct - done);
        u64 *pwx[POLY_MAX_B + 1] = {}, *pwy[POLY_MAX_B] = {};
        pwx[1] = const_cast<u64 *>(ct) + (size_t)done * 2 * nl * n;  // read only: the ladder writes pw[k] for k >= 2
        for (uint32_t k = 2; k <= B; ++k) pwx[k] = buf + off_x[k];
        power_ladder_core(pwx, nlx, rlk, cnt, B, buf + off_ladder);
        pwy[1] = pwx[B];
        for (uint32_t k = 2; k < G; ++k) pwy[k] = buf + off_y[k];
        power_ladder_core(pwy, nly, rlk, cnt, G - 1, buf + off_ladder);
        PolyOpnd bo[POLY_MAX_B - 1] = {}, go[POLY_MAX_B - 1] = {};
        for (uint32_t i = 1; i < B; ++i) bo[i - 1] = PolyOpnd{pwx[i], nlx[i], 0};
        for (uint32_t j = 1; j < G; ++j) go[j - 1] = PolyOpnd{pwy[j], nly[j], 0};
        poly_tensor_core(bo, go, table, buf + off_out3, B, G, cnt, nl_T, buf + off_comp);
        relinearize(buf + off_out3, rlk, buf + off_relin, cnt, nl_T);
        rescale(buf + off_relin, buf + off_resc, cnt, nl_T, nullptr);
        rescale(buf + off_resc, out + (size_t)done * 2 * p.nl_out * n, cnt, nl_T - 1, nullptr);
    }
}

// ---- Chebyshev series ("Chebyshev series"); overlaps and alignment are refused in capi.cpp ---------------------

// A new entry of the weight-table cache, uploaded: the one place where the cache grows and is emptied (weight_table,
// poly_table, cheb_table and affine_core all end here).  At 64 tables it is emptied: the stream is waited for, so work
// already enqueued keeps its tables, and EVERY entry is freed.  So no table pointer may be held across another lookup:
// look a table up immediately before the launch that reads it, after every other lookup the call makes.
const u64 *Engine::cache_table(const std::string &key, const std::vector<u64> &t) {
    if (wt_cache_.size() >= 64) {
        MK_HIP(hipStreamSynchronize(stream_));
        for (auto &kv : wt_cache_) MK_HIP(hipFree(kv.second));
        wt_cache_.clear();
    }
    u64 *d = nullptr;
    MK_HIP(hipMalloc(&d, t.size() * sizeof(u64)));
    wt_cache_[key] = d;
    MK_HIP(hipMemcpy(d, t.data(), t.size() * sizeof(u64), hipMemcpyHostToDevice));
    return d;
}

// Device table of a step's weight, cached per (weight, nl) in the weight-table cache: M' u64[nl] with M' = (q - M mod q)
// mod q (k_cheb_tensor, k_poly_add_const), then the composition's two weight-table entries [2][nl][WT_WORDS]: 2 and M'
const u64 *Engine::cheb_table(double w, uint32_t nl) {
    std::string key((const char *)&w, sizeof(double));
    key += "@cheb" + std::to_string(nl);
    auto it = wt_cache_.find(key);
    if (it != wt_cache_.end()) return it->second;
    const std::vector<u64> m = ps_.poly_constants(&w, 1, nl);  // throws on a weight that does not fit
    std::vector<u64> t((size_t)nl * (1 + 2 * WT_WORDS), 0);
    for (uint32_t l = 0; l < nl; ++l) {
        const u64 q = ps_.moduli[l], neg = m[l] ? q - m[l] : 0;
        t[l] = neg;
        u64 *two = &t[nl + (size_t)l * WT_WORDS], *term = &t[nl + ((size_t)nl + l) * WT_WORDS];
        two[0] = 2;
        two[1] = h_shoup(2, q);
        term[0] = neg;
        term[1] = h_shoup(neg, q);
    }
    return cache_table(key, t);
}

// words of scratch cheb_step_core needs: none for the kernel; the composition packs the prefixes of a and b and keeps the
// tensor product and the packed term side by side (the two terms of k_wsum_ct)
size_t Engine::cheb_step_scratch(uint32_t cnt, uint32_t nl) const {
    if (knobs_.cheb_fused != 0) return 0;
    return (size_t)4 * cnt * 2 * nl * ps_.n;
}

// (d0, d1) -> o01, d2 -> o2 for `cnt` items.  The composition writes packed items: o01_stride = 2 * nl * N, o2_stride = nl * N
void Engine::cheb_step_core(const u64 *a, uint32_t nl_a, const u64 *b, uint32_t nl_b, const u64 *t, uint32_t nl_t,
                            const u64 *table, u64 *o01, size_t o01_stride, u64 *o2, size_t o2_stride, uint32_t cnt, uint32_t nl,
                            u64 *scratch) {
    const uint32_t n = ps_.n;
    if (!cnt) return;
    if (((uintptr_t)a | (uintptr_t)b | (uintptr_t)t | (uintptr_t)o01 | (uintptr_t)o2) & 15)
        throw std::invalid_argument("ciphertext arrays must be 16-byte aligned");
    const bool square = a == b;
    if (cheb_step_fused(square, t != nullptr, knobs_.cheb_fused)) {
        const ChebArgs c{a, b, t, table, o01, o2, o01_stride, o2_stride, nl_a, nl_b, t ? nl_t : nl, n, nl};
        const dim3 grid((n / 2 + CHEB_THREADS - 1) / CHEB_THREADS, nl, cnt);
        if (square && t) k_cheb_tensor<true, true><<<grid, CHEB_THREADS, 0, stream_>>>(c, d_limb_);
        else if (square) k_cheb_tensor<true, false><<<grid, CHEB_THREADS, 0, stream_>>>(c, d_limb_);
        else if (t) k_cheb_tensor<false, true><<<grid, CHEB_THREADS, 0, stream_>>>(c, d_limb_);
        else k_cheb_tensor<false, false><<<grid, CHEB_THREADS, 0, stream_>>>(c, d_limb_);
        MK_HIP(hipGetLastError());
        return;
    }
    // the composition, from kernels that were there before: packed prefix copies, k_tensor, then 2 * (d0, d1) + M' t by
    // k_wsum_ct (2 * (d0, d1) and M' onto d0 by k_poly_add_const for the constant), and 2 * d2 by k_wsum_ct in place
    const size_t poly = (size_t)nl * n, term = (size_t)cnt * 2 * poly;
    if (o01_stride != 2 * poly || o2_stride != poly) throw std::logic_error("cheb_step_core: the composition writes packed items");
    u64 *ap = scratch, *bp = ap + term, *s0 = bp + term;
    const u64 *pa = a, *pb = b;
    if (nl_a != nl) {
        k_copy_slots<<<ew_grid(n, nl, 2 * cnt), EW_THREADS, 0, stream_>>>(a, (size_t)nl_a * n, 0, ap, poly, 0, n);
        pa = ap;
    }
    if (square) {
        pb = pa;
    } else if (nl_b != nl) {
        k_copy_slots<<<ew_grid(n, nl, 2 * cnt), EW_THREADS, 0, stream_>>>(b, (size_t)nl_b * n, 0, bp, poly, 0, n);
        pb = bp;
    }
    MK_HIP(hipGetLastError());
    launch_tensor(pa, pb, 0, 1, s0, 2 * poly, o2, poly, cnt, nl);
    EwGeom g{n, nl, ps_.L};
    const u64 *wt = table + nl;
    if (t) {
        k_copy_slots<<<ew_grid(n, nl, 2 * cnt), EW_THREADS, 0, stream_>>>(t, (size_t)nl_t * n, 0, s0 + term, poly, 0, n);
        k_wsum_ct<<<ew_grid(n, 2 * nl, cnt), EW_THREADS, 0, stream_>>>(s0, o01, g, d_limb_, 2 * nl, 2, term, wt, nl, 0);
    } else {
        k_wsum_ct<<<ew_grid(n, 2 * nl, cnt), EW_THREADS, 0, stream_>>>(s0, o01, g, d_limb_, 2 * nl, 1, term, wt, nl, 0);
        k_poly_add_const<<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(o01, g, d_limb_, table);
    }
    k_wsum_ct<<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(o2, o2, g, d_limb_, nl, 1, 0, wt, nl, 0);
    MK_HIP(hipGetLastError());
}

void Engine::cheb_tensor(const u64 *a, uint32_t nl_a, const u64 *b, uint32_t nl_b, const u64 *t, uint32_t nl_t, double w,
                         u64 *out3, uint32_t n_ct, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!n_ct) return;
    const uint32_t n = ps_.n;
    const size_t poly = (size_t)nl * n;
    const u64 *table = cheb_table(w, nl);
    constexpr uint32_t MAX_ITEMS = 16384;  // grid.z, and twice as many polynomials in the composition's copies
    const uint32_t step = std::min(n_ct, MAX_ITEMS);
    const bool fused = cheb_step_fused(a == b, t != nullptr, knobs_.cheb_fused);
    // the composition writes packed (d0, d1) and d2: they pass through the poly buffer on their way to out3
    u64 *buf = fused ? nullptr : poly_buffer((size_t)step * 3 * poly + cheb_step_scratch(step, nl));
    for (uint32_t done = 0; done < n_ct; done += step) {
        const uint32_t cnt = std::min(step, n_ct - done);
        const u64 *pa = a + (size_t)done * 2 * nl_a * n, *pb = a == b ? pa : b + (size_t)done * 2 * nl_b * n;
        const u64 *pt = t ? t + (size_t)done * 2 * nl_t * n : nullptr;
        u64 *o = out3 + (size_t)done * 3 * poly;
        if (fused) {
            cheb_step_core(pa, nl_a, pb, nl_b, pt, nl_t, table, o, 3 * poly, o + 2 * poly, 3 * poly, cnt, nl, nullptr);
            continue;
        }
        u64 *p01 = buf, *p2 = buf + (size_t)step * 2 * poly;
        cheb_step_core(pa, nl_a, pb, nl_b, pt, nl_t, table, p01, 2 * poly, p2, poly, cnt, nl, buf + (size_t)step * 3 * poly);
        k_copy_slots<<<ew_grid(n, 2 * nl, cnt), EW_THREADS, 0, stream_>>>(p01, 2 * poly, 0, o, 3 * poly, 0, n);
        k_copy_slots<<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(p2, poly, 0, o, 3 * poly, 2 * nl, n);
        MK_HIP(hipGetLastError());
    }
}

void Engine::cheb_ladder_core(u64 *const *pw, const uint32_t *nlk, const double *sk, const u64 *rlk, uint32_t cnt, uint32_t n_cheb,
                              u64 *scratch) {
    const uint32_t n = ps_.n;
    if (n_cheb < 2) return;
    u64 *prod = scratch, *comp = scratch + (size_t)cnt * 2 * nlk[1] * n;
    u64 *d2 = chunk_buffer((size_t)cnt * nlk[1] * n);
    for (uint32_t k = 2; k <= n_cheb; ++k) {
        const uint32_t i = (k + 1) / 2, j = k - i, nli = nlk[i];
        const size_t poly = (size_t)nli * n;
        const bool term = i != j;  // T_{i-j} = T_1; else the constant T_0 = 1 with scale 1
        const double prod_s = sk[i] * sk[j];
        const double w = term ? prod_s / sk[1] : prod_s;
        cheb_step_core(pw[i], nli, pw[j], nlk[j], term ? pw[1] : nullptr, nlk[1], cheb_table(w, nli), prod, 2 * poly, d2, poly, cnt,
                       nli, comp);
        relin_chunk(d2, poly, rlk, prod, cnt, nli);
        rescale(prod, pw[k], cnt, nli, nullptr);
    }
}

void Engine::cheb_ladder(const u64 *u, const u64 *rlk, u64 *out, uint32_t n_ct, uint32_t nl, uint32_t n_cheb, double scale_in) {
    need_device();
    check_nl(nl);
    std::vector<uint32_t> nlk(n_cheb + 1);
    std::vector<double> sk(n_cheb + 1);
    ps_.power_ladder(nl, n_cheb, scale_in, nlk.data() + 1, sk.data() + 1);
    if (!n_ct) return;
    const uint32_t n = ps_.n;
    MK_HIP(hipMemcpyAsync(out, u, (size_t)n_ct * 2 * nl * n * sizeof(u64), hipMemcpyDeviceToDevice, stream_));
    if (n_cheb < 2) return;
    const uint32_t chunk = std::min(knobs_.chunk, n_ct);
    u64 *scratch = poly_buffer((size_t)chunk * 2 * nl * n + cheb_step_scratch(chunk, nl));
    std::vector<size_t> off(n_cheb + 1, 0);
    for (uint32_t k = 2; k <= n_cheb; ++k) off[k] = off[k - 1] + (size_t)n_ct * 2 * nlk[k - 1] * n;
    std::vector<u64 *> pw(n_cheb + 1, nullptr);
    for (uint32_t done = 0; done < n_ct; done += chunk) {
        const uint32_t cnt = std::min(chunk, n_ct - done);
        for (uint32_t k = 1; k <= n_cheb; ++k) pw[k] = out + off[k] + (size_t)done * 2 * nlk[k] * n;
        cheb_ladder_core(pw.data(), nlk.data(), sk.data(), rlk, cnt, n_cheb, scratch);
    }
}

// Device table of an affine map's constants, cached like a step's: Ma u64[nl], then Mc u64[nl]
void Engine::affine_core(const u64 *in, u64 *out, uint32_t cnt, uint32_t nl, double w_mul, double w_add) {
    if (!cnt) return;
    const double w[2] = {w_mul, w_add};
    std::string key((const char *)w, sizeof(w));
    key += "@affine" + std::to_string(nl);
    auto it = wt_cache_.find(key);
    // poly_constants throws on a weight that does not fit
    const u64 *table = it != wt_cache_.end() ? it->second : cache_table(key, ps_.poly_constants(w, 2, nl));
    const dim3 grid((ps_.n / 2 + CHEB_THREADS - 1) / CHEB_THREADS, 2 * nl, cnt);
    k_affine<<<grid, CHEB_THREADS, 0, stream_>>>(in, out, table, ps_.n, nl, d_limb_);
    MK_HIP(hipGetLastError());
}

void Engine::affine(const u64 *in, u64 *out, uint32_t n_ct, uint32_t nl, double w_mul, double w_add) {
    need_device();
    check_nl(nl);
    if (((uintptr_t)in | (uintptr_t)out) & 15) throw std::invalid_argument("ciphertext arrays must be 16-byte aligned");
    constexpr uint32_t MAX_ITEMS = 32768;  // grid.z
    for (uint32_t done = 0; done < n_ct; done += MAX_ITEMS) {
        const size_t off = (size_t)done * 2 * nl * ps_.n;
        affine_core(in + off, out + off, std::min(MAX_ITEMS, n_ct - done), nl, w_mul, w_add);
    }
}

// per chunk, everything but the input and the output in the poly buffer: the mapped input before and after its rescale,
// T_2 .. T_B of u, T_2 .. T_{G-1} of y = T_B, the ladder's scratch, the outer sum, its relinearisation and the first rescale
void Engine::cheb_eval(const u64 *ct, const u64 *rlk, const double *coef, uint32_t degree, double a, double b, u64 *out,
                       uint32_t n_ct, uint32_t nl, double scale_in) {
    need_device();
    check_nl(nl);
    const bool mapped = !(a == -1.0 && b == 1.0);
    if (mapped && nl < 2) throw std::invalid_argument("the map onto [-1, 1] needs 2 limbs, the input has 1");
    const uint32_t nl_u = mapped ? nl - 1 : nl;
    const double scale_u = mapped ? ps_.sf.at(ps_.L - nl_u) : scale_in;
    const PolyPlan p = ps_.poly_plan(degree, nl_u);
    std::vector<double> w((size_t)p.B * p.G);
    ps_.cheb_weights(coef, degree, nl_u, scale_u, w.data());
    double w_mul = 0.0, w_add = 0.0;
    if (mapped) {
        const double alpha = 2.0 / (b - a), beta = -(a + b) / (b - a);
        const double sigma1 = scale_u * (double)ps_.moduli[nl - 1];
        w_mul = alpha * (sigma1 / scale_in);
        w_add = beta * sigma1;
    }
    if (!n_ct) return;
    const uint32_t n = ps_.n, B = p.B, G = p.G, nl_T = p.nl_T;
    uint32_t nlx[POLY_MAX_B + 1] = {}, nly[POLY_MAX_B] = {};
    double sx[POLY_MAX_B + 1] = {}, sy[POLY_MAX_B] = {};
    ps_.power_ladder(nl_u, B, scale_u, nlx + 1, sx + 1);
    ps_.power_ladder(nlx[B], G - 1, sx[B], nly + 1, sy + 1);
    const uint32_t chunk = std::min(knobs_.chunk, n_ct);
    const size_t ctw = (size_t)chunk * 2 * n;  // words of a chunk's ciphertexts per limb
    size_t words = 0, off_x[POLY_MAX_B + 1] = {}, off_y[POLY_MAX_B] = {};
    const size_t off_map = words;
    if (mapped) words += ctw * nl + ctw * nl_u;
    for (uint32_t k = 2; k <= B; ++k) {
        off_x[k] = words;
        words += ctw * nlx[k];
    }
    for (uint32_t k = 2; k < G; ++k) {
        off_y[k] = words;
        words += ctw * nly[k];
    }
    const size_t off_ladder = words;
    words += ctw * nl_u + cheb_step_scratch(chunk, nl_u);
    const size_t off_out3 = words;
    words += (size_t)chunk * 3 * nl_T * n;
    const size_t off_relin = words;
    words += ctw * nl_T;
    const size_t off_resc = words;
    words += ctw * (nl_T - 1);
    const size_t off_comp = words;
    words += poly_tensor_scratch(B, G, chunk, nl_T);
    u64 *buf = poly_buffer(words);
    for (uint32_t done = 0; done < n_ct; done += chunk) {
        const uint32_t cnt = std::min(chunk, n_ct - done);
        u64 *pwx[POLY_MAX_B + 1] = {}, *pwy[POLY_MAX_B] = {};
        pwx[1] = const_cast<u64 *>(ct) + (size_t)done * 2 * nl * n;  // read only: the ladder writes pw[k] for k >= 2
        if (mapped) {
            u64 *pre = buf + off_map;
            pwx[1] = pre + ctw * nl;
            affine_core(ct + (size_t)done * 2 * nl * n, pre, cnt, nl, w_mul, w_add);
            rescale(pre, pwx[1], cnt, nl, nullptr);
        }
        for (uint32_t k = 2; k <= B; ++k) pwx[k] = buf + off_x[k];
        cheb_ladder_core(pwx, nlx, sx, rlk, cnt, B, buf + off_ladder);
        pwy[1] = pwx[B];
        for (uint32_t k = 2; k < G; ++k) pwy[k] = buf + off_y[k];
        cheb_ladder_core(pwy, nly, sy, rlk, cnt, G - 1, buf + off_ladder);
        PolyOpnd bo[POLY_MAX_B - 1] = {}, go[POLY_MAX_B - 1] = {};
        for (uint32_t i = 1; i < B; ++i) bo[i - 1] = PolyOpnd{pwx[i], nlx[i], 0};
        for (uint32_t j = 1; j < G; ++j) go[j - 1] = PolyOpnd{pwy[j], nly[j], 0};
        // looked up here, per chunk, behind the map's and the ladders' own lookups: any of them may empty the cache
        const u64 *table = poly_table(w.data(), B, G, nl_T);
        poly_tensor_core(bo, go, table, buf + off_out3, B, G, cnt, nl_T, buf + off_comp);
        relinearize(buf + off_out3, rlk, buf + off_relin, cnt, nl_T);
        rescale(buf + off_relin, buf + off_resc, cnt, nl_T, nullptr);
        rescale(buf + off_resc, out + (size_t)done * 2 * p.nl_out * n, cnt, nl_T - 1, nullptr);
    }
}

void Engine::lift_ntt(const double *coef, u64 *out, uint32_t cnt, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!cnt) return;
    EwGeom g{ps_.n, nl, ps_.L};
    k_lift<double><<<ew_grid(ps_.n, nl, cnt), EW_THREADS, 0, stream_>>>(coef, out, g, d_limb_, nl);
    MK_HIP(hipGetLastError());
    ntt_launch(out, cnt, nl, nl, false, nullptr, nullptr);
}

void Engine::encrypt(const u64 *pk, const u64 *pt, const int8_t *v, const int32_t *e0, const int32_t *e1, u64 *ct,
                     uint32_t n_ct, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!n_ct) return;
    const uint32_t n = ps_.n, D = ps_.D;
    const size_t poly = (size_t)nl * n;
    u64 *ws = workspace(3 * poly * n_ct);
    u64 *ve = ws, *e0e = ve + poly * n_ct, *e1e = e0e + poly * n_ct;
    EwGeom g{n, nl, ps_.L};
    k_lift<int8_t><<<ew_grid(n, nl, n_ct), EW_THREADS, 0, stream_>>>(v, ve, g, d_limb_, nl);
    k_lift<int32_t><<<ew_grid(n, nl, n_ct), EW_THREADS, 0, stream_>>>(e0, e0e, g, d_limb_, nl);
    k_lift<int32_t><<<ew_grid(n, nl, n_ct), EW_THREADS, 0, stream_>>>(e1, e1e, g, d_limb_, nl);
    MK_HIP(hipGetLastError());
    ntt_launch(ve, 3 * n_ct, nl, nl, false, nullptr, nullptr);
    // c0 = pk0*v + e0 + m ; c1 = pk1*v + e1   (pk addressed by limb id: first nl of its D limbs)
    Opnd p0{pk, 0, 1}, p1{pk + (size_t)D * n, 0, 1}, vv{ve, poly, 0};
    Opnd z0{e0e, poly, 0}, z1{e1e, poly, 0}, m{pt, poly, 0}, none{nullptr, 0, 0};
    k_fma<<<ew_grid(n, nl, n_ct), EW_THREADS, 0, stream_>>>(p0, vv, z0, m, nullptr, 0, ct, 2 * poly, 0, g, d_limb_, nl);
    k_fma<<<ew_grid(n, nl, n_ct), EW_THREADS, 0, stream_>>>(p1, vv, z1, none, nullptr, 0, ct + poly, 2 * poly, 0, g,
                                                         d_limb_, nl);
    MK_HIP(hipGetLastError());
}

void Engine::decrypt(const u64 *ct, const u64 *sk, u64 *m, uint32_t n_ct, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!n_ct) return;
    const uint32_t n = ps_.n;
    const size_t poly = (size_t)nl * n;
    EwGeom g{n, nl, ps_.L};
    // b = c1*s + c0 in EVALUATION, then COEFFICIENT
    Opnd c1{ct + poly, 2 * poly, 0}, s{sk, 0, 1}, c0{ct, 2 * poly, 0}, none{nullptr, 0, 0};
    k_fma<<<ew_grid(n, nl, n_ct), EW_THREADS, 0, stream_>>>(c1, s, c0, none, nullptr, 0, m, poly, 0, g, d_limb_, nl);
    MK_HIP(hipGetLastError());
    ntt_launch(m, n_ct, nl, nl, true, nullptr, nullptr);
}

// ---- re-randomisation before a key switch (PREBase::ReEncrypt(ct, evalKey, publicKey) -> EncryptZeroCore) ----------

// The fused endpoints (re-randomisation, partial decryption, collective key switch) run one column and one row kernel
// per arithmetic class of the first nl limbs: f(col_h, row_h, ar, mask, nsel) with the radices of the two passes (2, 3 or
// 4 each: two-round rows only) and the class as integral constants.  A ring size without such a pair is the caller's
// to keep away (the `fused` conditions of the three endpoints): it throws here instead of launching nothing.
template <typename F>
static void for_each_radix_class(const NttTables &T, const ClassMasks &m, F &&f) {
    bool found = false;
    dispatch<2, 3, 4>(fast_log_h(T.log_r1, 1u << T.log_r2), [&](auto col_h) {
        found = dispatch<2, 3, 4>(fast_row(T.log_r2, 1u << T.log_r1), [&](auto row_h) {
            for_each_class(T, m, [&](auto ar, unsigned long long mask, uint32_t nsel) { f(col_h, row_h, ar, mask, nsel); });
        });
    });
    if (!found) throw std::logic_error("fused endpoint needs a radix column pass and a two-round radix row pass");
}
template <typename F>
static void for_each_radix_class(const NttTables &T, uint32_t nl, F &&f) {
    for_each_radix_class(T, limb_classes(nl, T), f);
}

static void launch_rerand(LiftIo li, RerandArgs ra, const NttTables &T, uint32_t cnt, hipStream_t s) {
    for_each_radix_class(T, ra.nl, [&](auto col_h, auto row_h, auto ar, unsigned long long mask, uint32_t nsel) {
        constexpr int COL_H = decltype(col_h)::value, ROW_H = decltype(row_h)::value, AR = decltype(ar)::value;
        li.slot_mask = ra.slot_mask = mask;
        li.nsel = ra.nsel = nsel;
        k_lift_col<COL_H, AR><<<dim3(col_tiles<COL_H>(T), 3 * nsel, cnt), NTT_THREADS, 0, s>>>(li, T);
        k_rerand_row<ROW_H, AR><<<dim3(row_tiles<ROW_H>(T) * nsel * cnt), NTT_THREADS, 0, s>>>(ra, T);
    });
}

void Engine::rerandomize(const u64 *ct, const u64 *pk, const int8_t *v, const int64_t *e0, const int64_t *e1, u64 *out,
                         uint32_t n_ct, uint32_t nl_in, uint32_t nl) {
    need_device();
    check_nl(nl);
    check_nl(nl_in);
    if (nl > nl_in) throw std::invalid_argument("need nl <= nl_in");
    if (!n_ct) return;
    const uint32_t n = ps_.n, D = ps_.D;
    const size_t poly = (size_t)nl * n;
    // fused: lift inside the column pass, the products and sums inside the row pass's copy-out (two-round rows only)
    const int col_h = fast_log_h(tabs_.log_r1, 1u << tabs_.log_r2), row_h = fast_row(tabs_.log_r2, 1u << tabs_.log_r1);
    const bool fused = col_h != 0 && row_h >= 2 && row_h <= 4;
    const uint32_t chunk = knobs_.chunk;
    u64 *ws = workspace(3 * poly * (n_ct < chunk ? n_ct : chunk));
    for (uint32_t b0 = 0; b0 < n_ct; b0 += chunk) {
        const uint32_t cnt = n_ct - b0 < chunk ? n_ct - b0 : chunk;
        const u64 *cin = ct + (size_t)b0 * 2 * nl_in * n;
        u64 *cout = out + (size_t)b0 * 2 * poly;
        const int8_t *vb = v + (size_t)b0 * n;
        const int64_t *e0b = e0 + (size_t)b0 * n, *e1b = e1 + (size_t)b0 * n;
        if (fused) {
            const LiftIo li{vb, e0b, e1b, ws, nl, 0, 0};
            const RerandArgs ra{ws, cin, pk, cout, nl_in, nl, D, 0, 0};
            launch_rerand(li, ra, tabs_, cnt, stream_);
            MK_HIP(hipGetLastError());
        } else {  // the composition of Engine::encrypt with the ciphertext's components in the plaintext's place
            u64 *ve = ws, *e0e = ve + poly * cnt, *e1e = e0e + poly * cnt;
            EwGeom g{n, nl, ps_.L};
            k_lift<int8_t><<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(vb, ve, g, d_limb_, nl);
            k_lift<int64_t><<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(e0b, e0e, g, d_limb_, nl);
            k_lift<int64_t><<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(e1b, e1e, g, d_limb_, nl);
            MK_HIP(hipGetLastError());
            ntt_launch(ve, 3 * cnt, nl, nl, false, nullptr, nullptr);
            const size_t cstride = (size_t)2 * nl_in * n;
            Opnd p0{pk, 0, 1}, p1{pk + (size_t)D * n, 0, 1}, vv{ve, poly, 0}, z0{e0e, poly, 0}, z1{e1e, poly, 0};
            Opnd c0{cin, cstride, 0}, c1{cin + (size_t)nl_in * n, cstride, 0};
            k_fma<<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(p0, vv, z0, c0, nullptr, 0, cout, 2 * poly, 0, g, d_limb_, nl);
            k_fma<<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(p1, vv, z1, c1, nullptr, 0, cout + poly, 2 * poly, 0, g,
                                                                 d_limb_, nl);
            MK_HIP(hipGetLastError());
        }
    }
}

// ---- threshold decryption (MultipartyKeyGen / MultipartyDecryptLead, Main / MultipartyDecryptFusion) ---------------

void Engine::keygen_join(const u64 *pk_prev, const int8_t *s, const int32_t *e, u64 *pk, u64 *sk) {
    need_device();
    const uint32_t n = ps_.n, D = ps_.D, L = ps_.L;
    u64 *ee = workspace((size_t)D * n);
    EwGeom g{n, L, L};
    k_lift<int8_t><<<ew_grid(n, D, 1), EW_THREADS, 0, stream_>>>(s, sk, g, d_limb_, D);
    k_lift<int32_t><<<ew_grid(n, D, 1), EW_THREADS, 0, stream_>>>(e, ee, g, d_limb_, D);
    MK_HIP(hipGetLastError());
    ntt_launch(sk, 1, L, D, false, nullptr, nullptr);
    ntt_launch(ee, 1, L, D, false, nullptr, nullptr);
    // b = b_prev + e - a*s ; a copied
    Opnd x{pk_prev + (size_t)D * n, 0, 0}, y{sk, 0, 0}, z{ee, 0, 0}, w{pk_prev, 0, 0};
    k_fma<<<ew_grid(n, D, 1), EW_THREADS, 0, stream_>>>(x, y, z, w, nullptr, 1, pk, 0, 0, g, d_limb_, D);
    MK_HIP(hipGetLastError());
    if (pk != pk_prev)
        MK_HIP(hipMemcpyAsync(pk + (size_t)D * n, pk_prev + (size_t)D * n, (size_t)D * n * sizeof(u64), hipMemcpyDeviceToDevice,
                              stream_));
}

static void launch_pdec(PdecArgs pa, const NttTables &T, uint32_t cnt, hipStream_t s) {
    for_each_radix_class(T, pa.nl, [&](auto col_h, auto row_h, auto ar, unsigned long long mask, uint32_t nsel) {
        constexpr int COL_H = decltype(col_h)::value, ROW_H = decltype(row_h)::value, AR = decltype(ar)::value;
        pa.slot_mask = mask;
        pa.nsel = nsel;
        k_pdec_row<ROW_H, AR><<<dim3(row_tiles<ROW_H>(T) * nsel * cnt), NTT_THREADS, 0, s>>>(pa, T);
        k_pdec_col<COL_H, AR><<<dim3(col_tiles<COL_H>(T), nsel, cnt), NTT_THREADS, 0, s>>>(pa, T);
    });
}

void Engine::partial_decrypt(const u64 *ct, const u64 *sk, const int64_t *e, u64 *share, uint32_t n_ct, uint32_t nl_in,
                             uint32_t nl, bool lead) {
    need_device();
    check_nl(nl);
    check_nl(nl_in);
    if (nl > nl_in) throw std::invalid_argument("need nl <= nl_in");
    if (!n_ct) return;
    const uint32_t n = ps_.n;
    const size_t poly = (size_t)nl * n;
    // fused: the product inside the inverse row pass's copy-in, the error inside the inverse column pass's stores (two-round
    // rows only); the library switches take the composition
    const int col_h = fast_log_h(tabs_.log_r1, 1u << tabs_.log_r2), row_h = fast_row(tabs_.log_r2, 1u << tabs_.log_r1);
    const bool fused = col_h != 0 && row_h >= 2 && row_h <= 4 && !knobs_.generic_ntt && !knobs_.no_fp64 && !knobs_.no_pm;
    // the fused pair needs no workspace: its chunk is MKCKKS_CHUNK full-level ciphertexts' worth of limbs, so that a batch
    // of compact (1-limb) ciphertexts is not cut into launches of 16 limb polynomials (measured launch-bound: DESIGN.md)
    const uint32_t chunk = fused ? knobs_.chunk * (ps_.L / nl) : knobs_.chunk;
    u64 *ws = fused ? nullptr : workspace(poly * (n_ct < chunk ? n_ct : chunk));
    for (uint32_t b0 = 0; b0 < n_ct; b0 += chunk) {
        const uint32_t cnt = n_ct - b0 < chunk ? n_ct - b0 : chunk;
        const u64 *cin = ct + (size_t)b0 * 2 * nl_in * n;
        const int64_t *eb = e + (size_t)b0 * n;
        u64 *out = share + (size_t)b0 * poly;
        if (fused) {
            const PdecArgs pa{cin, sk, eb, out, nl_in, nl, lead ? 1u : 0u, 0, 0};
            launch_pdec(pa, tabs_, cnt, stream_);
            MK_HIP(hipGetLastError());
        } else {  // Engine::decrypt on the prefix, then the lifted error added
            EwGeom g{n, nl, ps_.L};
            const size_t cstride = (size_t)2 * nl_in * n;
            Opnd c1{cin + (size_t)nl_in * n, cstride, 0}, s{sk, 0, 1}, c0{lead ? cin : nullptr, cstride, 0}, none{nullptr, 0, 0};
            k_fma<<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(c1, s, c0, none, nullptr, 0, out, poly, 0, g, d_limb_, nl);
            MK_HIP(hipGetLastError());
            ntt_launch(out, cnt, nl, nl, true, nullptr, nullptr);
            k_lift<int64_t><<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(eb, ws, g, d_limb_, nl);
            k_add<<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(out, ws, out, g, d_limb_, nl);
            MK_HIP(hipGetLastError());
        }
    }
}

// ---- collective public-key switch: one party's share (Mouchet et al., PCKS) -----------------------------------------

static void launch_kswitch(LiftIo li, KswitchArgs ka, const NttTables &T, uint32_t cnt, hipStream_t s) {
    for_each_radix_class(T, ka.nl, [&](auto col_h, auto row_h, auto ar, unsigned long long mask, uint32_t nsel) {
        constexpr int COL_H = decltype(col_h)::value, ROW_H = decltype(row_h)::value, AR = decltype(ar)::value;
        li.slot_mask = ka.slot_mask = mask;
        li.nsel = ka.nsel = nsel;
        k_lift_col<COL_H, AR><<<dim3(col_tiles<COL_H>(T), 3 * nsel, cnt), NTT_THREADS, 0, s>>>(li, T);
        k_kswitch_row<ROW_H, AR><<<dim3(row_tiles<ROW_H>(T) * nsel * cnt), NTT_THREADS, 0, s>>>(ka, T);
    });
}

void Engine::switch_share(const u64 *ct, const u64 *sk, const u64 *pk, const int8_t *v, const int64_t *e0, const int64_t *e1,
                          u64 *share, uint32_t n_ct, uint32_t nl_in, uint32_t nl, bool lead) {
    need_device();
    check_nl(nl);
    check_nl(nl_in);
    if (nl > nl_in) throw std::invalid_argument("need nl <= nl_in");
    if (!n_ct) return;
    const uint32_t n = ps_.n, D = ps_.D;
    const size_t poly = (size_t)nl * n;
    // fused: lift inside the column pass, c1 * s (+ c0) and the mask inside the row pass's copy-outs (two-round rows only);
    // the library switches take the composition
    const int col_h = fast_log_h(tabs_.log_r1, 1u << tabs_.log_r2), row_h = fast_row(tabs_.log_r2, 1u << tabs_.log_r1);
    const bool fused = col_h != 0 && row_h >= 2 && row_h <= 4 && !knobs_.generic_ntt && !knobs_.no_fp64 && !knobs_.no_pm;
    const uint32_t chunk = knobs_.chunk;
    const uint32_t cmax = n_ct < chunk ? n_ct : chunk;
    u64 *ws = workspace((fused ? 3 : 4) * poly * cmax);
    for (uint32_t b0 = 0; b0 < n_ct; b0 += chunk) {
        const uint32_t cnt = n_ct - b0 < chunk ? n_ct - b0 : chunk;
        const u64 *cin = ct + (size_t)b0 * 2 * nl_in * n;
        u64 *cout = share + (size_t)b0 * 2 * poly;
        const int8_t *vb = v + (size_t)b0 * n;
        const int64_t *e0b = e0 + (size_t)b0 * n, *e1b = e1 + (size_t)b0 * n;
        if (fused) {
            const LiftIo li{vb, e0b, e1b, ws, nl, 0, 0};
            const KswitchArgs ka{ws, cin, sk, pk, cout, nl_in, nl, D, lead ? 1u : 0u, 0, 0};
            launch_kswitch(li, ka, tabs_, cnt, stream_);
            MK_HIP(hipGetLastError());
        } else {  // Engine::rerandomize's composition on the ciphertext (c1 * s (+ c0), 0): x from one k_fma into the workspace
            u64 *ve = ws, *e0e = ve + poly * cnt, *e1e = e0e + poly * cnt, *x = ws + 3 * poly * cmax;
            EwGeom g{n, nl, ps_.L};
            k_lift<int8_t><<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(vb, ve, g, d_limb_, nl);
            k_lift<int64_t><<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(e0b, e0e, g, d_limb_, nl);
            k_lift<int64_t><<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(e1b, e1e, g, d_limb_, nl);
            MK_HIP(hipGetLastError());
            ntt_launch(ve, 3 * cnt, nl, nl, false, nullptr, nullptr);
            const size_t cstride = (size_t)2 * nl_in * n;
            Opnd c1{cin + (size_t)nl_in * n, cstride, 0}, s{sk, 0, 1}, c0{lead ? cin : nullptr, cstride, 0}, none{nullptr, 0, 0};
            k_fma<<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(c1, s, c0, none, nullptr, 0, x, poly, 0, g, d_limb_, nl);
            Opnd p0{pk, 0, 1}, p1{pk + (size_t)D * n, 0, 1}, vv{ve, poly, 0}, z0{e0e, poly, 0}, z1{e1e, poly, 0}, xx{x, poly, 0};
            k_fma<<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(p0, vv, z0, xx, nullptr, 0, cout, 2 * poly, 0, g, d_limb_, nl);
            k_fma<<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(p1, vv, z1, none, nullptr, 0, cout + poly, 2 * poly, 0, g,
                                                                 d_limb_, nl);
            MK_HIP(hipGetLastError());
        }
    }
}

void Engine::fuse_shares(const u64 *shares, u64 *m, uint32_t n_parties, uint32_t n_ct, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!n_parties) throw std::invalid_argument("need n_parties >= 1");
    if (!n_ct) return;
    EwGeom g{ps_.n, nl, ps_.L};
    // every thread reads its words of all shares before it writes them: m may be shares[0]
    k_sum<<<ew_grid(ps_.n, nl, n_ct), EW_THREADS, 0, stream_>>>(shares, m, g, d_limb_, nl, n_parties, (size_t)n_ct * nl * ps_.n);
    MK_HIP(hipGetLastError());
}

// ---- collective evaluation keys of a joint key ("collective evaluation keys"); refusals in capi.cpp -------

// all D limbs of an evaluation-key polynomial by arithmetic class: bit i = limb id i, so bits >= L are the P limbs.  It is
// the selection ntt_launch(.., L, D, ..) makes (virtual slot v >= nl -> limb id L + v - nl) at nl = L, where v == id.
static ClassMasks qp_classes(uint32_t D, const NttTables &T) {
    NttIo sel{};
    sel.nslots = D;
    sel.nl = T.L;
    return slot_classes(sel, T);
}

// k_sum over the 2 * D limb rows of every (key, digit): geometry {n, D, L} makes row r's limb id r % D.  The lazy sum
// folds every 4 terms, so 64 terms of q - 1 are exact.  A thread reads its words of all parties before it writes them:
// out may be in[0].
void Engine::evk_sum(const u64 *in, u64 *out, uint32_t n_parties, uint32_t n_keys) {
    need_device();
    if (!n_parties || n_parties > SHAMIR_MAX_PARTIES) throw std::invalid_argument("need 1 <= n_parties <= MKCKKS_MAX_PARTIES");
    const uint32_t n = ps_.n, D = ps_.D;
    const size_t rows = (size_t)n_keys * ps_.beta, row_words = (size_t)2 * D * n;
    EwGeom g{n, D, ps_.L};
    for (size_t r0 = 0; r0 < rows; r0 += 32768) {  // grid.z
        const uint32_t cnt = (uint32_t)std::min<size_t>(32768, rows - r0);
        k_sum<<<ew_grid(n, 2 * D, cnt), EW_THREADS, 0, stream_>>>(in + r0 * row_words, out + r0 * row_words, g, d_limb_, 2 * D,
                                                                  n_parties, rows * row_words);
        MK_HIP(hipGetLastError());
    }
}

static void launch_relshare(RelshareLift li, RelshareArgs ra, const NttTables &T, uint32_t polys, hipStream_t s) {
    for_each_radix_class(T, qp_classes(ra.D, T), [&](auto col_h, auto row_h, auto ar, unsigned long long mask, uint32_t nsel) {
        constexpr int COL_H = decltype(col_h)::value, ROW_H = decltype(row_h)::value, AR = decltype(ar)::value;
        li.slot_mask = ra.slot_mask = mask;
        li.nsel = ra.nsel = nsel;
        k_relshare_col<COL_H, AR><<<dim3(col_tiles<COL_H>(T), nsel, polys), NTT_THREADS, 0, s>>>(li, T);
        k_relshare_row<ROW_H, AR><<<dim3(row_tiles<ROW_H>(T) * nsel * polys), NTT_THREADS, 0, s>>>(ra, T);
    });
}

void Engine::relin_share(const u64 *key1, const u64 *sk, const int32_t *e0, const int32_t *e1, u64 *share) {
    need_device();
    const uint32_t n = ps_.n, D = ps_.D, L = ps_.L, beta = ps_.beta;
    const size_t poly = (size_t)D * n;
    // fused: lift inside the column pass, key1 * sk + E inside the row pass's copy-out (two-round rows only); the library
    // switches take the composition
    const int col_h = fast_log_h(tabs_.log_r1, 1u << tabs_.log_r2), row_h = fast_row(tabs_.log_r2, 1u << tabs_.log_r1);
    const bool fused = col_h != 0 && row_h >= 2 && row_h <= 4 && !knobs_.generic_ntt && !knobs_.no_fp64 && !knobs_.no_pm &&
                       knobs_.relshare_fused != 0;
    u64 *ws = workspace(2 * beta * poly);
    if (fused) {
        const RelshareLift li{e0, e1, ws, D, 0, 0};
        const RelshareArgs ra{ws, key1, sk, share, D, 0, 0};
        launch_relshare(li, ra, tabs_, 2 * beta, stream_);
        MK_HIP(hipGetLastError());
        return;
    }
    // the composition (and the definition): the lifts and transforms of the key generators, one k_fma per component
    u64 *e0e = ws, *e1e = ws + beta * poly;
    EwGeom g{n, L, L};
    k_lift<int32_t><<<ew_grid(n, D, beta), EW_THREADS, 0, stream_>>>(e0, e0e, g, d_limb_, D);
    k_lift<int32_t><<<ew_grid(n, D, beta), EW_THREADS, 0, stream_>>>(e1, e1e, g, d_limb_, D);
    MK_HIP(hipGetLastError());
    ntt_launch(ws, 2 * beta, L, D, false, nullptr, nullptr);
    Opnd s{sk, 0, 0}, none{nullptr, 0, 0};
    Opnd k0{key1, 2 * poly, 0}, k1{key1 + poly, 2 * poly, 0}, z0{e0e, poly, 0}, z1{e1e, poly, 0};
    k_fma<<<ew_grid(n, D, beta), EW_THREADS, 0, stream_>>>(k0, s, z0, none, nullptr, 0, share, 2 * poly, 0, g, d_limb_, D);
    k_fma<<<ew_grid(n, D, beta), EW_THREADS, 0, stream_>>>(k1, s, z1, none, nullptr, 0, share + poly, 2 * poly, 0, g, d_limb_, D);
    MK_HIP(hipGetLastError());
}

void Engine::combine_key_shares(const u64 *in, const u64 *w, u64 *out, uint32_t m, uint32_t nl) {
    need_device();
    check_nl(nl);
    if (!m) throw std::invalid_argument("need m >= 1");
    EwGeom g{ps_.n, nl, ps_.L};
    const size_t poly = (size_t)nl * ps_.n;
    for (uint32_t l0 = 0; l0 < nl; l0 += WSUM_LIMBS) {
        const uint32_t lcnt = std::min(WSUM_LIMBS, nl - l0);
        for (uint32_t j0 = 0; j0 < m; j0 += WSUM_IN) {
            const uint32_t cnt = std::min(WSUM_IN, m - j0);
            WsumTable t{};
            for (uint32_t j = 0; j < cnt; ++j)
                for (uint32_t i = 0; i < lcnt; ++i) t.w[j][i] = w[(size_t)(j0 + j) * nl + l0 + i];
            // the first chunk of a limb reads in[0] before it writes out, the later ones add to out: out may be in[0]
            k_wsum<<<ew_grid(ps_.n, lcnt, 1), EW_THREADS, 0, stream_>>>(in + (size_t)j0 * poly, out, g, d_limb_, l0, cnt, poly,
                                                                        j0 != 0, t);
            MK_HIP(hipGetLastError());
        }
    }
}

// ---- randomness ------------------------------------------------------------------------------------

static ChaChaKey load_key(const uint8_t *key32) {
    if (!key32) throw std::invalid_argument("null sampler key");
    ChaChaKey k;
    for (int i = 0; i < 8; ++i)  // little-endian words, RFC 8439
        k.k[i] = (uint32_t)key32[4 * i] | ((uint32_t)key32[4 * i + 1] << 8) | ((uint32_t)key32[4 * i + 2] << 16) |
                 ((uint32_t)key32[4 * i + 3] << 24);
    return k;
}

void Engine::chacha_block(uint32_t *d_out16, const uint8_t *key32, uint32_t counter, const uint32_t nonce[3]) {
    need_device();
    k_chacha_block<<<1, 64, 0, stream_>>>(d_out16, load_key(key32), counter, nonce[0], nonce[1], nonce[2]);
    MK_HIP(hipGetLastError());
}

void Engine::sample_ternary(int8_t *out, size_t count, const uint8_t *key32, uint32_t sid) {
    need_device();
    const ChaChaKey key = load_key(key32);
    if (!count) return;
    k_sample_ternary<<<(unsigned)((count + 255) / 256), 256, 0, stream_>>>(out, count, key, sid);
    MK_HIP(hipGetLastError());
}

void Engine::sample_gauss(int32_t *out, size_t count, double sigma, const uint8_t *key32, uint32_t sid) {
    need_device();
    const ChaChaKey key = load_key(key32);
    if (!count) return;
    if (!(sigma > 0) || 12.0 * sigma > GAUSS_TABLE - 1) throw std::invalid_argument("sigma out of range");
    GaussTable t{};
    t.count = (int)std::ceil(12.0 * sigma) + 1;
    std::vector<long double> w(t.count);
    long double total = 0;
    for (int k = 0; k < t.count; ++k) {
        w[k] = std::exp(-(long double)k * k / (2.0L * sigma * sigma)) * (k ? 2.0L : 1.0L);
        total += w[k];
    }
    long double acc = 0;
    for (int k = 0; k < t.count; ++k) {
        acc += w[k] / total;
        const long double scaled = acc * 18446744073709551616.0L;
        t.thr[k] = scaled >= 18446744073709551615.0L ? ~0ull : (u64)scaled;
    }
    t.thr[t.count - 1] = ~0ull;
    k_sample_gauss<<<(unsigned)((count + 255) / 256), 256, 0, stream_>>>(out, count, key, sid, t);
    MK_HIP(hipGetLastError());
}

void Engine::sample_gauss_wide(int64_t *out, size_t count, double sigma, const uint8_t *key32, uint32_t sid) {
    need_device();
    const ChaChaKey key = load_key(key32);
    if (!count) return;
    const size_t pairs = (count + 1) / 2;
    k_sample_gauss_wide<<<(unsigned)((pairs + 255) / 256), 256, 0, stream_>>>(out, count, sigma, key, sid);
    MK_HIP(hipGetLastError());
}

void Engine::sample_uniform(u64 *out, uint32_t items, uint32_t nl, bool with_p, const uint8_t *key32, uint32_t sid) {
    need_device();
    const ChaChaKey key = load_key(key32);
    if (nl > ps_.L || (nl == 0 && !with_p)) throw std::invalid_argument("nl out of range");
    if (!items) return;
    const uint32_t slots = nl + (with_p ? ps_.K : 0);
    k_sample_uniform<<<dim3((ps_.n + 255) / 256, slots, items), 256, 0, stream_>>>(out, ps_.n, nl, ps_.L, d_limb_, key, sid);
    MK_HIP(hipGetLastError());
}

void Engine::share_key(const u64 *sk, u64 *shares, uint32_t nl, uint32_t n_parties, uint32_t threshold, const uint8_t *key32,
                       uint32_t sid0) {
    need_device();
    check_nl(nl);
    const ChaChaKey key = load_key(key32);
    if (threshold < 1 || threshold > n_parties || n_parties > SHAMIR_MAX_PARTIES)
        throw std::invalid_argument("need 1 <= threshold <= n_parties <= 64");
    if ((uint64_t)sid0 + threshold - 1 > 0xFFFFFFFFull) throw std::invalid_argument("stream ids overflow 32 bits");
    const uint32_t n = ps_.n, groups = (n_parties + SHAMIR_GROUP - 1) / SHAMIR_GROUP;
    k_shamir_share<<<dim3((n / 8 + 255) / 256, nl, groups), 256, 0, stream_>>>(sk, shares, n, nl, n_parties, threshold, d_limb_,
                                                                               key, sid0);
    MK_HIP(hipGetLastError());
}

void Engine::encrypt_seeded(const u64 *sk, const u64 *pt, const int32_t *e, u64 *c0, uint32_t n_ct, uint32_t nl,
                            const uint8_t *key32, uint32_t sid0) {
    need_device();
    check_nl(nl);
    const ChaChaKey key = load_key(key32);
    if (!n_ct) return;
    if ((uint64_t)sid0 + n_ct - 1 > 0xFFFFFFFFull) throw std::invalid_argument("stream ids overflow 32 bits");
    const uint32_t n = ps_.n;
    u64 *ee = workspace((size_t)n_ct * nl * n);
    EwGeom g{n, nl, ps_.L};
    k_lift<int32_t><<<ew_grid(n, nl, n_ct), EW_THREADS, 0, stream_>>>(e, ee, g, d_limb_, nl);
    MK_HIP(hipGetLastError());
    ntt_launch(ee, n_ct, nl, nl, false, nullptr, nullptr);
    k_encrypt_seeded<<<dim3((n / 8 + 255) / 256, nl, n_ct), 256, 0, stream_>>>(pt, ee, sk, c0, n, nl, d_limb_, key, sid0);
    MK_HIP(hipGetLastError());
}

void Engine::expand_seeded(u64 *ct, uint32_t n_ct, uint32_t nl, const uint8_t *keys32, const uint32_t *sids) {
    need_device();
    check_nl(nl);
    if (!n_ct) return;
    if (!keys32 || !sids) throw std::invalid_argument("null seed array");
    const uint32_t n = ps_.n;
    for (uint32_t t0 = 0; t0 < n_ct; t0 += SEED_ITEMS) {
        const uint32_t cnt = std::min(SEED_ITEMS, n_ct - t0);
        SeedTable t{};
        for (uint32_t i = 0; i < cnt; ++i) {
            t.key[i] = load_key(keys32 + (size_t)(t0 + i) * 32);
            t.sid[i] = sids[t0 + i];
        }
        k_expand_seeded<<<dim3((n / 8 + 255) / 256, nl, cnt), 256, 0, stream_>>>(ct + (size_t)t0 * 2 * nl * n, n, nl,
                                                                                d_limb_, t);
        MK_HIP(hipGetLastError());
    }
}

// ---- CKKS encode / decode (fp64 canonical embedding on the device) ---------------------------------

void Engine::encode(const double *vals, u64 *pt, uint32_t cnt, uint32_t nl, double scale) {
    need_device();
    check_nl(nl);
    if (!cnt) return;
    const uint32_t n = ps_.n, slots = n / 2;
    CodecTables t{d_rot_, reinterpret_cast<const double2 *>(d_ksi_), slots, ps_.log_n - 1, 2 * n};
    // arena: complex work array [cnt][slots] then coefficient doubles [cnt][N] (both 16*slots bytes per item)
    u64 *ws = workspace((size_t)cnt * n * 2 + (size_t)cnt * n);
    double2 *v = reinterpret_cast<double2 *>(ws);
    double *coef = reinterpret_cast<double *>(ws + (size_t)cnt * n * 2);
    const dim3 gs((slots + 255) / 256, cnt), gh((slots / 2 + 255) / 256, cnt);
    k_codec_load<<<gs, 256, 0, stream_>>>(vals, v, slots);
    for (uint32_t len = slots; len >= 2; len >>= 1) k_fft_special_inv_stage<<<gh, 256, 0, stream_>>>(v, t, len);
    k_codec_to_coef<<<gs, 256, 0, stream_>>>(v, coef, t, scale);
    MK_HIP(hipGetLastError());
    EwGeom g{n, nl, ps_.L};
    k_lift<double><<<ew_grid(n, nl, cnt), EW_THREADS, 0, stream_>>>(coef, pt, g, d_limb_, nl);
    MK_HIP(hipGetLastError());
    ntt_launch(pt, cnt, nl, nl, false, nullptr, nullptr);
}

// encode over Q_l P: the same rounded integer polynomial, lifted to every limb of the extended basis
void Engine::encode_ext(const double *vals, u64 *pt, uint32_t cnt, uint32_t nl, double scale) {
    need_device();
    check_nl(nl);
    if (!cnt) return;
    const uint32_t n = ps_.n, slots = n / 2, ext = nl + ps_.K;
    CodecTables t{d_rot_, reinterpret_cast<const double2 *>(d_ksi_), slots, ps_.log_n - 1, 2 * n};
    u64 *ws = workspace((size_t)cnt * n * 2 + (size_t)cnt * n);
    double2 *v = reinterpret_cast<double2 *>(ws);
    double *coef = reinterpret_cast<double *>(ws + (size_t)cnt * n * 2);
    const dim3 gs((slots + 255) / 256, cnt), gh((slots / 2 + 255) / 256, cnt);
    k_codec_load<<<gs, 256, 0, stream_>>>(vals, v, slots);
    for (uint32_t len = slots; len >= 2; len >>= 1) k_fft_special_inv_stage<<<gh, 256, 0, stream_>>>(v, t, len);
    k_codec_to_coef<<<gs, 256, 0, stream_>>>(v, coef, t, scale);
    MK_HIP(hipGetLastError());
    EwGeom g{n, nl, ps_.L};
    k_lift<double><<<ew_grid(n, ext, cnt), EW_THREADS, 0, stream_>>>(coef, pt, g, d_limb_, ext);
    MK_HIP(hipGetLastError());
    ntt_launch(pt, cnt, nl, ext, false, nullptr, nullptr);
}

const u64 *Engine::garner_table(uint32_t nl) {
    // Garner constants for the first nl limbs: inv[a] = (q_0..q_{a-1})^-1 mod q_a, G[a][k] = q_k mod q_a
    std::vector<u64> gar((size_t)nl + (size_t)nl * nl, 0);
    for (uint32_t a = 1; a < nl; ++a) {
        const u64 qa = ps_.moduli[a];
        u64 prod = 1;
        for (uint32_t k = 0; k < a; ++k) {
            gar[nl + (size_t)a * nl + k] = ps_.moduli[k] % qa;
            prod = h_mulmod(prod, ps_.moduli[k] % qa, qa);
        }
        gar[a] = h_invmod(prod, qa);
    }
    return limb_vector("garner_" + std::to_string(nl), gar);
}

void Engine::decode(const u64 *m, double *vals, uint32_t cnt, uint32_t nl, double scale) {
    need_device();
    check_nl(nl);
    if (!cnt) return;
    if (nl > (uint32_t)CRT_MAX_LIMBS) throw std::invalid_argument("decode supports at most 32 limbs");
    const uint32_t n = ps_.n, slots = n / 2;
    CodecTables t{d_rot_, reinterpret_cast<const double2 *>(d_ksi_), slots, ps_.log_n - 1, 2 * n};
    const u64 *d_gar = garner_table(nl);
    double2 *v = reinterpret_cast<double2 *>(workspace((size_t)cnt * n * 2));
    const dim3 gs((slots + 255) / 256, cnt), gh((slots / 2 + 255) / 256, cnt);
    k_crt_to_complex<<<gs, 256, 0, stream_>>>(m, v, t, d_limb_, d_gar, nl, scale);
    for (uint32_t len = 2; len <= slots; len <<= 1) k_fft_special_stage<<<gh, 256, 0, stream_>>>(v, t, len);
    k_codec_store_real<<<gs, 256, 0, stream_>>>(v, vals, slots);
    MK_HIP(hipGetLastError());
}

void Engine::decode_flood(const u64 *m, double *vals, uint32_t cnt, uint32_t nl, double scale, const uint8_t *key32,
                          uint32_t sid, double *h_log2) {
    need_device();
    check_nl(nl);
    const ChaChaKey key = load_key(key32);
    if (!cnt) return;
    if (nl > (uint32_t)CRT_MAX_LIMBS) throw std::invalid_argument("decode supports at most 32 limbs");
    const uint32_t n = ps_.n, slots = n / 2, nb = (n / 4 + FLOOD_THREADS - 1) / FLOOD_THREADS;
    CodecTables t{d_rot_, reinterpret_cast<const double2 *>(d_ksi_), slots, ps_.log_n - 1, 2 * n};
    const u64 *d_gar = garner_table(nl);
    // arena: complex work array [cnt][slots], per-block partials [cnt][nb][3], per-item statistics [cnt][4]
    u64 *ws = workspace((size_t)cnt * n + (size_t)cnt * nb * 3 + (size_t)cnt * 4);
    double2 *v = reinterpret_cast<double2 *>(ws);
    double *part = reinterpret_cast<double *>(ws + (size_t)cnt * n);
    double *stats = part + (size_t)cnt * nb * 3;
    const dim3 gs((slots + 255) / 256, cnt), gh((slots / 2 + 255) / 256, cnt);
    k_crt_symmetrise<<<dim3(nb, cnt), FLOOD_THREADS, (size_t)nl * FLOOD_THREADS * sizeof(u64), stream_>>>(
        m, v, part, t, d_limb_, d_gar, nl);
    const double max_log2 = (double)ps_.scaling_bits - 5.0;
    const double unit = scale / std::ldexp(1.0, (int)ps_.scaling_bits);  // estimate in units of scale / 2^p
    k_flood_stats<<<(cnt + 63) / 64, 64, 0, stream_>>>(part, stats, cnt, nb, n, std::sqrt((double)n) / 8.0, max_log2,
                                                       unit);
    k_flood<<<gs, 256, 0, stream_>>>(v, stats, t, key, sid, scale);
    for (uint32_t len = 2; len <= slots; len <<= 1) k_fft_special_stage<<<gh, 256, 0, stream_>>>(v, t, len);
    k_codec_store_real<<<gs, 256, 0, stream_>>>(v, vals, slots);
    MK_HIP(hipGetLastError());
    std::vector<double> h((size_t)cnt * 4);
    MK_HIP(hipMemcpyAsync(h.data(), stats, h.size() * sizeof(double), hipMemcpyDeviceToHost, stream_));
    MK_HIP(hipStreamSynchronize(stream_));
    if (h_log2)
        for (uint32_t i = 0; i < cnt; ++i) h_log2[i] = h[(size_t)i * 4 + 1];
    for (uint32_t i = 0; i < cnt; ++i)
        if (h[(size_t)i * 4 + 3] != 0.0) {
            char detail[160];
            std::snprintf(detail, sizeof detail, " (item %u: log2 sigma = %.3f > scaling_bits - 5 = %.0f)", i,
                          h[(size_t)i * 4 + 1], max_log2);
            throw PrecisionError(std::string("The decryption failed because the approximation error is too high. "
                                             "Check the parameters.") + detail);
        }
}

// the op ids of the public header are the probe's
#define X(name, id, n_in, n_out, n_tw, twk, cls, host) static_assert(MKCKKS_OP_##name == id, "MKCKKS_OP_" #name);
MK_PROBE_OPS(X)
#undef X
static_assert(MKCKKS_OP_COUNT == POP_COUNT, "MKCKKS_OP_COUNT");
// diagnostics (tests/test_device_arith.py): one primitive per element, device form on a device context, host form on a
// device = -1 context.  Companions of the twiddle planes are made here with the table code of the NTT tables.
void Engine::debug_arith(uint32_t op, u64 q, const u64 *in, u64 *out, size_t count) {
    ProbeDesc d;
    if (!probe_desc(op, d)) throw std::invalid_argument("debug_arith: unknown op");
    if (!(q & 1) || q <= (1ull << 17) || q >= (1ull << 60))
        throw std::invalid_argument("debug_arith: q must be odd with 2^17 < q < 2^60");
    if (d.cls == PCL_FP && q >= (5ull << 48)) throw std::invalid_argument("debug_arith: fp64 op with q >= 5 * 2^48");
    if (d.cls == PCL_PM && !pm_eligible(q)) throw std::invalid_argument("debug_arith: q is not pseudo-Mersenne");
    {
        const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out;
        const uintptr_t an = (uintptr_t)d.n_in * count * sizeof(u64), bn = (uintptr_t)d.n_out * count * sizeof(u64);
        if (a < b + bn && b < a + an && count) throw std::invalid_argument("debug_arith: in and out overlap");
    }
    if (device_ < 0 && !d.host) throw NoDevice("debug_arith: this op has a device form only");
    if (!count) return;
    ProbeK K;
    K.lc = make_limb_const(q, 1);
    K.P = PmK{};
    if (d.cls == PCL_FP) K.lc.fp = 1;
    if (d.cls == PCL_PM) {
        K.lc.pm = 1;
        K.lc.pm_c = (uint32_t)(((u64)1 << K.lc.k) - q);
        K.P = pm_consts(K.lc);
    }
    const uint32_t n_data = d.n_in - d.n_tw, n_exp = n_data + 2 * d.n_tw;
    // expanded twiddle planes: [n_tw][count] table entries, then [n_tw][count] companions
    std::vector<u64> tw;
    auto expand = [&](const u64 *w) {
        const size_t m = (size_t)d.n_tw * count;
        tw.resize(2 * m);
        for (size_t j = 0; j < m; ++j) {
            if (w[j] >= q) throw std::invalid_argument("debug_arith: twiddle not below q");
            if (d.tw == PTW_SHOUP) { tw[j] = w[j]; tw[m + j] = h_shoup(w[j], q); }
            else if (d.tw == PTW_PM) pm_table_entry(w[j], K.lc, tw[j], tw[m + j]);
            else fp_table_entry(w[j], q, tw[j], tw[m + j]);
        }
    };
    if (device_ < 0) {
        std::vector<u64> exp;
        const u64 *src = in;
        if (d.n_tw) {
            expand(in + (size_t)n_data * count);
            exp.assign(in, in + (size_t)n_data * count);
            exp.insert(exp.end(), tw.begin(), tw.end());
            src = exp.data();
        }
        switch (op) {
#define X(name, id, n_in, n_out, n_tw, twk, cls, host) \
    case id: for (size_t i = 0; i < count; ++i) probe_hd<id>(K, src, out, count, i); break;
            MK_PROBE_OPS(X)
#undef X
        }
        return;
    }
    MK_HIP(hipSetDevice(device_));
    const u64 *src = in;
    u64 *d_exp = nullptr;
    if (d.n_tw) {
        std::vector<u64> w((size_t)d.n_tw * count);
        MK_HIP(hipMemcpyAsync(w.data(), in + (size_t)n_data * count, w.size() * sizeof(u64), hipMemcpyDeviceToHost, stream_));
        MK_HIP(hipStreamSynchronize(stream_));
        expand(w.data());
        MK_HIP(hipMalloc(&d_exp, (size_t)n_exp * count * sizeof(u64)));
        hipError_t e = hipMemcpyAsync(d_exp, in, (size_t)n_data * count * sizeof(u64), hipMemcpyDeviceToDevice, stream_);
        if (e == hipSuccess)
            e = hipMemcpyAsync(d_exp + (size_t)n_data * count, tw.data(), tw.size() * sizeof(u64), hipMemcpyHostToDevice, stream_);
        if (e != hipSuccess) { (void)hipFree(d_exp); MK_HIP(e); }
        src = d_exp;
    }
    const unsigned grid = (unsigned)std::min<size_t>((count + PROBE_THREADS - 1) / PROBE_THREADS, 4096);
    switch (op) {
#define X(name, id, n_in, n_out, n_tw, twk, cls, host) \
    case id: k_arith_probe<id, host != 0><<<grid, PROBE_THREADS, 0, stream_>>>(K, src, out, count); break;
        MK_PROBE_OPS(X)
#undef X
    }
    hipError_t e = hipGetLastError();
    if (d_exp) {  // the staging buffer goes away with the call: wait for the kernel first
        if (e == hipSuccess) e = hipStreamSynchronize(stream_);
        (void)hipFree(d_exp);
    }
    MK_HIP(e);
}

void Engine::host_twiddles(uint32_t limb, bool inverse, std::vector<u64> &out) const {
    std::vector<u64> sh;
    ps_.twiddles(limb, inverse, out, sh);
}

}  // namespace mk
