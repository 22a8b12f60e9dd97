// qsum_kernels.hpp -- the Q-limb half of the n-client server step in ONE kernel per arithmetic class (gfx950): k_qsum3_fp
// for the fp64-class limbs, described here, and k_qsum3_int below for the integer-class ones (q_0).
//
// For a (ciphertext index b, Q limb t, row tile) the workgroup walks ALL clients c and, per client,
//   * finishes the forward transform (row pass) of every converted ModUp digit d_j[t] and accumulates the eval-key
//     inner products  d_j[t] * b_j[t],  d_j[t] * a_j[t]   (EvalFastKeySwitchCoreExt; the digit that owns t is c1 itself),
//   * adds c0 * P (component 0),
// then finishes the forward transform of ApproxModDown's converted limbs -- already summed over the clients in
// coefficient format (k_icol_sum + k_conv_col_psum: the conversion is linear in the INTEGER sum of the clients' canonical
// coefficients, the transform is linear) -- and subtracts them,
// keeping the two running sums over digits AND clients in registers as exact doubles; after the last client one
// multiplication by P^-1 gives  sum_c [ (ctilde_c - conv_c) * P^-1 (+ c0_c) ]  mod q_t, the coefficient-wise sum of the
// clients' re-encryptions (ReEncrypt x n at changeCipherDomain.cpp:74 + the EvalAdd chain of
// aggregateEncryptedWeights.cpp:82).  Everything between the products and the final canonical value is ring arithmetic
// mod q_t, so the stored residues are those of the reference's per-client chain, bit for bit.
//
// Against a per-client fused row pass + inner product followed by a tail + sum kernel (rounds 1-2) this removes the
// round trip of the key-switch accumulators over Q through HBM (2 L limb writes + 2 L limb reads per client ciphertext)
// and n - 1 of the n multiplications by P^-1.
#pragma once
#include "ntt_radix.hpp"

#ifndef MK_QSUM_PARK_C
#define MK_QSUM_PARK_C 1
#endif

namespace mk {

struct QSumArgs {
    const u64 *dig;    // [client][cnt][nparts][ext][N] column-passed converted digits (doubles on fp64-class limbs)
    const u64 *conv;   // [cnt][2][nl][N]  column-passed ModDown conversions SUMMED over the clients (k_conv_col_psum)
    const u64 *cts;    // input ciphertexts: client c, index i at cts + c * ct_cstride + i * ct_stride, [2][nl][N]
    const u64 *evk;    // client c at evk + c * evk_cstride: [nparts][2][D][N]
    u64 *out;          // index i at out + i * ct_stride_out: [2][nl][N]
    const u64 *pq;     // per Q limb t, 4 doubles: P mod q, (P mod q) / q, P^-1 mod q, (P^-1 mod q) / q
    size_t ct_cstride, ct_stride, evk_cstride, out_stride;
    uint32_t n_clients, cnt, nl, ext, D, alpha;
    unsigned long long slot_mask;  // fp64-class Q limbs
    uint32_t nsel;
    uint32_t init_from_out;  // continue a running sum held in `out` (client groups)
    // weighted instance (W): client c, limb t at wt + (c * D + t) * 4: M_c mod q_t, its Shoup companion, and on fp64-class
    // Q limbs the doubles P * M_c mod q_t and that / q_t (Engine::weight_table)
    const u64 *wt;
    // integer-class Q limbs (k_qsum3_int): P^-1 mod q_t and its Shoup companion per limb; slot_mask / nsel then select those limbs
    const u64 *pinv = nullptr, *pinv_sh = nullptr;
};

// Three-round row geometry (RowT<LOGC>: 8 words per thread, 256-point rows as 8 x 8 x 4, 512-point rows as 8 x 8 x 8): the
// accumulators are 32 registers, every twiddle of the limb's rows is staged once (rounds A, B in LDS, round C parked in
// LDS too: MK_QSUM_PARK_C) instead of being re-read from L2 per transform, and the kernel runs 3 waves per SIMD.  (A
// two-round form with 16 words per thread and 2 waves was 1.5 % slower and is gone.)
// W: weighted aggregation -- the key-switch part runs unchanged on eval keys already scaled by M_c; c0 enters with
// P * M_c mod q_t in place of P mod q_t, read per client (wave-uniform).  The running sum taken over from `out` is already
// weighted: the prologue keeps the plain P.  The factor's size does not enter fp_mulmod's bound, so the sums grow as below.
template <int NPARTS, int LOGC, int MINW, bool W = false>
__global__ __launch_bounds__(NTT_THREADS, MINW) void k_qsum3_fp(QSumArgs a, NttTables T) {
    using TL = RowT<LOGC>;
    constexpr int R = TL::R, S = TL::ROWS, TPR = TL::TPR, PAIRS = 4;
    constexpr int ND = NPARTS - 1;
    // round-C twiddles parked in LDS (MK_QSUM_PARK_C): 28 registers less across the client loop
    constexpr int NC = MK_QSUM_PARK_C ? (LOGC == 3 ? 7 : 6) : 0;
    __shared__ u64 lds[TL::WORDS + 2 * (TL::TWA + TL::TWB)];
    __shared__ ulong2 ldsc[NC ? NC * NTT_THREADS : 1];
    Row3Ctx c;
    c.lds = lds;
    c.twa = lds + TL::WORDS;
    c.twa_sh = c.twa + TL::TWA;
    c.twb = c.twa_sh + TL::TWA;
    c.twb_sh = c.twb + TL::TWB;
    c.twc = ldsc;
    const uint32_t n = 1u << T.log_n, r1 = 1u << T.log_r1;
    const uint32_t tiles = r1 / S, groups = tiles * a.nsel;
    uint32_t grp, b;
    group_member(blockIdx.x, groups, a.cnt, T.cu_affine, grp, b);
    const uint32_t sl = nth_set_bit(a.slot_mask, grp / tiles);
    const LimbConst lc = T.limb[sl];
    const int own = (int)(sl / a.alpha);
    const uint32_t row0 = (grp % tiles) * S;
    c.g = threadIdx.x / TPR;
    c.t = threadIdx.x % TPR;
    const u64 *tw = T.tw + (size_t)sl * n, *tw_sh = T.tw_sh + (size_t)sl * n;
    row3_stage_twiddles<LOGC>(c, tw, tw_sh, r1 + row0);
    u64 wc[7], wpc[7];
    row3_load_c_twiddles<LOGC>(tw, tw_sh, r1 + row0 + c.g, c.t, wc, wpc);
    if (MK_QSUM_PARK_C) {
        row3_park_c_twiddles<LOGC>(c, wc, wpc);
#pragma unroll
        for (int i = 0; i < 7; ++i) wc[i] = wpc[i] = 0;
    }
    const size_t tile_off = (size_t)row0 * R;
    const double q = lc.qd, qinv = lc.qinv;
    const double pm = bitsd(a.pq[4 * sl]), pmq = bitsd(a.pq[4 * sl + 1]);
    u64 *o0 = a.out + (size_t)b * a.out_stride + (size_t)sl * n + tile_off;
    u64 *o1 = o0 + (size_t)a.nl * n;
    double2 acc0[PAIRS], acc1[PAIRS];
#pragma unroll
    for (int i = 0; i < PAIRS; ++i) {
        if (a.init_from_out) {
            const int e = row3_pair<LOGC>(c.g, c.t, i);
            const ulong2 v0 = reinterpret_cast<const ulong2 *>(o0)[e], v1 = reinterpret_cast<const ulong2 *>(o1)[e];
            acc0[i].x = fp_mulmod(u52_to_double(v0.x), pm, pmq, q);
            acc0[i].y = fp_mulmod(u52_to_double(v0.y), pm, pmq, q);
            acc1[i].x = fp_mulmod(u52_to_double(v1.x), pm, pmq, q);
            acc1[i].y = fp_mulmod(u52_to_double(v1.y), pm, pmq, q);
        } else {
            acc0[i] = double2{0.0, 0.0};
            acc1[i] = double2{0.0, 0.0};
        }
    }
    const size_t th_off = tile_off + (size_t)c.g * R + c.t;
    auto src_of = [&](uint32_t cl, int u) -> const u64 * {
        if (cl < a.n_clients && ND > 0) {
            const size_t item = (size_t)cl * a.cnt + b;
            const int dj = u < own ? u : u + 1;
            return a.dig + ((item * NPARTS + dj) * a.ext + sl) * n + th_off;
        }
        return a.conv + (((size_t)b * 2 + u) * a.nl + sl) * n + th_off;
    };
    Stamper stm;  // diagnostic build: [0] own-digit products, [1] transforms, [2] digit products, [3] conversions + store, [4] total
    auto transform = [&](u64 (&x)[8], const u64 *next) {
        wave_lds_sync();  // previous transform's consumers finished reading this wave's rows
        row3_forward<AR_FP, LOGC, MK_QSUM_PARK_C != 0>(x, c, wc, wpc, lc);
#pragma unroll
        for (int k = 0; k < 8; ++k) lds[TL::at(c.g, 8 * c.t + k)] = dbits(fp_reduce(bitsd(x[k]), q, qinv));
        if (next) {
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = ld_stream(next + TPR * k);
        }
        wave_lds_sync();
    };
    u64 x[8];
    {
        const u64 *src = src_of(ND > 0 ? 0 : a.n_clients, 0);
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = ld_stream(src + TPR * k);
    }
    __syncthreads();  // twiddles staged
    const unsigned long long t_begin = stm.now();
    unsigned long long t_mark = t_begin;
#pragma unroll 1
    for (uint32_t cl = 0; cl < a.n_clients; ++cl) {
        const u64 *ct = a.cts + (size_t)cl * a.ct_cstride + (size_t)b * a.ct_stride + (size_t)sl * n + tile_off;
        const u64 *ek = a.evk + (size_t)cl * a.evk_cstride + (size_t)sl * n + tile_off;
        {
            const u64 *wc0 = W ? a.wt + ((size_t)cl * a.D + sl) * 4 : nullptr;
            const double pmc = W ? bitsd(wc0[2]) : pm, pmqc = W ? bitsd(wc0[3]) : pmq;
            const u64 *y1 = ct + (size_t)a.nl * n;
            const u64 *e0 = ek + ((size_t)own * 2 + 0) * a.D * n, *e1 = ek + ((size_t)own * 2 + 1) * a.D * n;
#pragma unroll
            for (int i = 0; i < PAIRS; ++i) {
                const int e = row3_pair<LOGC>(c.g, c.t, i);
                const ulong2 yy = ld_stream2(reinterpret_cast<const ulong2 *>(y1) + e);
                const ulong2 zz = ld_stream2(reinterpret_cast<const ulong2 *>(ct) + e);
                const ulong2 bb = reinterpret_cast<const ulong2 *>(e0)[e];
                const ulong2 aa = reinterpret_cast<const ulong2 *>(e1)[e];
                const double yx = u52_to_double(yy.x), yz = u52_to_double(yy.y);
                acc0[i].x += fp_mulmod_any(yx, u52_to_double(bb.x), q, qinv) + fp_mulmod(u52_to_double(zz.x), pmc, pmqc, q);
                acc0[i].y += fp_mulmod_any(yz, u52_to_double(bb.y), q, qinv) + fp_mulmod(u52_to_double(zz.y), pmc, pmqc, q);
                acc1[i].x += fp_mulmod_any(yx, u52_to_double(aa.x), q, qinv);
                acc1[i].y += fp_mulmod_any(yz, u52_to_double(aa.y), q, qinv);
                if (NPARTS > 4 || ND == 0) {
                    acc0[i].x = fp_reduce(acc0[i].x, q, qinv);
                    acc0[i].y = fp_reduce(acc0[i].y, q, qinv);
                    acc1[i].x = fp_reduce(acc1[i].x, q, qinv);
                    acc1[i].y = fp_reduce(acc1[i].y, q, qinv);
                }
            }
        }
        t_mark = stm.add<0>(t_mark);
        int nd = ND;
        if (ND == 1) asm volatile("" : "+s"(nd));  // two digits: keep this a loop -- inlined into the client loop it costs 50 more spilled registers
#pragma unroll 1
        for (int u = 0; u < nd; ++u) {
            const bool last_u = u == ND - 1;
            const int dj = u < own ? u : u + 1;
            const u64 *e0 = ek + ((size_t)dj * 2 + 0) * a.D * n, *e1 = ek + ((size_t)dj * 2 + 1) * a.D * n;
            // the digit's eval-key tiles in ONE burst right after its transform: loaded pair by pair at the point of use
            // (the `last_u` branch between the pairs kept the compiler from hoisting them) every pair waited for its own
            // L2 round trip -- +0.9 % on the step (before the transform instead: +0.4 %, 61 registers in scratch; the next
            // client's c1 / c0 tiles loaded a phase ahead as well: -1.0 ... -2.2 %, 74-85 registers in scratch)
            ulong2 ebb[PAIRS], eaa[PAIRS];
            transform(x, last_u ? src_of(cl + 1, 0) : src_of(cl, u + 1));
            t_mark = stm.add<1>(t_mark);
#pragma unroll
            for (int i = 0; i < PAIRS; ++i) {
                const int e = row3_pair<LOGC>(c.g, c.t, i);
                ebb[i] = reinterpret_cast<const ulong2 *>(e0)[e];
                eaa[i] = reinterpret_cast<const ulong2 *>(e1)[e];
            }
            __builtin_amdgcn_sched_barrier(0);  // the burst stays where it is written
#pragma unroll
            // per client the sums grow by at most 0.97 q (own digit) + 0.82 q (c0 P) + 0.75 q per converted digit on top
            // of the 0.51 q carried over: < 3.8 q < 2^53 for up to 4 digits (5, 6 digits: the extra reduction above);
            // the last digit's products end with the reduction that brings them back to 0.51 q
            for (int i = 0; i < PAIRS; ++i) {
                const int e = row3_pair<LOGC>(c.g, c.t, i);
                const int xx = (2 * e) % R;
                const ulong2 bb = ebb[i], aa = eaa[i];
                const double yx = bitsd(lds[TL::at(c.g, xx)]), yz = bitsd(lds[TL::at(c.g, xx + 1)]);
                acc0[i].x += fp_mulmod_any(yx, u52_to_double(bb.x), q, qinv);
                acc0[i].y += fp_mulmod_any(yz, u52_to_double(bb.y), q, qinv);
                acc1[i].x += fp_mulmod_any(yx, u52_to_double(aa.x), q, qinv);
                acc1[i].y += fp_mulmod_any(yz, u52_to_double(aa.y), q, qinv);
            }
            if (last_u) {  // one block of products, then the reductions: no branch between the pairs
#pragma unroll
                for (int i = 0; i < PAIRS; ++i) {
                    acc0[i].x = fp_reduce(acc0[i].x, q, qinv);
                    acc0[i].y = fp_reduce(acc0[i].y, q, qinv);
                    acc1[i].x = fp_reduce(acc1[i].x, q, qinv);
                    acc1[i].y = fp_reduce(acc1[i].y, q, qinv);
                }
            }
            t_mark = stm.add<2>(t_mark);
        }
    }
#pragma unroll 1
    for (int comp = 0; comp < 2; ++comp) {  // the summed ModDown conversions
        transform(x, comp == 0 ? src_of(a.n_clients, 1) : nullptr);
#pragma unroll
        for (int i = 0; i < PAIRS; ++i) {
            const int xx = (2 * row3_pair<LOGC>(c.g, c.t, i)) % R;
            const double yx = bitsd(lds[TL::at(c.g, xx)]), yz = bitsd(lds[TL::at(c.g, xx + 1)]);
            if (comp == 0) {
                acc0[i].x -= yx;
                acc0[i].y -= yz;
            } else {
                acc1[i].x -= yx;
                acc1[i].y -= yz;
            }
        }
    }
    const double pi = bitsd(a.pq[4 * sl + 2]), piq = bitsd(a.pq[4 * sl + 3]);
#pragma unroll
    for (int i = 0; i < PAIRS; ++i) {
        const int e = row3_pair<LOGC>(c.g, c.t, i);
        ulong2 r0, r1v;
        r0.x = fp_to_canonical(fp_mulmod(acc0[i].x, pi, piq, q), q, qinv);
        r0.y = fp_to_canonical(fp_mulmod(acc0[i].y, pi, piq, q), q, qinv);
        r1v.x = fp_to_canonical(fp_mulmod(acc1[i].x, pi, piq, q), q, qinv);
        r1v.y = fp_to_canonical(fp_mulmod(acc1[i].y, pi, piq, q), q, qinv);
        reinterpret_cast<ulong2 *>(o0)[e] = r0;
        reinterpret_cast<ulong2 *>(o1)[e] = r1v;
    }
    t_mark = stm.add<3>(t_mark);
    stm.add<4>(t_begin);
    stm.flush<2>(T.stamps, false);
}

// The same shape for the INTEGER-class Q limbs (q_0): a workgroup owns (ciphertext index b, integer Q limb, row tile),
// walks the clients of the group and keeps ONE pair of 128-bit accumulator sets over digits and clients, where
// k_row3_inner_int<.., false> reduced them once per client and wrote them to a til that k_row3_tail_once read back and
// summed.  The epilogue is k_row3_tail_once's, on its operands: forward row pass of the two summed ModDown conversions,
//   out = ( sum_c ctilde_c - conv_sum ) * P^-1 + sum_c c0_c   (component 0; without the c0 term on component 1).
// Ring arithmetic mod q throughout, and the stored words are canonical: they are those of the two-kernel form, bit for bit.
//
// Deferred reduction.  A product is (lazy transform output or canonical c1 word) x (eval-key residue):
//   AR_PM:  the lazy words go in as they are, < 8U = 2^(k+3) <= 2^63; a residue is < 2^60: a product is < 2^123, and 31 of
//           them plus the canonical value carried over from the previous run (< 2^60) stay below 32 * 2^123 = 2^128.
//           pm_reduce128 itself stops at 2^(2k+6), i.e. 8 such products: the runs end in pm_reduce128_wide.
//   AR_INT: the words are made canonical before the product (as in k_row3_inner_int), a product is < q^2 <= 2^120, and
//           reduce_wide takes X < 2^124: 15 products plus the carried value (15 * 2^120 + 2^60 < 2^124).
// A client adds NPARTS products to every accumulator, so a run is floor(31 / NPARTS) or floor(15 / NPARTS) clients; the
// reduced value becomes the first addend of the next run.  The flagship's 8 clients x 3 digits are one run of 24.
// c0 is summed as 64-bit integers of canonical residues, reduced every 8 terms (< 9 * 2^60), as in k_row3_tail_once.
template <int AR>
MK_HD constexpr int qsum_int_products() { return AR == AR_PM ? 31 : 15; }
// The round-C twiddles are parked in LDS as in k_qsum3_fp (MK_QSUM_INT_PARK_C): held in registers across the client loop
// they put 13-24 registers of the pseudo-Mersenne instances into scratch.
#ifndef MK_QSUM_INT_PARK_C
#define MK_QSUM_INT_PARK_C 1
#endif
template <int NPARTS, int LOGC, int AR, bool W = false>
__global__ __launch_bounds__(NTT_THREADS, 2) void k_qsum3_int(QSumArgs a, NttTables T) {
    using TL = RowT<LOGC>;
    constexpr int R = TL::R, S = TL::ROWS, TPR = TL::TPR, PAIRS = 4;
    static_assert(NPARTS >= 2 && NPARTS <= qsum_int_products<AR>(), "a client's products must fit one run");
    constexpr uint32_t RUN = qsum_int_products<AR>() / NPARTS;  // clients between two reductions
    constexpr bool PARK = MK_QSUM_INT_PARK_C != 0;
    constexpr int NC = PARK ? (LOGC == 3 ? 7 : 6) : 0;
    __shared__ u64 lds[TL::WORDS + 2 * (TL::TWA + TL::TWB)];
    __shared__ ulong2 ldsc[NC ? NC * NTT_THREADS : 1];
    Row3Ctx c;
    c.lds = lds;
    c.twa = lds + TL::WORDS;
    c.twa_sh = c.twa + TL::TWA;
    c.twb = c.twa_sh + TL::TWA;
    c.twb_sh = c.twb + TL::TWB;
    c.twc = ldsc;
    const uint32_t n = 1u << T.log_n, r1 = 1u << T.log_r1;
    const uint32_t tiles = r1 / S, groups = tiles * a.nsel;
    uint32_t grp, b;
    group_member(blockIdx.x, groups, a.cnt, T.cu_affine, grp, b);
    const uint32_t sl = nth_set_bit(a.slot_mask, grp / tiles);  // Q limb: slot == limb id
    const LimbConst lc = T.limb[sl];
    const int own = (int)(sl / a.alpha), j0 = own == 0 ? 1 : 0;
    const uint32_t row0 = (grp % tiles) * S;
    c.g = threadIdx.x / TPR;
    c.t = threadIdx.x % TPR;
    const u64 *tw = T.tw + (size_t)sl * n, *tw_sh = T.tw_sh + (size_t)sl * n;
    row3_stage_twiddles<LOGC>(c, tw, tw_sh, r1 + row0);
    u64 wc[7], wpc[7];
    row3_load_c_twiddles<LOGC>(tw, tw_sh, r1 + row0 + c.g, c.t, wc, wpc);
    if (PARK) {
        row3_park_c_twiddles<LOGC>(c, wc, wpc);
#pragma unroll
        for (int i = 0; i < 7; ++i) wc[i] = wpc[i] = 0;
    }
    const size_t tile_off = (size_t)row0 * R;
    const uint32_t th = (uint32_t)c.g * R + c.t;
    const size_t dig_limb = (size_t)a.ext * n, dig_item = NPARTS * dig_limb;
    // wave-uniform bases: digit j of client cl at digs + cl * cnt * dig_item + j * dig_limb, conversion u at convs + u * nl * n
    const u64 *digs = a.dig + (size_t)b * dig_item + (size_t)sl * n + tile_off;
    const u64 *convs = a.conv + ((size_t)b * 2 * a.nl + sl) * n + tile_off;
    u64 h0[2 * PAIRS], l0[2 * PAIRS], h1[2 * PAIRS], l1[2 * PAIRS], z[2 * PAIRS];
#pragma unroll
    for (int i = 0; i < 2 * PAIRS; ++i) h0[i] = l0[i] = h1[i] = l1[i] = z[i] = 0;
    auto reduce = [&](u64 hi, u64 lo) -> u64 {
        if (AR == AR_PM) return pm_reduce128_wide(hi, lo, pm_consts(lc), lc.q);
        return reduce_wide(hi, lo, lc);
    };
    u64 x[8];
    {
        const u64 *src = digs + j0 * dig_limb;
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = ld_stream(src + th + TPR * k);
    }
    __syncthreads();  // twiddles staged
    uint32_t in_run = 0, cl = 0;
    // a group has at least one client and a context of this kernel at least one converted digit: both loops test at the
    // bottom, so no value of the limb (the pseudo-Mersenne constants live in scalar registers) meets a skipped-loop path
#pragma unroll 1
    do {
        const u64 *ct = a.cts + (size_t)cl * a.ct_cstride + (size_t)b * a.ct_stride + (size_t)sl * n + tile_off;
        const u64 *ek = a.evk + (size_t)cl * a.evk_cstride + (size_t)sl * n + tile_off;
        {   // the digit that owns this limb: c1 itself; c0 joins its sum
            const u64 *y1 = ct + (size_t)a.nl * n;
            const u64 *e0 = ek + ((size_t)own * 2 + 0) * a.D * n, *e1 = ek + ((size_t)own * 2 + 1) * a.D * n;
            const u64 *w = W ? a.wt + ((size_t)cl * a.D + sl) * 4 : nullptr;
            const u64 w0 = W ? w[0] : 0, w1 = W ? w[1] : 0;
#pragma unroll
            for (int i = 0; i < PAIRS; ++i) {
                const int e = row3_pair<LOGC>(c.g, c.t, i);
                const ulong2 yy = ld_stream2(reinterpret_cast<const ulong2 *>(y1) + e);
                const ulong2 zz = ld_stream2(reinterpret_cast<const ulong2 *>(ct) + e);
                const ulong2 bb = reinterpret_cast<const ulong2 *>(e0)[e];
                const ulong2 cc = reinterpret_cast<const ulong2 *>(e1)[e];
                mac128(h0[2 * i], l0[2 * i], yy.x, bb.x);
                mac128(h0[2 * i + 1], l0[2 * i + 1], yy.y, bb.y);
                mac128(h1[2 * i], l1[2 * i], yy.x, cc.x);
                mac128(h1[2 * i + 1], l1[2 * i + 1], yy.y, cc.y);
                z[2 * i] += W ? shoup_mul(zz.x, w0, w1, lc.q) : zz.x;
                z[2 * i + 1] += W ? shoup_mul(zz.y, w0, w1, lc.q) : zz.y;
            }
            if ((cl & 7) == 7) {
#pragma unroll
                for (int i = 0; i < 2 * PAIRS; ++i) z[i] = reduce_word(z[i], lc);
            }
        }
        int jn = j0, np = NPARTS;
        if (NPARTS == 2) asm volatile("" : "+s"(np));  // two digits: keep this a loop, as in k_qsum3_fp
        int dj = jn;
#pragma unroll 1
        do {
            jn = dj + 1 == own ? dj + 2 : dj + 1;
            wave_lds_sync();  // previous transform's consumers finished reading this wave's row
            row3_forward<AR, LOGC, PARK>(x, c, wc, wpc, lc);
#pragma unroll
            for (int k = 0; k < 8; ++k) lds[TL::at(c.g, 8 * c.t + k)] = AR == AR_PM ? x[k] : canon8(x[k], lc.q, lc.q2);
            {   // the next digit, the next client's first digit, or the first summed conversion
                const u64 *src = jn < NPARTS ? digs + jn * dig_limb
                                             : (cl + 1 < a.n_clients ? digs + (size_t)a.cnt * dig_item + j0 * dig_limb : convs);
#pragma unroll
                for (int k = 0; k < 8; ++k) x[k] = ld_stream(src + th + TPR * k);
            }
            wave_lds_sync();
            const u64 *e0 = ek + ((size_t)dj * 2 + 0) * a.D * n, *e1 = ek + ((size_t)dj * 2 + 1) * a.D * n;
            ulong2 eb[PAIRS], ec[PAIRS];  // the digit's eval-key tiles in one burst (see k_qsum3_fp)
#pragma unroll
            for (int i = 0; i < PAIRS; ++i) {
                const int e = row3_pair<LOGC>(c.g, c.t, i);
                eb[i] = reinterpret_cast<const ulong2 *>(e0)[e];
                ec[i] = reinterpret_cast<const ulong2 *>(e1)[e];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < PAIRS; ++i) {
                const int xx = (2 * row3_pair<LOGC>(c.g, c.t, i)) % R;
                const u64 yx = lds[TL::at(c.g, xx)], yz = lds[TL::at(c.g, xx + 1)];
                mac128(h0[2 * i], l0[2 * i], yx, eb[i].x);
                mac128(h0[2 * i + 1], l0[2 * i + 1], yz, eb[i].y);
                mac128(h1[2 * i], l1[2 * i], yx, ec[i].x);
                mac128(h1[2 * i + 1], l1[2 * i + 1], yz, ec[i].y);
            }
            dj = jn;
        } while (dj < np);
        if (++in_run == RUN) {  // the run is full: its canonical value opens the next one
            in_run = 0;
#pragma unroll
            for (int i = 0; i < 2 * PAIRS; ++i) {
                l0[i] = reduce(h0[i], l0[i]);
                l1[i] = reduce(h1[i], l1[i]);
                h0[i] = h1[i] = 0;
            }
        }
        digs += (size_t)a.cnt * dig_item;
    } while (++cl < a.n_clients);
#pragma unroll
    for (int i = 0; i < 2 * PAIRS; ++i) {  // the last run (a value already canonical stays what it is)
        l0[i] = reduce(h0[i], l0[i]);
        l1[i] = reduce(h1[i], l1[i]);
        z[i] = reduce_word(z[i], lc);
    }
    const u64 pi = a.pinv[sl], pi_sh = a.pinv_sh[sl];
    u64 *o0 = a.out + (size_t)b * a.out_stride + (size_t)sl * n + tile_off;
#pragma unroll 1
    for (int comp = 0; comp < 2; ++comp) {  // the summed ModDown conversions, tail and store
        wave_lds_sync();
        row3_forward<AR, LOGC, PARK>(x, c, wc, wpc, lc);
#pragma unroll
        for (int k = 0; k < 8; ++k) lds[TL::at(c.g, 8 * c.t + k)] = canon8(x[k], lc.q, lc.q2);
        if (comp == 0) {
            const u64 *src = convs + (size_t)a.nl * n;
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = ld_stream(src + th + TPR * k);
        }
        wave_lds_sync();
        u64 *dst = o0 + (size_t)comp * a.nl * n;
#pragma unroll
        for (int i = 0; i < PAIRS; ++i) {
            const int e = row3_pair<LOGC>(c.g, c.t, i);
            const int xx = (2 * e) % R;
            const u64 tx = comp ? l1[2 * i] : l0[2 * i], ty = comp ? l1[2 * i + 1] : l0[2 * i + 1];
            ulong2 v;
            v.x = shoup_mul(sub_mod(tx, lds[TL::at(c.g, xx)], lc.q), pi, pi_sh, lc.q);
            v.y = shoup_mul(sub_mod(ty, lds[TL::at(c.g, xx + 1)], lc.q), pi, pi_sh, lc.q);
            if (comp == 0) {
                v.x = add_mod(v.x, z[2 * i], lc.q);
                v.y = add_mod(v.y, z[2 * i + 1], lc.q);
            }
            if (a.init_from_out) {
                const ulong2 o = reinterpret_cast<const ulong2 *>(dst)[e];
                v.x = add_mod(v.x, o.x, lc.q);
                v.y = add_mod(v.y, o.y, lc.q);
            }
            reinterpret_cast<ulong2 *>(dst)[e] = v;
        }
    }
}

}  // namespace mk
