// fanout_kernels.hpp -- fused kernels of the fan-out re-encryption (one ciphertext batch, many eval keys).
//
// Hybrid key switching splits into a half that depends on the ciphertext only (INTT of c1, ModUp conversions, forward
// transform of every converted digit = EvalKeySwitchPrecomputeCore) and a half that needs the key (inner product,
// ApproxModDown = EvalFastKeySwitchCoreExt).  These kernels are k_row3_inner_fp / k_row3_inner_int with the first half
// hoisted out of the key loop: a workgroup owns (ciphertext, limb, row tile), finishes the forward row transform of
// every converted digit ONCE, keeps all NPARTS transformed tiles in LDS (18 KiB each in both geometries), and then walks
// the keys of its group with one accumulator set, reading the digits from LDS and only the key tiles from HBM.
// Same helpers, same order per accumulator as the single-key kernels (owning digit first, then the converted digits in
// ascending order), so the residues are theirs bit for bit.
//
// LDS per workgroup (three digits): 3 x 18 KiB + twiddles (4 KiB at 512-point rows, 8 KiB at 256-point rows) = 58-62 KiB;
// the P-limb instance adds one scratch tile for the inverse row pass (76-80 KiB).  Two workgroups fit the 160 KiB of a
// CU either way, which is the 2-waves-per-SIMD residency these kernels are compiled for.
#pragma once
#include "ntt_radix.hpp"

namespace mk {

struct FanArgs {
    const u64 *dig;      // [item][nparts][ext][N] column-passed converted limbs (doubles on fp limbs)
    const u64 *c1;       // component 1 of the input ciphertexts, items c1_stride words apart: [nl][N] canonical
    const u64 *evks;     // key k at evks + k * evk_kstride: [nparts][2][D][N]
    u64 *til;            // [key][item][2][ext][N]
    u64 *pc;             // [key][item][2][K][N] (P-limb instance)
    size_t c1_stride, evk_kstride;
    uint32_t nl, ext, D, alpha, items, n_keys, K;
    unsigned long long slot_mask;
    uint32_t nsel;
};

// workgroups per CU (= waves per SIMD) the LDS footprint of `tiles_n` resident tiles allows: 2 up to three digits plus the
// scratch tile (2 x 79.9 KiB at 256-point rows), 1 beyond
template <int LOGC>
constexpr int fan_lds_words(int tiles_n) { return tiles_n * RowT<LOGC>::WORDS + 2 * (RowT<LOGC>::TWA + RowT<LOGC>::TWB); }
template <int LOGC>
constexpr int fan_waves(int tiles_n) { return 2 * fan_lds_words<LOGC>(tiles_n) * 8 <= 160 * 1024 ? 2 : 1; }

// digit at position s of the accumulation order: the owning digit first (own >= 0), then the others ascending
MK_D int fan_digit(int s, int own) { return own < 0 ? s : (s == 0 ? own : (s - 1 < own ? s - 1 : s)); }

// forward row pass of every converted digit of this wave's row(s) into tile j of `tiles` (TRANSFORM-ONCE half); the
// owning digit's tile is c1 itself.  STORE(x) maps a transformed word to what the products consume.
template <int NPARTS, int LOGC, int AR, typename FOwn, typename FStore>
MK_D void fan_transform_digits(u64 *tiles, Row3Ctx &c, const u64 *dig0, size_t dig_stride, const u64 *c1_tile, int own,
                               const u64 (&wc)[7], const u64 (&wpc)[7], const LimbConst &lc, FOwn &&own_word, FStore &&store_word) {
    using TL = RowT<LOGC>;
    constexpr int R = TL::R, TPR = TL::TPR, PAIRS = 4;
    int jn = own == 0 ? 1 : 0;
    u64 x[8];
    if (jn < NPARTS) {
        const u64 *src = dig0 + (size_t)jn * dig_stride;
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = ld_stream(src + TPR * k);
    }
    if (own >= 0) {
        u64 *tile = tiles + (size_t)own * TL::WORDS;
#pragma unroll
        for (int i = 0; i < PAIRS; ++i) {
            const int e = row3_pair<LOGC>(c.g, c.t, i);
            const int xx = (2 * e) % R;
            const ulong2 yy = ld_stream2(reinterpret_cast<const ulong2 *>(c1_tile) + e);
            tile[TL::at(c.g, xx)] = own_word(yy.x);
            tile[TL::at(c.g, xx + 1)] = own_word(yy.y);
        }
    }
    __syncthreads();  // twiddles staged
#pragma unroll 1
    for (int dj = jn; dj < NPARTS; dj = jn) {
        jn = dj + 1 == own ? dj + 2 : dj + 1;
        c.lds = tiles + (size_t)dj * TL::WORDS;
        row3_forward<AR, LOGC>(x, c, wc, wpc, lc);
#pragma unroll
        for (int k = 0; k < 8; ++k) c.lds[TL::at(c.g, 8 * c.t + k)] = store_word(x[k]);
        if (jn < NPARTS) {
            const u64 *src = dig0 + (size_t)jn * dig_stride;
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = ld_stream(src + TPR * k);
        }
    }
    wave_lds_sync();  // every tile of this wave's rows is complete
}

// this lane's eval-key words of digit d: 4 pairs of b_d and of a_d
template <int LOGC>
MK_D void fan_load_key(const u64 *evk, int d, uint32_t D, uint32_t id, uint32_t n, size_t tile_off, int g, int t,
                       ulong2 (&eb)[4], ulong2 (&ec)[4]) {
    const ulong2 *e0 = reinterpret_cast<const ulong2 *>(evk + (((size_t)d * 2 + 0) * D + id) * n + tile_off);
    const ulong2 *e1 = reinterpret_cast<const ulong2 *>(evk + (((size_t)d * 2 + 1) * D + id) * n + tile_off);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = row3_pair<LOGC>(g, t, i);
        eb[i] = e0[e];
        ec[i] = e1[e];
    }
}

// fp64-class Q limbs: til[key][item][comp][slot] = sum_j d_j * (b_j | a_j) of key `key`
template <int NPARTS, int LOGC>
__global__ __launch_bounds__(NTT_THREADS, fan_waves<LOGC>(NPARTS)) void k_fan3_inner_fp(FanArgs a, NttTables T) {
    using TL = RowT<LOGC>;
    constexpr int R = TL::R, S = TL::ROWS, PAIRS = 4;
    __shared__ u64 lds[fan_lds_words<LOGC>(NPARTS)];
    Row3Ctx c;
    c.lds = lds;
    c.twa = lds + NPARTS * TL::WORDS;
    c.twa_sh = c.twa + TL::TWA;
    c.twb = c.twa_sh + TL::TWA;
    c.twb_sh = c.twb + TL::TWB;
    const uint32_t n = 1u << T.log_n, r1 = 1u << T.log_r1;
    const uint32_t tiles = r1 / S, groups = tiles * a.nsel;
    uint32_t grp, item;
    group_member(blockIdx.x, groups, a.items, T.cu_affine, grp, item);
    const uint32_t sl = nth_set_bit(a.slot_mask, grp / tiles);
    const LimbConst lc = T.limb[sl];
    const int own = (int)(sl / a.alpha);
    const uint32_t row0 = (grp % tiles) * S;
    c.g = threadIdx.x / TL::TPR;
    c.t = threadIdx.x % TL::TPR;
    const u64 *tw = T.tw + (size_t)sl * n, *tw_sh = T.tw_sh + (size_t)sl * n;
    row3_stage_twiddles<LOGC>(c, tw, tw_sh, r1 + row0);
    const size_t tile_off = (size_t)row0 * R;
    const double q = lc.qd, qinv = lc.qinv;
    {
        u64 wc[7], wpc[7];
        row3_load_c_twiddles<LOGC>(tw, tw_sh, r1 + row0 + c.g, c.t, wc, wpc);
        const u64 *dig0 = a.dig + ((size_t)item * NPARTS * a.ext + sl) * n + tile_off + (size_t)c.g * R + c.t;
        fan_transform_digits<NPARTS, LOGC, AR_FP>(
            lds, c, dig0, (size_t)a.ext * n, a.c1 + (size_t)item * a.c1_stride + (size_t)sl * n + tile_off, own, wc, wpc, lc,
            [](u64 v) { return dbits(u52_to_double(v)); },
            [q, qinv](u64 v) { return dbits(fp_reduce(bitsd(v), q, qinv)); });
    }
    ulong2 eb[PAIRS], ec[PAIRS];
    fan_load_key<LOGC>(a.evks, own, a.D, sl, n, tile_off, c.g, c.t, eb, ec);
#pragma unroll 1
    for (uint32_t key = 0; key < a.n_keys; ++key) {
        const u64 *evk = a.evks + (size_t)key * a.evk_kstride;
        double2 acc0[PAIRS], acc1[PAIRS];
#pragma unroll
        for (int i = 0; i < PAIRS; ++i) acc0[i] = acc1[i] = double2{0.0, 0.0};
        // a rolled loop: unrolled, the compiler hoists every digit's key loads and the kernel's registers grow by ~40 per digit
#pragma unroll 1
        for (int s = 0; s < NPARTS; ++s) {
            const u64 *tile = lds + (size_t)fan_digit(s, own) * TL::WORDS;
            ulong2 nb[PAIRS], nc[PAIRS];  // the next digit's key tiles (the next key's first digit after the last one)
            const bool more = s + 1 < NPARTS || key + 1 < a.n_keys;
            if (more)
                fan_load_key<LOGC>(s + 1 < NPARTS ? evk : evk + a.evk_kstride, fan_digit(s + 1 < NPARTS ? s + 1 : 0, own), a.D,
                                   sl, n, tile_off, c.g, c.t, nb, nc);
#pragma unroll
            for (int i = 0; i < PAIRS; ++i) {
                const int xx = (2 * row3_pair<LOGC>(c.g, c.t, i)) % R;
                const double yx = bitsd(tile[TL::at(c.g, xx)]), yz = bitsd(tile[TL::at(c.g, xx + 1)]);
                const double p0x = fp_mulmod_any(yx, u52_to_double(eb[i].x), q, qinv);
                const double p0y = fp_mulmod_any(yz, u52_to_double(eb[i].y), q, qinv);
                const double p1x = fp_mulmod_any(yx, u52_to_double(ec[i].x), q, qinv);
                const double p1y = fp_mulmod_any(yz, u52_to_double(ec[i].y), q, qinv);
                acc0[i].x += p0x;  // (the single-key kernel assigns the first product: 0 + p is p)
                acc0[i].y += p0y;
                acc1[i].x += p1x;
                acc1[i].y += p1y;
            }
            if (more) {
#pragma unroll
                for (int i = 0; i < PAIRS; ++i) {
                    eb[i] = nb[i];
                    ec[i] = nc[i];
                }
            }
        }
        const size_t kitem = (size_t)key * a.items + item;
        u64 *t0 = a.til + ((kitem * 2 + 0) * a.ext + sl) * n + tile_off;
        u64 *t1 = a.til + ((kitem * 2 + 1) * a.ext + sl) * n + tile_off;
#pragma unroll
        for (int i = 0; i < PAIRS; ++i) {
            const int e = row3_pair<LOGC>(c.g, c.t, i);
            ulong2 r0, r1v;
            r0.x = fp_to_canonical(acc0[i].x, q, qinv);
            r0.y = fp_to_canonical(acc0[i].y, q, qinv);
            r1v.x = fp_to_canonical(acc1[i].x, q, qinv);
            r1v.y = fp_to_canonical(acc1[i].y, q, qinv);
            st_stream2(reinterpret_cast<ulong2 *>(t0) + e, r0);
            st_stream2(reinterpret_cast<ulong2 *>(t1) + e, r1v);
        }
    }
}

// integer-class limbs: q_0 (INVP = false: accumulators to til) and the P limbs (INVP = true: accumulators straight through
// the inverse row pass into pc, as k_row3_inner_int<.., true> does); a.slot_mask selects SLOTS of one kind only
template <int NPARTS, int LOGC, bool INVP, int AR>
__global__ __launch_bounds__(NTT_THREADS, fan_waves<LOGC>(NPARTS + (INVP ? 1 : 0))) void k_fan3_inner_int(FanArgs a, NttTables T,
                                                                                                        uint32_t L) {
    using TL = RowT<LOGC>;
    constexpr int R = TL::R, S = TL::ROWS, TPR = TL::TPR, PAIRS = 4;
    constexpr int TILES = NPARTS + (INVP ? 1 : 0);  // + the scratch tile of the inverse row pass
    __shared__ u64 lds[fan_lds_words<LOGC>(TILES)];
    Row3Ctx c;
    c.lds = lds;
    c.twa = lds + TILES * TL::WORDS;
    c.twa_sh = c.twa + TL::TWA;
    c.twb = c.twa_sh + TL::TWA;
    c.twb_sh = c.twb + TL::TWB;
    const uint32_t n = 1u << T.log_n, r1 = 1u << T.log_r1;
    const uint32_t tiles = r1 / S, groups = tiles * a.nsel;
    uint32_t grp, item;
    group_member(blockIdx.x, groups, a.items, T.cu_affine, grp, item);
    const uint32_t sl = nth_set_bit(a.slot_mask, grp / tiles);
    const uint32_t id = limb_id_of(sl, a.nl, L);
    const LimbConst lc = T.limb[id];
    const int own = sl < a.nl ? (int)(sl / a.alpha) : -1;
    const uint32_t row0 = (grp % tiles) * S;
    c.g = threadIdx.x / TPR;
    c.t = threadIdx.x % TPR;
    const u64 *tw = T.tw + (size_t)id * n, *tw_sh = T.tw_sh + (size_t)id * n;
    row3_stage_twiddles<LOGC>(c, tw, tw_sh, r1 + row0);
    const size_t tile_off = (size_t)row0 * R;
    {
        u64 wc[7], wpc[7];
        row3_load_c_twiddles<LOGC>(tw, tw_sh, r1 + row0 + c.g, c.t, wc, wpc);
        const u64 *dig0 = a.dig + ((size_t)item * NPARTS * a.ext + sl) * n + tile_off + (size_t)c.g * R + c.t;
        // AR_PM: the lazy words (< 7.001U) go into the products as they are -- pm_reduce128 takes 6 x 2^63 x q
        fan_transform_digits<NPARTS, LOGC, AR>(
            lds, c, dig0, (size_t)a.ext * n, a.c1 + (size_t)item * a.c1_stride + (size_t)sl * n + tile_off, own, wc, wpc, lc,
            [](u64 v) { return v; }, [&lc](u64 v) { return AR == AR_PM ? v : canon8(v, lc.q, lc.q2); });
    }
    const u64 *itw = T.itw + (size_t)id * n, *itw_sh = T.itw_sh + (size_t)id * n;
    if (INVP) {
        __syncthreads();  // every wave is done with the forward round-A/B twiddles
        row3_stage_twiddles<LOGC>(c, itw, itw_sh, r1 + row0);
        __syncthreads();
        c.lds = lds + (size_t)NPARTS * TL::WORDS;
    }
    // the next digit's key tiles are requested one digit ahead; across the key boundary only where the epilogue is short
    // (INVP: 32 more live registers through two inverse row passes would spill)
    ulong2 eb[PAIRS], ec[PAIRS];
    if (!INVP) fan_load_key<LOGC>(a.evks, fan_digit(0, own), a.D, id, n, tile_off, c.g, c.t, eb, ec);
#pragma unroll 1
    for (uint32_t key = 0; key < a.n_keys; ++key) {
        const u64 *evk = a.evks + (size_t)key * a.evk_kstride;
        if (INVP) fan_load_key<LOGC>(evk, fan_digit(0, own), a.D, id, n, tile_off, c.g, c.t, eb, ec);
        u64 h0[2 * PAIRS], l0[2 * PAIRS], h1[2 * PAIRS], l1[2 * PAIRS];
#pragma unroll
        for (int i = 0; i < 2 * PAIRS; ++i) h0[i] = l0[i] = h1[i] = l1[i] = 0;
#pragma unroll 1
        for (int s = 0; s < NPARTS; ++s) {
            const u64 *tile = lds + (size_t)fan_digit(s, own) * TL::WORDS;
            ulong2 nb[PAIRS], nc[PAIRS];
            const bool more = s + 1 < NPARTS || (!INVP && key + 1 < a.n_keys);
            if (more)
                fan_load_key<LOGC>(s + 1 < NPARTS ? evk : evk + a.evk_kstride, fan_digit(s + 1 < NPARTS ? s + 1 : 0, own), a.D,
                                   id, n, tile_off, c.g, c.t, nb, nc);
#pragma unroll
            for (int i = 0; i < PAIRS; ++i) {
                const int xx = (2 * row3_pair<LOGC>(c.g, c.t, i)) % R;
                const u64 yx = tile[TL::at(c.g, xx)], yz = tile[TL::at(c.g, xx + 1)];
                mac128_split(h0[2 * i], l0[2 * i], yx, eb[i].x);
                mac128_split(h0[2 * i + 1], l0[2 * i + 1], yz, eb[i].y);
                mac128_split(h1[2 * i], l1[2 * i], yx, ec[i].x);
                mac128_split(h1[2 * i + 1], l1[2 * i + 1], yz, ec[i].y);
            }
            if (more) {
#pragma unroll
                for (int i = 0; i < PAIRS; ++i) {
                    eb[i] = nb[i];
                    ec[i] = nc[i];
                }
            }
        }
        const size_t kitem = (size_t)key * a.items + item;
#pragma unroll 1
        for (int comp = 0; comp < 2; ++comp) {
            ulong2 res[PAIRS];
#pragma unroll
            for (int i = 0; i < PAIRS; ++i) {
                const u64 hx = comp ? h1[2 * i] : h0[2 * i], lx = comp ? l1[2 * i] : l0[2 * i];
                const u64 hy = comp ? h1[2 * i + 1] : h0[2 * i + 1], ly = comp ? l1[2 * i + 1] : l0[2 * i + 1];
                if (AR == AR_PM) {
                    const PmK P = pm_consts(lc);
                    res[i].x = pm_reduce128(hx, lx, P, lc.q);
                    res[i].y = pm_reduce128(hy, ly, P, lc.q);
                } else {
                    res[i].x = NPARTS <= 4 ? reduce_sum4(hx, lx, lc) : reduce_wide(hx, lx, lc);
                    res[i].y = NPARTS <= 4 ? reduce_sum4(hy, ly, lc) : reduce_wide(hy, ly, lc);
                }
            }
            if (!INVP) {
                u64 *td = a.til + ((kitem * 2 + comp) * a.ext + sl) * n + tile_off;
#pragma unroll
                for (int i = 0; i < PAIRS; ++i) st_stream2(reinterpret_cast<ulong2 *>(td) + row3_pair<LOGC>(c.g, c.t, i), res[i]);
            } else {
                wave_lds_sync();  // the previous inverse pass finished reading this wave's scratch rows
#pragma unroll
                for (int i = 0; i < PAIRS; ++i) {
                    const int xx = (2 * row3_pair<LOGC>(c.g, c.t, i)) % R;
                    c.lds[TL::at(c.g, xx)] = res[i].x;
                    c.lds[TL::at(c.g, xx + 1)] = res[i].y;
                }
                wave_lds_sync();
                u64 x[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) x[k] = c.lds[TL::at(c.g, 8 * c.t + k)];
                u64 iwc[7], iwpc[7];  // (re)loaded per component: keeps them out of the accumulators' live range
                row3_load_c_twiddles<LOGC>(itw, itw_sh, r1 + row0 + c.g, c.t, iwc, iwpc);
                row3_inverse_int<LOGC, AR>(x, c, iwc, iwpc, lc);
                u64 *pd = a.pc + ((kitem * 2 + comp) * a.K + (sl - a.nl)) * n + tile_off + (size_t)c.g * R + c.t;
#pragma unroll
                for (int k = 0; k < 8; ++k) st_pass(pd + TPR * k, x[k]);  // lazy [0,2q): the inverse column pass scales
            }
        }
    }
}

}  // namespace mk
