// relshare_kernels.hpp -- round 2 of the collective relinearisation key, one party's share
// (mkckks_relin_share; Engine::relin_share; DESIGN.md: "collective evaluation keys"):
//   share[j][c][i] = key1[j][c][i] * sk[i] + NTT_i(e_c[j])   on ALL D limbs i (the Q limbs and the K limbs of P).
// Two kernels in the manner of k_lift_col / k_kswitch_row; the lifted errors exist in HBM only as the column pass's
// output, never in COEFFICIENT or in EVALUATION form.  Kernels of their own: no instance of the re-randomisation, the
// partial decryption or the collective key switch moves.
//
// Limb selection.  The fused endpoints before this one run on the first nl Q limbs, where slot == limb id.  An
// evaluation key is u64[D][N] per polynomial, limb id i at word offset i * N, and every table the transforms read
// (NttTables::limb, tw, tw_sh, twb) is indexed by limb id over all D limbs.  So the P limbs need no second addressing
// rule: the class masks are taken over limb ids 0 .. D-1 (Engine: qp_classes) and bit i >= L selects P limb i - L.
#pragma once
#include "ntt_radix.hpp"

namespace mk {

struct RelshareLift {
    const int32_t *e0, *e1;  // [beta][N], COEFFICIENT, signed
    u64 *out;                // [beta][2][D][N]: E0_j, E1_j after the column pass (lazy u64, doubles on an fp limb)
    uint32_t D;
    unsigned long long slot_mask;  // limb ids (Q and P) of this instance's arithmetic class
    uint32_t nsel;
};

// k_lift_col on 32-bit errors over limb ids: grid (column tile, nsel, 2 * beta: polynomial j * 2 + c).  The 8 N source
// bytes of a digit feed all D limbs of its two polynomials.
template <int LOG_H, int AR>
__global__ __launch_bounds__(NTT_THREADS, 4) void k_relshare_col(RelshareLift io, NttTables T) {
    using TL = ColTile<LOG_H>;
    constexpr int H = TL::H, S = TL::S;
    __shared__ u64 lds[TL::WORDS + ColTwB<LOG_H>::WORDS];
    const uint32_t n = 1u << T.log_n, r2 = 1u << T.log_r2;
    const uint32_t id = nth_set_bit(io.slot_mask, blockIdx.y), p = blockIdx.z;
    const LimbConst lc = T.limb[id];
    if ((lc.fp != 0) != (AR == AR_FP)) return;  // never: the host selects the limbs of this instance's class
    const int c = threadIdx.x % S, j = threadIdx.x / S;
    const int32_t *e = ((p & 1) ? io.e1 : io.e0) + (size_t)(p >> 1) * n + blockIdx.x * S + c;
    u64 x[H];
#pragma unroll
    for (int k = 0; k < H; ++k) x[k] = lift_signed((int64_t)e[(size_t)(j + H * k) * r2], lc);
    if (AR == AR_FP) {  // canonical residues -> doubles (exact, q < 2^51)
#pragma unroll
        for (int k = 0; k < H; ++k) x[k] = dbits(u52_to_double(x[k]));
    }
    u64 *dst = io.out + ((size_t)p * io.D + id) * n + blockIdx.x * S + c;
    col_forward_finish<LOG_H, AR>(x, lds, T.tw + (size_t)id * n, T.tw_sh + (size_t)id * n, lc, j, c, dst, r2);
}

struct RelshareArgs {
    const u64 *col;   // [beta][2][D][N] from k_relshare_col
    const u64 *key1;  // [beta][2][D][N], canonical
    const u64 *sk;    // [D][N], canonical
    u64 *out;         // [beta][2][D][N]; may be key1 (every word is read by the thread that writes it)
    uint32_t D;
    unsigned long long slot_mask;
    uint32_t nsel;
};

// Row pass with the share's tail: one workgroup per (polynomial, limb, row tile) finishes the forward transform of its S
// rows of E and the copy-out writes key1 * sk + E.  Product as k_fma (mul_mod on canonical words, every arithmetic
// class).  One LDS tile (k_kswitch_row has two).  Grid order of k_ntt_row_r: the 2 * beta polynomials of one
// (limb, tile) are neighbours in one XCD's queue, so the twiddle tile and the secret's tile are fetched once and then
// hit in L2.
template <int LOG_H, int AR>
__global__ __launch_bounds__(NTT_THREADS) void k_relshare_row(RelshareArgs a, NttTables T) {
    using TL = RowTile<LOG_H>;
    using TA = RowTwA<LOG_H>;
    constexpr int S = TL::S, R = TL::R, H = TL::H, PAIRS = S * R / 2 / NTT_THREADS;
    __shared__ u64 lds[TL::WORDS + 2 * TA::WORDS];
    u64 *twa = lds + TL::WORDS, *twa_sh = twa + TA::WORDS;
    const uint32_t n = 1u << T.log_n, r1 = 1u << T.log_r1;
    const uint32_t tiles = r1 / S, groups = tiles * a.nsel, items = gridDim.x / groups;
    uint32_t grp, item;
    group_member(blockIdx.x, groups, items, T.cu_affine, grp, item);
    const uint32_t id = nth_set_bit(a.slot_mask, grp / tiles);  // limb id, P limbs included
    const LimbConst lc = T.limb[id];
    if ((lc.fp != 0) != (AR == AR_FP)) return;  // block-uniform
    const uint32_t row0 = (grp % tiles) * S;
    const int g = threadIdx.x / H, j = threadIdx.x % H;
    const size_t tile = (size_t)id * n + (size_t)row0 * R, at = (size_t)item * a.D * n + tile;
    stage_twiddles_wave<LOG_H>(twa, twa_sh, T.tw + (size_t)id * n, T.tw_sh + (size_t)id * n, r1 + row0);
    wave_lds_sync();

    rerand_row_forward<LOG_H, AR>(a.col + at, lds, twa, twa_sh, T.twb + (size_t)id * 2 * n, row0, g, j, lc);
    const ulong2 *k1 = reinterpret_cast<const ulong2 *>(a.key1 + at), *sk = reinterpret_cast<const ulong2 *>(a.sk + tile);
    ulong2 *out = reinterpret_cast<ulong2 *>(a.out + at);
#pragma unroll
    for (int i = 0; i < PAIRS; ++i) {
        const int e = wave_pair<LOG_H>(i);
        const int gg = (2 * e) / R, xx = (2 * e) % R;
        const ulong2 k = ld_pass2(k1 + e), s = sk[e];
        ulong2 r;
        r.x = add_mod(mul_mod(k.x, s.x, lc), lds[TL::at(gg, xx)], lc.q);
        r.y = add_mod(mul_mod(k.y, s.y, lc), lds[TL::at(gg, xx + 1)], lc.q);
        st_pass2(out + e, r);
    }
}

}  // namespace mk
