// bsgs_kernels.hpp -- the kernels of the baby-step giant-step linear transform ("linear transforms";
// include/mkckks.h: mkckks_linear_transform_bsgs_batch has the definition).
//
// The engine compacts the plan before it launches anything: babies whose column has no present entry and giants whose
// row has none are dropped, the giants with a key come first.  Below n1 and n2 are the compacted counts and every index
// is a compacted one; kidx[] gives the key slot of a baby or giant in the caller's key array, ptidx[t n1 + b] the
// plaintext slot of (giant t, baby b) in the caller's array, or BSGS_ABSENT.
//
//   k_bsgs_baby<NPARTS>   lt_tile in its LT_BABY mode: the load, LDS-permute and inner-sum work of k_lt_accum per baby,
//                         the reduced pair (Bb_b, Ba_b) stored to bab u64[cnt][n1][2][ext][N].
//   k_bsgs_inner          streaming, a workgroup per (ciphertext, extended slot, tile): Ub_t = sum_b pt_{t,b} Bb_b and
//                         Ua_t likewise, for every giant, to ub / ua u64[n2][cnt][ext][N] (giant-major: the Ua_t of the
//                         keyed giants are one contiguous batch for ModDown).  A thread keeps BSGS_GROUP babies and the
//                         running sums of BSGS_GIANTS giants in registers: with at most BSGS_GROUP babies they are
//                         fetched once and every giant walks them; with more, a group of giants takes the babies group
//                         by group, so a baby tile is read once per BSGS_GIANTS giants, and the re-reads hit the 2 n1
//                         tiles of 4 KiB that the workgroup's XCD has just fetched.  The sums are lazy with the cadences
//                         of LtOps' outer sum (LtOps::addw), taken by the baby's position.  Only present plaintext tiles are read;
//                         the grid order of k_lt_accum puts the ciphertexts of a chunk that share them next to each
//                         other on one XCD.
//   k_bsgs_giant<NPARTS>  lt_tile in its LT_GIANT mode: a workgroup owns an output tile and keeps A_b, A_a in registers
//                         over all giants; giant t reads its own digits e_j (own limbs from v_t), its key, and Ub_t on
//                         all ext slots; the giants without a key follow and add their (Ub_t, Ua_t) unpermuted.
//                         til u64[cnt][2][ext][N], stored once.
//
// Bounds: as in lintrans_kernels.hpp (masked tile indices, clamped loads, predicated stores, exits before the first
// barrier); k_bsgs_inner has no barrier, clamps a baby index past n1 to n1 - 1 for its loads and never uses the words.
// LDS: that of k_lt_accum<NPARTS> for the two tile kernels, none for k_bsgs_inner.
#pragma once
#include <type_traits>

#include "lintrans_kernels.hpp"

namespace mk {

constexpr uint32_t BSGS_MAX = 64;
constexpr uint32_t BSGS_ABSENT = 0xffffffffu;
// babies a thread of k_bsgs_inner keeps in registers: 8 babies x 2 components x 2 words, 64 VGPRs
constexpr int BSGS_GROUP = 8;
// giants whose running sums it keeps beside them (2 components x 2 words, lazy: up to 64 VGPRs in the 128-bit class)
constexpr int BSGS_GIANTS = 4;

struct BsgsArgs : LtArgs {
    const uint32_t *kidx;  // key slot of rotation r (LT_BABY, LT_GIANT)
    const u64 *v;          // LT_GIANT: u64[n_rot][cnt][nl][N], ModDown(Ua_t) of the giants with a key
    const u64 *ub, *ua;    // LT_GIANT: u64[n_all][cnt][ext][N]
    uint32_t n_all;        // LT_GIANT: all giants; [0, n_rot) have a key, [n_rot, n_all) have none
};

struct BsgsInnerArgs {
    const u64 *bab;          // u64[cnt][n1][2][ext][N]
    const u64 *pts;          // u64[..][ext][N], indexed through ptidx
    const uint32_t *ptidx;   // u32[n2][n1]
    u64 *ub, *ua;            // u64[n2][cnt][ext][N]
    uint32_t n1, n2, cnt, nl, ext, L, log_n, log_t;
    uint32_t groups, members, xcd_order;
};

template <int NPARTS>
__global__ __launch_bounds__(LT_THREADS) void k_bsgs_baby(BsgsArgs a, const LimbConst *limb) {
    __shared__ ulonglong2 lds[(NPARTS + 1) * LT_TILE_PAIRS];
    lt_block<NPARTS, LT_BABY>(a, limb, lds);
}

template <int NPARTS>
__global__ __launch_bounds__(LT_THREADS) void k_bsgs_giant(BsgsArgs a, const LimbConst *limb) {
    __shared__ ulonglong2 lds[(NPARTS + 1) * LT_TILE_PAIRS];
    lt_block<NPARTS, LT_GIANT>(a, limb, lds);
}

// one (ciphertext, extended slot, tile): all giants
template <int CLS>
MK_D void bsgs_inner_tile(const BsgsInnerArgs &a, const LimbConst &lc, uint32_t item, uint32_t slot, uint32_t dbase) {
    typedef LtOps<CLS> Op;
    typedef typename Op::Word Word;
    const PmK P = CLS == LT_PM ? pm_consts(lc) : PmK{};
    const uint32_t n = 1u << a.log_n, pairs = 1u << (a.log_t - 1);
    const uint32_t c = threadIdx.x, cl = min(c, pairs - 1u);  // clamped: loads stay inside the tile
    const size_t comp = (size_t)a.ext * n;                     // words between the two components of a baby
    const u64 *bab = a.bab + ((size_t)item * a.n1 * 2 * a.ext + slot) * n + dbase;
    const bool once = a.n1 <= (uint32_t)BSGS_GROUP;
    Word Bb[BSGS_GROUP][2], Ba[BSGS_GROUP][2];
    auto fetch = [&](uint32_t b0) __attribute__((always_inline)) {
#pragma unroll
        for (int b = 0; b < BSGS_GROUP; ++b) {
            const u64 *row = bab + (size_t)min(b0 + (uint32_t)b, a.n1 - 1u) * 2 * comp;
            const ulonglong2 x = lt_ld(row, cl), y = lt_ld(row + comp, cl);
            Bb[b][0] = Op::in(x.x);
            Bb[b][1] = Op::in(x.y);
            Ba[b][0] = Op::in(y.x);
            Ba[b][1] = Op::in(y.y);
        }
    };
    if (once) fetch(0);
    for (uint32_t t0 = 0; t0 < a.n2; t0 += BSGS_GIANTS) {
        typename Op::Acc ab[BSGS_GIANTS][2], aa[BSGS_GIANTS][2];
        for (uint32_t b0 = 0; b0 < a.n1; b0 += BSGS_GROUP) {
            if (!once) fetch(b0);
            // one giant of the group against the babies in registers; tg is a compile-time index (written out below: in
            // a loop over tg the compiler indexes the sums in memory)
            auto giant = [&](auto TG) __attribute__((always_inline)) {
                constexpr int tg = decltype(TG)::value;
                if (t0 + (uint32_t)tg >= a.n2) return;  // block-uniform
#pragma unroll
                for (int b = 0; b < BSGS_GROUP; ++b) {
                    // the cadence by position: a fold before every FOLD_ROT-th baby, present or not, so no run between
                    // two folds has more than FOLD_ROT terms (a fold of an empty sum leaves it)
                    if constexpr (Op::FOLD_ROT != 0) {
                        if ((b0 + (uint32_t)b) % Op::FOLD_ROT == 0) {
#pragma unroll
                            for (int h = 0; h < 2; ++h) {
                                Op::fold(ab[tg][h], lc, P);
                                Op::fold(aa[tg][h], lc, P);
                            }
                        }
                    }
                    const uint32_t idx = b0 + (uint32_t)b < a.n1 ? a.ptidx[(t0 + tg) * a.n1 + b0 + b] : BSGS_ABSENT;  // block-uniform
                    if (idx == BSGS_ABSENT) continue;
                    const ulonglong2 pt = lt_ld(a.pts + ((size_t)idx * a.ext + slot) * n + dbase, cl);
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const Word ptw = Op::in(h ? pt.y : pt.x);
                        Op::addw(ab[tg][h], Bb[b][h], ptw, lc, P);
                        Op::addw(aa[tg][h], Ba[b][h], ptw, lc, P);
                    }
                }
            };
            giant(std::integral_constant<int, 0>{});
            giant(std::integral_constant<int, 1>{});
            giant(std::integral_constant<int, 2>{});
            giant(std::integral_constant<int, 3>{});
        }
        auto store = [&](auto TG) __attribute__((always_inline)) {
            constexpr int tg = decltype(TG)::value;
            if (t0 + (uint32_t)tg < a.n2 && c < pairs) {
                const size_t row = (((size_t)(t0 + tg) * a.cnt + item) * a.ext + slot) * n + dbase;
                reinterpret_cast<ulonglong2 *>(a.ub + row)[c] =
                    make_ulonglong2(Op::out(ab[tg][0], lc, P), Op::out(ab[tg][1], lc, P));
                reinterpret_cast<ulonglong2 *>(a.ua + row)[c] =
                    make_ulonglong2(Op::out(aa[tg][0], lc, P), Op::out(aa[tg][1], lc, P));
            }
        };
        store(std::integral_constant<int, 0>{});
        store(std::integral_constant<int, 1>{});
        store(std::integral_constant<int, 2>{});
        store(std::integral_constant<int, 3>{});
    }
}
static_assert(BSGS_GIANTS == 4, "k_bsgs_inner writes its giants out");

__global__ __launch_bounds__(LT_THREADS) void k_bsgs_inner(BsgsInnerArgs a, const LimbConst *limb) {
    uint32_t grp, m;
    lt_place(a, grp, m);
    if (grp >= a.groups) return;
    const uint32_t log_tiles = a.log_n - a.log_t;
    const uint32_t slot = grp >> log_tiles, dbase = (grp & ((1u << log_tiles) - 1u)) << a.log_t;
    const LimbConst lc = limb[limb_id_of(slot, a.nl, a.L)];
    if (lc.fp) bsgs_inner_tile<LT_FP>(a, lc, m, slot, dbase);
    else if (lc.pm) bsgs_inner_tile<LT_PM>(a, lc, m, slot, dbase);
    else bsgs_inner_tile<LT_INT>(a, lc, m, slot, dbase);
}

}  // namespace mk
