// lintrans_kernels.hpp -- the accumulate kernel of the double-hoisted linear transform ("linear transforms").
//
// k_lt_accum: EVALUATION format over the extended basis Q_l P.  With d_j the ModUp digits of c1 (made once per
// ciphertext), sigma_g the gather of k_automorph and (kb, ka)_{r,j} the Galois key of rotation r, extended slot i of
// ciphertext `item` receives
//     A_b[i] = sum_r pt_r[i] ( sum_j sigma_{g_r}(d_j[i]) kb_{r,j}[i] + [i < nl] [P]_{q_i} sigma_{g_r}(c0[i]) )   mod m_i
//     A_a[i] = sum_r pt_r[i] ( sum_j sigma_{g_r}(d_j[i]) ka_{r,j}[i] )                                           mod m_i
// and for g_r = 1 (no rotation, no key) the inner sums are [i < nl] [P]_{q_i} c0[i] and [i < nl] [P]_{q_i} c1[i].
// ModDown of (A_b, A_a) closes the transform; P x on the Q limbs passes through it as + x.
//
// A workgroup owns one aligned OUTPUT tile of 2^log_t words (4 KiB where N >= 512, the whole row below) of one
// (ciphertext, extended slot) row.  By the block property (galois.hpp) the tile's words under sigma_g all come from ONE
// aligned source tile, and a 16-byte pair stays a pair (possibly swapped).  Per rotation the workgroup reads the source
// tile of every digit (the digit's own limbs and c0 straight from the ciphertext, as k_inner_product_b does) with
// coalesced 16-byte loads, parks them in LDS, reads them back permuted the way k_automorph does, and meets them with the
// key and plaintext words of its own tile.  The loads of rotation r + 1 (source tiles, keys, plaintext) are issued before
// the arithmetic of rotation r.  The two running sums of a word stay in registers over all rotations; every output word
// is stored once.  A thread owns one pair (two words).
//
// Arithmetic classes, block-uniform from the limb table (the flags the engine set under MKCKKS_NO_FP64 / MKCKKS_NO_PM).
// Every class stores canonical residues and every sum is exact mod m_i, so the bits do not depend on the class, the fold
// cadence or the order of the rotations.  Inputs are canonical residues, q < 2^60; an inner sum has T <= 7 products
// (at most 6 digits and the c0 term).
//   fp64 (q < 1.25 * 2^50): a product is fp_mulmod_any, the exact integer x y - b q with |.| <= 0.97 q for |x| <= q and
//       |.| <= 0.75 q for |x| <= 0.51 q.  Sums of such integers are exact below 2^53 >= 6.4 q, and fp_reduce brings a sum
//       with |.| < 2^53 back to |.| <= 0.51 q.  Inner sum: reduced before every LT_FP_TERMS = 4th product, so it stays
//       within 0.51 q + 4 * 0.97 q = 4.39 q; it is reduced to |u| <= 0.51 q before it meets the plaintext word.  Outer
//       sum: u pt is within 0.75 q; folded every LT_FP_ROT = 4 rotations it stays within 0.51 q + 4 * 0.75 q = 3.51 q.
//   pseudo-Mersenne (q = 2^k - c): 128-bit sums of whole products (mac128: x < 2^63, y < 2^60).  pm_reduce128 takes
//       X < 2^(2k+6), i.e. 64 products of canonical residues (each below 2^(2k)).  Inner sum: 7 products, one reduction
//       to a canonical u.  Outer sum: u pt products, folded every LT_PM_ROT = 32 rotations: 32 products plus one carried
//       residue, below 2^(2k+6) and below 2^126.
//   Shoup/Barrett (any other integer limb): the inner sum is a 128-bit sum of 7 products below 2^120, below 2^123:
//       inside reduce_wide's range 2^124.  u pt is one mul_mod (u, pt < q); terms are added canonically: no cadence.
// Long sums are handled by the cadences; n_rot has no cap.
//
// Key and plaintext tiles are shared by the ciphertexts of a chunk.  Two orders reuse them (LtArgs::xcd_order / walk,
// Knobs::lt_order; profiles/linear_transform_ab.txt has both): the grid order puts the workgroups that share an
// (extended slot, tile) next to each other on one XCD (block ids congruent mod 8 share an L2), the walk lets one
// workgroup serve all the chunk's ciphertexts one after the other.  The grid order measured 1.6 x faster and is the
// default.
// Bounds: a tile index is masked to its tile, the source tile base is below N by construction; pair indices past a
// short tile are clamped for loads (parked in the unused part of the LDS array) and predicated for stores; groups past
// the last (slot, tile) and items past the chunk leave before the first barrier (block-uniform).
#pragma once
#include <hip/hip_runtime.h>

#include "galois.hpp"
#include "galois_kernels.hpp"
#include "modarith.hpp"
#include "ntt_radix.hpp"

namespace mk {

constexpr uint32_t LT_FP_TERMS = 4, LT_FP_ROT = 4, LT_PM_ROT = 32;
constexpr uint32_t LT_XCDS = 8;
// a tile is 2^9 words (4 KiB; the whole row on smaller rings), one 16-byte pair per thread: with two pairs per thread
// (k_automorph's tile) the prefetch registers of five and six digits no longer fit and the kernel spills
constexpr uint32_t LT_THREADS = 256, LT_LOG_TILE = 9;
constexpr int LT_PAIRS = 1;
constexpr uint32_t LT_TILE_PAIRS = (1u << LT_LOG_TILE) / 2;

struct LtArgs {
    const u64 *ct;      // u64[cnt][2][nl][N]
    const u64 *dig;     // u64[cnt][nparts][ext][N]: converted limbs only (modup_core)
    const u64 *evks;    // u64[n_rot][evk_words], a key is u64[beta][2][D][N]
    const u64 *pts;     // u64[n_rot][ext][N]
    const uint32_t *g;  // device array of n_rot Galois elements
    const u64 *pmod;    // [P]_{q_i}, nl words
    u64 *til;           // u64[cnt][2][ext][N]
    size_t evk_words;
    uint32_t n_rot, cnt, nl, ext, L, D, alpha, log_n, log_t;
    uint32_t groups;    // ext << (log_n - log_t): the (slot, tile) pairs
    uint32_t members;   // workgroups per group: cnt without the walk, 1 with it
    uint32_t walk;      // 1: a workgroup walks the cnt ciphertexts of its group
    uint32_t xcd_order; // 1: a group's members are neighbours on one XCD; 0: member-major (no reuse intended)
};

enum { LT_INT = 0, LT_PM = 1, LT_FP = 2 };

template <int CLS>
struct LtOps;

template <>
struct LtOps<LT_INT> {
    typedef u64 Word;
    struct Sum {
        u64 h = 0, l = 0;
    };
    struct Acc {
        u64 v = 0;
    };
    static constexpr uint32_t FOLD_ROT = 0;
    static MK_D Word in(u64 x) { return x; }
    static MK_D void mac(Sum &s, Word d, Word k, uint32_t, const LimbConst &, const PmK &) { mac128_split(s.h, s.l, d, k); }
    static MK_D void add(Acc &a, const Sum &s, Word pt, const LimbConst &lc, const PmK &) {
        a.v = add_mod(a.v, mul_mod(reduce_wide(s.h, s.l, lc), pt, lc), lc.q);
    }
    static MK_D void fold(Acc &, const LimbConst &, const PmK &) {}
    static MK_D u64 out(const Acc &a, const LimbConst &, const PmK &) { return a.v; }
    // the pieces the baby-step giant-step kernels add (bsgs_kernels.hpp): an inner sum as a canonical residue, an outer
    // sum of products of canonical residues, an outer sum of reduced inner sums; the cadences are those of add
    static MK_D u64 red(const Sum &s, const LimbConst &lc, const PmK &) { return reduce_wide(s.h, s.l, lc); }
    static MK_D void addw(Acc &a, Word x, Word pt, const LimbConst &lc, const PmK &) {
        a.v = add_mod(a.v, mul_mod(x, pt, lc), lc.q);
    }
    static MK_D void addr(Acc &a, const Sum &s, const LimbConst &lc, const PmK &) {
        a.v = add_mod(a.v, reduce_wide(s.h, s.l, lc), lc.q);
    }
};

template <>
struct LtOps<LT_PM> {
    typedef u64 Word;
    struct Sum {
        u64 h = 0, l = 0;
    };
    struct Acc {
        u64 h = 0, l = 0;
    };
    static constexpr uint32_t FOLD_ROT = LT_PM_ROT;
    static MK_D Word in(u64 x) { return x; }
    static MK_D void mac(Sum &s, Word d, Word k, uint32_t, const LimbConst &, const PmK &) { mac128(s.h, s.l, d, k); }
    static MK_D void add(Acc &a, const Sum &s, Word pt, const LimbConst &lc, const PmK &P) {
        mac128(a.h, a.l, pm_reduce128(s.h, s.l, P, lc.q), pt);
    }
    static MK_D void fold(Acc &a, const LimbConst &lc, const PmK &P) {
        a.l = pm_reduce128(a.h, a.l, P, lc.q);
        a.h = 0;
    }
    static MK_D u64 out(const Acc &a, const LimbConst &lc, const PmK &P) { return pm_reduce128(a.h, a.l, P, lc.q); }
    static MK_D u64 red(const Sum &s, const LimbConst &lc, const PmK &P) { return pm_reduce128(s.h, s.l, P, lc.q); }
    static MK_D void addw(Acc &a, Word x, Word pt, const LimbConst &, const PmK &) { mac128(a.h, a.l, x, pt); }
    static MK_D void addr(Acc &a, const Sum &s, const LimbConst &lc, const PmK &P) {
        const u64 u = pm_reduce128(s.h, s.l, P, lc.q);  // LT_PM_ROT residues and one carried: far below 2^(2k+6)
        a.l += u;
        a.h += a.l < u;
    }
};

template <>
struct LtOps<LT_FP> {
    typedef double Word;
    struct Sum {
        double s = 0.0;
    };
    struct Acc {
        double v = 0.0;
    };
    static constexpr uint32_t FOLD_ROT = LT_FP_ROT;
    static MK_D Word in(u64 x) { return u52_to_double(x); }
    // t: the product's index in its inner sum (a compile-time constant after unrolling)
    static MK_D void mac(Sum &s, Word d, Word k, uint32_t t, const LimbConst &lc, const PmK &) {
        if (t && t % LT_FP_TERMS == 0) s.s = fp_reduce(s.s, lc.qd, lc.qinv);
        s.s += fp_mulmod_any(d, k, lc.qd, lc.qinv);
    }
    static MK_D void add(Acc &a, const Sum &s, Word pt, const LimbConst &lc, const PmK &) {
        a.v += fp_mulmod_any(fp_reduce(s.s, lc.qd, lc.qinv), pt, lc.qd, lc.qinv);
    }
    static MK_D void fold(Acc &a, const LimbConst &lc, const PmK &) { a.v = fp_reduce(a.v, lc.qd, lc.qinv); }
    static MK_D u64 out(const Acc &a, const LimbConst &lc, const PmK &) { return fp_to_canonical(a.v, lc.qd, lc.qinv); }
    static MK_D u64 red(const Sum &s, const LimbConst &lc, const PmK &) { return fp_to_canonical(s.s, lc.qd, lc.qinv); }
    // x canonical: a product within 0.97 q; folded every LT_FP_ROT terms the sum stays within 0.51 q + 4 * 0.97 q
    static MK_D void addw(Acc &a, Word x, Word pt, const LimbConst &lc, const PmK &) {
        a.v += fp_mulmod_any(x, pt, lc.qd, lc.qinv);
    }
    static MK_D void addr(Acc &a, const Sum &s, const LimbConst &lc, const PmK &) { a.v += fp_reduce(s.s, lc.qd, lc.qinv); }
};

MK_D ulonglong2 lt_ld(const u64 *row, uint32_t pair) { return reinterpret_cast<const ulonglong2 *>(row)[pair]; }

// What a tile does with the inner sums of its rotations (bsgs_kernels.hpp has the two other kernels):
//   LT_ACCUM  k_lt_accum: multiplies them by the rotation's plaintext and sums over the rotations
//   LT_BABY   k_bsgs_baby: stores each rotation's reduced pair to til u64[cnt][n_rot][2][ext][N]; no plaintext, no outer sum
//   LT_GIANT  k_bsgs_giant: rotation r < n_rot is a giant WITH a key, whose own digits come from a.dig / a.v at item
//             r cnt + item; in the place of [P] sigma(c0) stands sigma(Ub_r) on ALL ext slots, unmultiplied; the reduced
//             sums are added over the giants, no plaintext; the giants [n_rot, n_all) have no key and add (Ub_r, Ua_r)
// In the last two modes the key of rotation r is key slot a.kidx[r] (the engine compacts the plan).
enum { LT_ACCUM = 0, LT_BABY = 1, LT_GIANT = 2 };

// one (ciphertext, extended slot, output tile): all rotations
template <int CLS, int NPARTS, int MODE = LT_ACCUM, class Args = LtArgs>
MK_D void lt_tile(const Args &a, const LimbConst &lc, uint32_t item, uint32_t slot, uint32_t id, uint32_t dbase,
                  ulonglong2 *lds) {
    typedef LtOps<CLS> Op;
    typedef typename Op::Word Word;
    constexpr int NT = NPARTS + 1;  // source tiles of a keyed rotation: the digits, then c0 (Q slots only)
    const PmK P = CLS == LT_PM ? pm_consts(lc) : PmK{};
    const uint32_t n = 1u << a.log_n, tmask = (1u << a.log_t) - 1u, pairs = 1u << (a.log_t - 1);
    const bool isq = slot < a.nl;
    uint32_t c[LT_PAIRS], cl[LT_PAIRS];
#pragma unroll
    for (int p = 0; p < LT_PAIRS; ++p) {
        c[p] = threadIdx.x + (uint32_t)p * LT_THREADS;
        cl[p] = min(c[p], pairs - 1u);  // clamped: loads stay inside the tile
    }
    // rows of this (item, slot): component 0 / 1 of the ciphertext (Q slots), the digits
    const u64 *c0row, *c1row, *dig0;
    if constexpr (MODE != LT_GIANT) {
        c0row = a.ct + ((size_t)item * 2 * a.nl + slot) * n;
        c1row = c0row + (size_t)a.nl * n;
        dig0 = a.dig + ((size_t)item * NPARTS * a.ext + slot) * n;  // digit j: a.ext rows further each
    }
    // giant r of this item (LT_GIANT): v_r in the place of c1 (read on Q slots only; the row index is clamped, not
    // selected), Ub_r in the place of c0 (every slot)
    auto giant_rows = [&](uint32_t r) __attribute__((always_inline)) {
        if constexpr (MODE == LT_GIANT) {
            const size_t it = (size_t)r * a.cnt + item;
            c0row = a.ub + (it * a.ext + slot) * n;
            dig0 = a.dig + (it * NPARTS * a.ext + slot) * n;
            c1row = a.v + (it * a.nl + min(slot, a.nl - 1u)) * n;
        }
    };
    const Word pmod = Op::in(MODE == LT_GIANT ? 1 : isq ? a.pmod[slot] : 0);

    // The prefetch registers of one rotation.  Every load below is unconditional and only its ADDRESS is selected (an
    // unrotated term reads c1 in the place of digit 0 and the plaintext row in the place of its absent key; a P slot reads
    // digit 0 in the place of c0): with the loads under branches the compiler merges the branches' stores and indexes
    // the arrays on the stack.  Words read through a substituted address are never used.
    ulonglong2 S[NT][LT_PAIRS], kb[NPARTS][LT_PAIRS], ka[NPARTS][LT_PAIRS], pt[LT_PAIRS];
    auto load = [&](uint32_t r, uint32_t g) __attribute__((always_inline)) {
        const bool keyed = MODE == LT_GIANT || g != 1u;
        giant_rows(r);
        // the stand-in address of an absent key: the plaintext row, or a row of this tile that the mode does read
        const u64 *ptrow;
        if constexpr (MODE == LT_ACCUM) {
            ptrow = a.pts + ((size_t)r * a.ext + slot) * n + dbase;
#pragma unroll
            for (int p = 0; p < LT_PAIRS; ++p) pt[p] = lt_ld(ptrow, cl[p]);
        } else {
            ptrow = dig0 + dbase;
        }
        const uint32_t sbase = galois_src(dbase, g, a.log_n) & ~tmask;  // g = 1: the own tile
#pragma unroll
        for (int j = 0; j < NPARTS; ++j) {
            // digit j's own limbs are slots [j alpha, (j + 1) alpha) of Q: read from c1
            const bool mine = isq && slot - (uint32_t)j * a.alpha < a.alpha;
            const u64 *drow = (mine || (j == 0 && !keyed && isq)) ? c1row : dig0 + (size_t)j * a.ext * n;
#pragma unroll
            for (int p = 0; p < LT_PAIRS; ++p) S[j][p] = lt_ld(drow + sbase, cl[p]);
        }
        const u64 *zrow = (MODE == LT_GIANT || isq) ? c0row : dig0;
#pragma unroll
        for (int p = 0; p < LT_PAIRS; ++p) S[NPARTS][p] = lt_ld(zrow + sbase, cl[p]);
        uint32_t kslot = r;
        if constexpr (MODE != LT_ACCUM) kslot = a.kidx[r];
        const u64 *key = a.evks + (size_t)kslot * a.evk_words + (size_t)id * n + dbase;
#pragma unroll
        for (int j = 0; j < NPARTS; ++j) {
            const u64 *kbrow = keyed ? key + ((size_t)j * 2 + 0) * a.D * n : ptrow;  // g = 1: the key slot is never read
            const u64 *karow = keyed ? key + ((size_t)j * 2 + 1) * a.D * n : ptrow;
#pragma unroll
            for (int p = 0; p < LT_PAIRS; ++p) {
                kb[j][p] = lt_ld(kbrow, cl[p]);
                ka[j][p] = lt_ld(karow, cl[p]);
            }
        }
    };

    typename Op::Acc accb[LT_PAIRS][2], acca[LT_PAIRS][2];
    uint32_t g = a.g[0], pending = 0;
    if (MODE != LT_GIANT || a.n_rot) load(0, g);  // a plan may have no giant with a key (a.g has an entry all the same)
    for (uint32_t r = 0; r < a.n_rot; ++r) {
        // this rotation's operands leave the prefetch registers: the source tiles through LDS, permuted (g = 1: the
        // identity, so an unrotated term of a Q slot takes the same way; on a P slot it adds nothing and only prefetches)
        ulonglong2 d[NT][LT_PAIRS], ckb[NPARTS][LT_PAIRS], cka[NPARTS][LT_PAIRS], cpt[LT_PAIRS];
        const bool keyed = MODE == LT_GIANT || g != 1u, active = keyed || isq;  // block-uniform
        if (active) {
            __syncthreads();  // the previous rotation's reads are done
#pragma unroll
            for (int t = 0; t < NT; ++t) {
#pragma unroll
                for (int p = 0; p < LT_PAIRS; ++p) lds[t * LT_TILE_PAIRS + c[p]] = S[t][p];
            }
            __syncthreads();
#pragma unroll
            for (int p = 0; p < LT_PAIRS; ++p) {
                const uint32_t s = galois_src(dbase + 2u * c[p], g, a.log_n) & tmask;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    const ulonglong2 v = lds[t * LT_TILE_PAIRS + (s >> 1)];
                    d[t][p] = (s & 1u) ? make_ulonglong2(v.y, v.x) : v;
                }
            }
        }
#pragma unroll
        for (int p = 0; p < LT_PAIRS; ++p) {
            if constexpr (MODE == LT_ACCUM) cpt[p] = pt[p];
#pragma unroll
            for (int j = 0; j < NPARTS; ++j) {
                ckb[j][p] = kb[j][p];
                cka[j][p] = ka[j][p];
            }
        }
        if (r + 1 < a.n_rot) {  // the next rotation's words are on their way while this one is multiplied
            g = a.g[r + 1];
            load(r + 1, g);
        }
        // a baby's pair of this tile: an unrotated baby is zero on the P slots
        ulonglong2 *bb = nullptr, *ba = nullptr;
        if constexpr (MODE == LT_BABY) {
            bb = reinterpret_cast<ulonglong2 *>(a.til + ((((size_t)item * a.n_rot + r) * 2 + 0) * a.ext + slot) * n + dbase);
            ba = bb + (size_t)a.ext * (n / 2);
            if (!active) {
#pragma unroll
                for (int p = 0; p < LT_PAIRS; ++p)
                    if (c[p] < pairs) bb[c[p]] = ba[c[p]] = make_ulonglong2(0, 0);
            }
        }
        if (!active) continue;
        if (MODE != LT_BABY && Op::FOLD_ROT && pending == Op::FOLD_ROT) {
#pragma unroll
            for (int p = 0; p < LT_PAIRS; ++p) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    Op::fold(accb[p][h], lc, P);
                    Op::fold(acca[p][h], lc, P);
                }
            }
            pending = 0;
        }
        ++pending;
        ulonglong2 rb[LT_PAIRS], ra[LT_PAIRS];  // LT_BABY: the reduced pair
#pragma unroll
        for (int p = 0; p < LT_PAIRS; ++p) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                auto w = [&](const ulonglong2 &v) __attribute__((always_inline)) { return Op::in(h ? v.y : v.x); };
                typename Op::Sum sb, sa;
                if (keyed) {
#pragma unroll
                    for (int j = 0; j < NPARTS; ++j) {
                        const Word dj = w(d[j][p]);
                        Op::mac(sb, dj, w(ckb[j][p]), j, lc, P);
                        Op::mac(sa, dj, w(cka[j][p]), j, lc, P);
                    }
                } else {
                    Op::mac(sa, w(d[0][p]), pmod, 0, lc, P);  // [P] c1
                }
                // [P] sigma(c0) (LT_GIANT: sigma(Ub_r), every slot)
                if (MODE == LT_GIANT || isq) Op::mac(sb, w(d[NPARTS][p]), pmod, NPARTS, lc, P);
                if constexpr (MODE == LT_ACCUM) {
                    const Word ptw = w(cpt[p]);
                    Op::add(accb[p][h], sb, ptw, lc, P);
                    Op::add(acca[p][h], sa, ptw, lc, P);
                } else if constexpr (MODE == LT_GIANT) {
                    Op::addr(accb[p][h], sb, lc, P);
                    Op::addr(acca[p][h], sa, lc, P);
                } else {
                    (h ? rb[p].y : rb[p].x) = Op::red(sb, lc, P);
                    (h ? ra[p].y : ra[p].x) = Op::red(sa, lc, P);
                }
            }
        }
        if constexpr (MODE == LT_BABY) {
#pragma unroll
            for (int p = 0; p < LT_PAIRS; ++p)
                if (c[p] < pairs) {
                    bb[c[p]] = rb[p];
                    ba[c[p]] = ra[p];
                }
        }
    }
    if constexpr (MODE == LT_BABY) return;
    if constexpr (MODE == LT_GIANT) {  // the giants without a key: (Ub_r, Ua_r) of the own tile, as they are
        for (uint32_t r = a.n_rot; r < a.n_all; ++r) {
            const size_t row = (((size_t)r * a.cnt + item) * a.ext + slot) * n + dbase;
            if (Op::FOLD_ROT && pending == Op::FOLD_ROT) {
#pragma unroll
                for (int p = 0; p < LT_PAIRS; ++p) {
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        Op::fold(accb[p][h], lc, P);
                        Op::fold(acca[p][h], lc, P);
                    }
                }
                pending = 0;
            }
            ++pending;
#pragma unroll
            for (int p = 0; p < LT_PAIRS; ++p) {
                const ulonglong2 xb = lt_ld(a.ub + row, cl[p]), xa = lt_ld(a.ua + row, cl[p]);
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    typename Op::Sum sb, sa;
                    Op::mac(sb, Op::in(h ? xb.y : xb.x), pmod, 0, lc, P);
                    Op::mac(sa, Op::in(h ? xa.y : xa.x), pmod, 0, lc, P);
                    Op::addr(accb[p][h], sb, lc, P);
                    Op::addr(acca[p][h], sa, lc, P);
                }
            }
        }
    }
    u64 *ob = a.til + (((size_t)item * 2 + 0) * a.ext + slot) * n + dbase;
    u64 *oa = a.til + (((size_t)item * 2 + 1) * a.ext + slot) * n + dbase;
#pragma unroll
    for (int p = 0; p < LT_PAIRS; ++p) {
        if (c[p] < pairs) {
            reinterpret_cast<ulonglong2 *>(ob)[c[p]] =
                make_ulonglong2(Op::out(accb[p][0], lc, P), Op::out(accb[p][1], lc, P));
            reinterpret_cast<ulonglong2 *>(oa)[c[p]] =
                make_ulonglong2(Op::out(acca[p][0], lc, P), Op::out(acca[p][1], lc, P));
        }
    }
}

// the (group, member) of a workgroup under the args' grid order; grid.x = round_up(groups, 8) * members
template <class Args>
MK_D void lt_place(const Args &a, uint32_t &grp, uint32_t &m) {
    if (a.xcd_order) {  // ids congruent mod 8 share an XCD: a group's members follow each other there
        const uint32_t seq = blockIdx.x / LT_XCDS;
        m = seq % a.members;
        grp = (seq / a.members) * LT_XCDS + blockIdx.x % LT_XCDS;
    } else {
        const uint32_t padded = gridDim.x / a.members;
        m = blockIdx.x / padded;
        grp = blockIdx.x % padded;
    }
}

// a workgroup of k_lt_accum and of the two kernels of bsgs_kernels.hpp that share its tile
template <int NPARTS, int MODE, class Args>
MK_D void lt_block(const Args &a, const LimbConst *limb, ulonglong2 *lds) {
    uint32_t grp, m;
    lt_place(a, grp, m);
    if (grp >= a.groups) return;
    const uint32_t log_tiles = a.log_n - a.log_t;
    const uint32_t slot = grp >> log_tiles, dbase = (grp & ((1u << log_tiles) - 1u)) << a.log_t;
    const uint32_t id = limb_id_of(slot, a.nl, a.L);
    const LimbConst lc = limb[id];
    const uint32_t first = a.walk ? 0u : m, last = a.walk ? a.cnt : m + 1u;
    for (uint32_t item = first; item < last; ++item) {
        if (lc.fp) lt_tile<LT_FP, NPARTS, MODE>(a, lc, item, slot, id, dbase, lds);
        else if (lc.pm) lt_tile<LT_PM, NPARTS, MODE>(a, lc, item, slot, id, dbase, lds);
        else lt_tile<LT_INT, NPARTS, MODE>(a, lc, item, slot, id, dbase, lds);
    }
}

// NPARTS is the digit count of the level.  The body is lt_block's, written out: through the helper two instances compile
// to other register counts than profiles/linear_transform_static.txt records
template <int NPARTS>
__global__ __launch_bounds__(LT_THREADS) void k_lt_accum(LtArgs a, const LimbConst *limb) {
    __shared__ ulonglong2 lds[(NPARTS + 1) * LT_TILE_PAIRS];
    uint32_t grp, m;
    if (a.xcd_order) {  // ids congruent mod 8 share an XCD: a group's members follow each other there
        const uint32_t seq = blockIdx.x / LT_XCDS;
        m = seq % a.members;
        grp = (seq / a.members) * LT_XCDS + blockIdx.x % LT_XCDS;
    } else {
        const uint32_t padded = gridDim.x / a.members;
        m = blockIdx.x / padded;
        grp = blockIdx.x % padded;
    }
    if (grp >= a.groups) return;
    const uint32_t log_tiles = a.log_n - a.log_t;
    const uint32_t slot = grp >> log_tiles, dbase = (grp & ((1u << log_tiles) - 1u)) << a.log_t;
    const uint32_t id = limb_id_of(slot, a.nl, a.L);
    const LimbConst lc = limb[id];
    const uint32_t first = a.walk ? 0u : m, last = a.walk ? a.cnt : m + 1u;
    for (uint32_t item = first; item < last; ++item) {
        if (lc.fp) lt_tile<LT_FP, NPARTS>(a, lc, item, slot, id, dbase, lds);
        else if (lc.pm) lt_tile<LT_PM, NPARTS>(a, lc, item, slot, id, dbase, lds);
        else lt_tile<LT_INT, NPARTS>(a, lc, item, slot, id, dbase, lds);
    }
}
static_assert(LT_TILE_PAIRS == LT_PAIRS * LT_THREADS, "k_lt_accum: a thread's pairs are one LDS tile");

}  // namespace mk
