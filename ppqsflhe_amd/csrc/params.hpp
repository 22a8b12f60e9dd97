// params.hpp -- host-side CKKS/RNS parameter set and CRT tables.
//
// Product-side counterpart of what OpenFHE builds in GenCryptoContext
// (reference server/src/genCC.cpp:32-79) and rebuilds on every
// Serial::DeserializeFromFile(cc) (changeCipherDomain.cpp:33 etc.):
// [upstream] ckksrns-parametergeneration.cpp (moduli selection, FLEXIBLEAUTOEXT),
// rns-cryptoparameters.cpp::PrecomputeCRTTables (HYBRID digits, special primes,
// base-conversion tables), ckksrns-cryptoparameters.cpp (scaling factors),
// nbtheory (FirstPrime/LastPrime/PreviousPrime/NextPrime, minimal RootOfUnity).
#pragma once
#include <cstdint>
#include <map>
#include <vector>

#include "modarith.hpp"

namespace mk {

// Number theory on the host.
u64 h_mulmod(u64 a, u64 b, u64 m);
u64 h_powmod(u64 a, u64 e, u64 m);
u64 h_invmod(u64 a, u64 m);
bool h_is_prime(u64 n);
u64 h_shoup(u64 w, u64 q);
u64 h_min_primitive_root(u64 order, u64 q);

// reduction constants of one modulus q (odd, 2^17 < q < 2^60) for ring dimension n; fp / pm are left 0 for the engine
LimbConst make_limb_const(u64 q, u64 n);
// NTT table entries of the twiddle w as the fp64 and the pseudo-Mersenne limbs hold them (the engine's tables and the
// arithmetic probe are built from these): (double) w and w / q as bit patterns; w << t and (w * 2^32 mod q) << t
void fp_table_entry(u64 w, u64 q, u64 &wd_bits, u64 &wq_bits);
void pm_table_entry(u64 w, const LimbConst &L, u64 &wt, u64 &wxt);

// Tables for one approximate base conversion (ApproxSwitchCRTBasis):
// source limbs S = {s_i}, target limbs T = {t_j}.
struct BaseConvTable {
    std::vector<uint32_t> src;   // limb ids (index into QP table)
    std::vector<uint32_t> dst;   // limb ids
    std::vector<u64> hatinv;     // [(S/s_i)^-1]_{s_i}
    std::vector<u64> hatinv_sh;  // Shoup companions
    std::vector<u64> hat;        // [S/s_i]_{t_j}, row-major [i][j]
};

// The fp64 form of a conversion matrix, as bit patterns of doubles: [S/s_i]_t and [S/s_i]_t / t, [n_in][n_out] each, then
// for source 0 alone [S/s_0 * 2^30]_t and its quotient by t, [n_out] each -- a packed 60-bit source x = lo + 2^30 hi
// meets an fp64-class target as lo [S/s_0]_t + hi [S/s_0 2^30]_t, two exact FMA products of 30-bit factors.
std::vector<u64> hat_as_doubles(const BaseConvTable &t, const std::vector<u64> &moduli);

// Plan of a fused Paterson-Stockmeyer evaluation (include/mkckks.h: "polynomial evaluation"): p(x) = sum_j sum_i
// c_{jB+i} x^i y^j with y = x^B.  baby_nl[i - 1] / giant_nl[j - 1]: limbs of x^i (0 < i < B) and y^j (0 < j < G).
constexpr uint32_t POLY_MAX_DEGREE = 63, POLY_MAX_B = 8;
struct PolyPlan {
    uint32_t B, G, nl_T, nl_out, n_relin, depth;
    uint32_t baby_nl[POLY_MAX_B - 1], giant_nl[POLY_MAX_B - 1];
};

struct ParamSet {
    uint32_t log_n = 0, n = 0;
    uint32_t L = 0, K = 0, D = 0;  // #Q limbs, #P limbs, L+K
    uint32_t alpha = 0, beta = 0;  // limbs per digit, digits at full level
    uint32_t mult_depth = 0, scaling_bits = 0, first_bits = 0, dnum = 0, aux_bits = 0, extra_bits = 0;
    std::vector<u64> moduli;       // D entries: Q then P
    std::vector<u64> roots;        // minimal primitive 2N-th roots
    std::vector<LimbConst> limb;   // per-limb reduction constants
    std::vector<double> sf, sf_big;

    // builds everything above; throws std::invalid_argument on unsupported input
    void generate(uint32_t log_n, uint32_t mult_depth, uint32_t scaling_bits, uint32_t first_bits,
                  uint32_t dnum, uint32_t aux_bits, uint32_t extra_bits);

    // psi^bitrev(k) (forward) or psi^-bitrev(k) (inverse) with Shoup companions, N entries each
    void twiddles(uint32_t limb_id, bool inverse, std::vector<u64> &w, std::vector<u64> &w_sh) const;

    // limb id (index into moduli) of slot i of a polynomial with nl Q-limbs (+K P-limbs when with_p)
    uint32_t limb_of(uint32_t i, uint32_t nl) const { return i < nl ? i : L + (i - nl); }
    uint32_t num_parts(uint32_t nl) const {
        uint32_t p = (nl + alpha - 1) / alpha;
        return p > beta ? beta : p;
    }

    // ModUp table of digit `part` of a ciphertext with nl limbs: digit limbs -> complement in Q_nl u P
    BaseConvTable modup_table(uint32_t nl, uint32_t part) const;
    // ModDown table: P -> first nl Q limbs
    BaseConvTable moddown_table(uint32_t nl) const;
    // N^-1 [(P/p_k)^-1]_{p_k}: what the inverse transform ahead of ModDown's conversion scales P limb k by
    u64 moddown_scale(uint32_t k) const;
    // modup_table with the constants of the P targets multiplied by moddown_scale: [S/s_i * sc_k]_{p_k}.  Everything
    // between ModUp's conversion into a P limb and ModDown's conversion out of it is linear mod p_k, so a flow that
    // converts with this table needs no scaling in its inverse transform of the P limbs.  Q targets are unchanged.
    BaseConvTable modup_table_pscaled(uint32_t nl, uint32_t part) const;
    // [P^-1]_{q_i} and [P]_{q_i}
    u64 p_inv_mod(uint32_t limb_id) const;
    u64 p_mod(uint32_t limb_id) const;
    // [q_l^-1]_{q_i}
    u64 q_inv_mod(uint32_t l, uint32_t i) const;
    // LeveledSHECKKSRNS::GetElementForEvalMult
    std::vector<u64> const_factors(uint32_t nl, uint32_t level, double operand) const;
    // the same integer reduced modulo all D limbs of QP (weighted aggregation: the constant meets the eval key's P
    // limbs too); the first nl entries are const_factors(nl, level, operand).  Throws std::invalid_argument unless
    // const_fits: operand finite and |operand * sf(level)| < 2^125 (the 128-bit conversion is undefined beyond)
    std::vector<u64> const_factors_qp(uint32_t level, double operand) const;
    bool const_fits(uint32_t level, double operand) const;
    // Lagrange coefficients at 0 of the 1-based evaluation points parties[0..n_active): out[a][l] =
    // prod_{m in set, m != parties[a]} m (m - parties[a])^-1 mod q_l over the L limbs of Q.  Indices outside
    // [1, LAGRANGE_MAX_PARTIES], a duplicate and an empty set throw std::invalid_argument
    static constexpr uint32_t LAGRANGE_MAX_PARTIES = 64;
    void lagrange_at_zero(const uint32_t *parties, uint32_t n_active, u64 *out) const;
    // polynomial evaluation, host side.  Every scale below is the same few double operations in a fixed order (a product
    // then a quotient, never a multiply-add), so a restatement in another language gives the same bits.
    //   power_ladder: limbs and scales of z^1 .. z^n_pow from z at nl limbs and scale_in: with i = ceil(k / 2), j = k - i,
    //                 nl_k = nl_i - 1 and S_k = S_i * S_j / q_{nl_i - 1}.  Throws unless 1 <= n_pow <= 64 and every nl_k >= 1
    //   poly_plan:    throws for a degree outside [2, 63], nl outside [1, L] or nl_out < 1
    //   poly_weights: w[j * B + i] = c_{jB+i} * (Sigma / (S_{x^i} * S_{y^j})) with Sigma = S_out * q_{nl_T-1} * q_{nl_T-2};
    //                 returns S_out = sf(L - nl_out).  Throws on a non-finite coefficient
    //   poly_constants: out[k * nl_T + t] = rint(w[k]) mod q_t (a negative one as q - (|M| mod q)); throws on a non-finite
    //                 w or |w| >= q_0 ... q_{nl_T-1} / 2
    void power_ladder(uint32_t nl, uint32_t n_pow, double scale_in, uint32_t *nl_out, double *scale_out) const;
    PolyPlan poly_plan(uint32_t degree, uint32_t nl) const;
    double poly_weights(const double *coef, uint32_t degree, uint32_t nl, double scale_in, double *w) const;
    std::vector<u64> poly_constants(const double *w, uint32_t count, uint32_t nl_T) const;
    // Chebyshev series (include/mkckks.h: "Chebyshev series"): p(u) = sum_k c_k T_k(u) as sum_j sum_i m_{j,i} T_i T_{jB}.
    //   cheb_weights: the top-down block rewrite of c into m[G][B] in the header's fixed order, then poly_weights on m with
    //                 the plan, limbs and scale of u (the Chebyshev ladder has the power ladder's limbs and scales);
    //                 returns S_out.  Throws on a non-finite coefficient and on everything poly_plan refuses
    double cheb_weights(const double *coef, uint32_t degree, uint32_t nl, double scale_in, double *w) const;
};

}  // namespace mk
