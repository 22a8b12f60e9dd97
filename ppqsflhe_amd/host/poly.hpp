// poly.hpp -- the header bookkeeping of evalPoly (cc->EvalPoly; include/mkckks.h: "polynomial evaluation").
// The plan of a degree-d evaluation (B, G, the limbs it consumes), the header of the result, the --coeffs parser and the
// headroom rule.  The plan restates mkckks_poly_plan so that a degree that does not fit the input's limbs is refused, by
// the number of limbs it needs, before a device is opened (poly_selftest.cpp holds it against the formulas of the header;
// tests/test_poly_surface.py holds the library's against the same formulas).  No dependency on the library.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "product.hpp"

namespace mkh {

constexpr uint32_t POLY_MIN_DEGREE = 2, POLY_MAX_DEGREE = 63;

struct PolyPlan {
    uint32_t B = 0, G = 0, depth = 0, n_relin = 0;  // depth: limbs consumed, nl - nl_out
};

inline uint32_t poly_ceil_log2(uint32_t v) {
    uint32_t r = 0;
    while ((1u << r) < v) ++r;
    return r;
}

// B = the smallest power of two with B^2 >= d + 1, G = ceil((d + 1) / B); depth log2 B + ceil(log2(G - 1)) + 2
inline PolyPlan poly_plan(uint32_t degree) {
    PolyPlan p;
    p.B = 2;
    while (p.B * p.B < degree + 1) p.B *= 2;
    p.G = (degree + p.B) / p.B;
    p.depth = poly_ceil_log2(p.B) + poly_ceil_log2(p.G - 1) + 2;
    p.n_relin = (p.B - 1) + (p.G - 2) + 1;
    return p;
}

// "c0,c1,...,cd" -> coefficients; the error text (empty on success).  Every entry is a finite number, nothing may follow
// it; the degree is the index of the last entry (a zero leading coefficient keeps its place: the plan follows the list)
inline std::string parse_coeffs(const std::string &list, std::vector<double> &coef) {
    coef.clear();
    size_t pos = 0;
    while (pos <= list.size()) {
        const size_t end = std::min(list.find(',', pos), list.size());
        const std::string tok = list.substr(pos, end - pos);
        if (tok.empty()) return "--coeffs: empty entry " + std::to_string(coef.size());
        char *rest = nullptr;
        const double v = std::strtod(tok.c_str(), &rest);
        if (rest == tok.c_str() || *rest || !std::isfinite(v)) return "--coeffs: entry " + std::to_string(coef.size()) + " (" + tok + ") is not a finite number";
        coef.push_back(v);
        pos = end + 1;
    }
    if (coef.size() < POLY_MIN_DEGREE + 1 || coef.size() > POLY_MAX_DEGREE + 1)
        return "--coeffs: the degree must be in [2, 63], got " + std::to_string(coef.size()) + " coefficient(s)";
    return "";
}

// empty when a noiseScaleDeg-1 input of nl limbs holds the plan, else the refusal naming the limbs needed
inline std::string poly_fit_error(uint32_t degree, uint32_t nl) {
    const PolyPlan p = poly_plan(degree);
    if (nl >= p.depth + 1) return "";
    return "degree " + std::to_string(degree) + " needs " + std::to_string(p.depth + 1) + " limbs (depth " + std::to_string(p.depth) +
           " and one limb for the result), the input has " + std::to_string(nl);
}

// header of the result of a noiseScaleDeg-1 input: depth limbs dropped, the standard scale of the output's level
inline ProductMeta poly_result(const ProductMeta &in, const PolyPlan &p, double scale_out) {
    ProductMeta r = in;
    r.nl = in.nl - p.depth;
    r.level = in.level + p.depth;
    r.scale = scale_out;
    r.noise_deg = 1;
    return r;
}

// the headroom rule of include/mkckks.h: Sigma * sum_k |c_k| A^k < q_0 ... q_{nl_T-1} / 2 for |x| <= A, in bits;
// log2_sigma = log2(S_out q_{nl_T-1} q_{nl_T-2}), log2_q = the bits of the first nl_T limbs.  Empty when it holds
inline std::string poly_headroom_error(const std::vector<double> &coef, double max_abs, double log2_sigma, double log2_q) {
    if (!(max_abs > 0) || !std::isfinite(max_abs)) return "--max-abs needs a positive number";
    long double sum = 0, pw = 1;
    for (double c : coef) {
        sum += std::fabs((long double)c) * pw;
        pw *= max_abs;
    }
    const double need = log2_sigma + (sum > 0 ? (double)std::log2(sum) : -INFINITY);
    if (need < log2_q - 1) return "";
    return "no headroom: the outer sum needs " + std::to_string(need) + " bits (log2 of Sigma * sum |c_k| " + std::to_string(max_abs) +
           "^k) below the " + std::to_string(log2_q - 1) + " bits its limbs hold";
}

}  // namespace mkh
