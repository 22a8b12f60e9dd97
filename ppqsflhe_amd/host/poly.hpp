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

// ---- Chebyshev series (evalPoly --cheb a,b; include/mkckks.h: "Chebyshev series") -------------------------------------------

// "a,b" -> the interval; the error text (empty on success)
inline std::string parse_interval(const std::string &s, double &a, double &b) {
    const size_t comma = s.find(',');
    if (comma == std::string::npos) return "--cheb needs an interval a,b";
    const std::string sa = s.substr(0, comma), sb = s.substr(comma + 1);
    char *ra = nullptr, *rb = nullptr;
    a = std::strtod(sa.c_str(), &ra);
    b = std::strtod(sb.c_str(), &rb);
    if (sa.empty() || sb.empty() || *ra || *rb || !std::isfinite(a) || !std::isfinite(b)) return "--cheb needs an interval a,b of two finite numbers";
    if (!(a < b)) return "--cheb needs a < b";
    return "";
}

// whether the interval costs a level: everything but exactly [-1, 1] is mapped onto it by one constant product and a rescale
inline bool cheb_mapped(double a, double b) { return !(a == -1.0 && b == 1.0); }

// the functions --function knows; nullptr for any other name
typedef double (*ChebFn)(double);
inline ChebFn cheb_function(const std::string &name) {
    if (name == "invsqrt") return [](double t) { return 1.0 / std::sqrt(t); };
    if (name == "sigmoid") return [](double t) { return 1.0 / (1.0 + std::exp(-t)); };
    if (name == "tanh") return [](double t) { return std::tanh(t); };
    if (name == "exp") return [](double t) { return std::exp(t); };
    return nullptr;
}

// empty when --function name --degree d on [a, b] can be fitted, else the refusal
inline std::string cheb_function_error(const std::string &name, uint32_t degree, double a, double /*b*/) {
    if (!cheb_function(name)) return "--function: unknown function " + name + " (invsqrt, sigmoid, tanh, exp)";
    if (degree < POLY_MIN_DEGREE || degree > POLY_MAX_DEGREE) return "--degree: the degree must be in [2, 63], got " + std::to_string(degree);
    if (name == "invsqrt" && !(a > 0)) return "--function invsqrt needs an interval with a > 0";
    return "";
}

// the series that interpolates f at the d + 1 Chebyshev nodes of [a, b] (upstream's EvalChebyshevFunction; the sums of
// numpy.polynomial.chebyshev.chebinterpolate): u_k = sin(pi (2k - d) / (2 (d + 1))), k = 0 .. d,
// c_j = (2 / (d + 1)) sum_k f(x(u_k)) T_j(u_k), c_0 halved: the plain coefficient of T_0
inline std::vector<double> cheb_fit(ChebFn f, double a, double b, uint32_t degree) {
    const uint32_t n = degree + 1;
    const double pi = 3.14159265358979323846;
    std::vector<double> y(n), u(n), c(n, 0.0);
    for (uint32_t k = 0; k < n; ++k) {
        u[k] = std::sin(0.5 * pi / n * (2.0 * k - degree));
        y[k] = f(0.5 * ((b - a) * u[k] + (a + b)));
    }
    for (uint32_t k = 0; k < n; ++k) {
        double t0 = 1.0, t1 = u[k];  // T_j(u_k) by the three-term recurrence
        c[0] += y[k];
        for (uint32_t j = 1; j < n; ++j) {
            c[j] += y[k] * t1;
            const double t2 = 2.0 * u[k] * t1 - t0;
            t0 = t1;
            t1 = t2;
        }
    }
    c[0] /= n;
    for (uint32_t j = 1; j < n; ++j) c[j] /= 0.5 * n;
    return c;
}

// sum_k c_k T_k(u) by Clenshaw's recurrence (the self-test's reference for the rewrite and the fit)
inline double cheb_value(const std::vector<double> &c, double u) {
    double b1 = 0, b2 = 0;
    for (size_t k = c.size(); k-- > 1;) {
        const double b0 = c[k] + 2 * u * b1 - b2;
        b2 = b1;
        b1 = b0;
    }
    return c[0] + u * b1 - b2;
}

// the block rewrite of mkckks.h, in its order: m[j * B + i] with sum_k c_k T_k = sum_j sum_i m_{j,i} T_i T_{jB}
inline std::vector<double> cheb_rewrite(const std::vector<double> &coef, uint32_t B, uint32_t G) {
    std::vector<double> c((size_t)B * G, 0.0), m((size_t)B * G, 0.0);
    std::copy(coef.begin(), coef.end(), c.begin());
    for (uint32_t j = G - 1; j >= 1; --j) {
        for (uint32_t i = B - 1; i >= 1; --i) {
            m[j * B + i] = 2.0 * c[j * B + i];
            c[(j - 1) * B + (B - i)] -= c[j * B + i];
        }
        m[j * B] = c[j * B];
    }
    for (uint32_t i = 0; i < B; ++i) m[i] = c[i];
    return m;
}

// empty when a noiseScaleDeg-1 input of nl limbs holds the series' plan (one limb more when the interval is mapped)
inline std::string cheb_fit_error(uint32_t degree, uint32_t nl, bool mapped) {
    const PolyPlan p = poly_plan(degree);
    const uint32_t need = p.depth + 1 + (mapped ? 1 : 0);
    if (nl >= need) return "";
    return "degree " + std::to_string(degree) + " needs " + std::to_string(need) + " limbs (depth " + std::to_string(need - 1) +
           (mapped ? ", the map onto [-1, 1] included," : "") + " and one limb for the result), the input has " + std::to_string(nl);
}

// the headroom rule of the Chebyshev block: |T_k| <= 1 on the interval, so Sigma * sum |m_{j,i}| < q_0 ... q_{nl_T-1} / 2
// suffices, in bits; *need_bits (nullable) receives the left side.  Empty when it holds
inline std::string cheb_headroom_error(const std::vector<double> &m, double log2_sigma, double log2_q, double *need_bits) {
    long double sum = 0;
    for (double v : m) sum += std::fabs((long double)v);
    const double need = log2_sigma + (sum > 0 ? (double)std::log2(sum) : -INFINITY);
    if (need_bits) *need_bits = need;
    if (need < log2_q - 1) return "";
    return "no headroom: the outer sum needs " + std::to_string(need) + " bits (log2 of Sigma * sum |m_{j,i}|) below the " +
           std::to_string(log2_q - 1) + " bits its limbs hold";
}

}  // namespace mkh
