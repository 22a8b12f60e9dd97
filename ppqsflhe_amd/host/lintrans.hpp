// lintrans.hpp -- the diagonals of linearTransform: a public linear map on the slots by the diagonal method,
//     out[j] = sum_r diag_r[j] * in[(j + r) mod slots]        (upstream: EvalLinearTransform),
// read from {"diagonals": [{"step": r, "values": [...]}, ...]} (values zero padded to the slots; step 0 needs no key; a
// step may appear more than once) or built from an n x n matrix {"matrix": [[...], ...]} (--block: n a power of two, at
// most the slots) as the 2n - 1 masked diagonals that apply it to every aligned n-slot block:
//     diag_r[j] = M[j mod n][(j mod n) + r] where that column exists, else 0,    r = -(n - 1) .. n - 1.
// No dependency on the library: built on its own by lintrans_selftest.cpp.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "json.hpp"

namespace mkh {

constexpr size_t LINTRANS_MAX_DIAGONALS = 4096;

struct Diagonals {
    std::vector<int32_t> steps;
    std::vector<double> values;  // [steps.size()][slots], zero padded
    double max_abs_sum = 0;      // max over the slots j of sum_r |diag_r[j]|: what the headroom rule multiplies by
};

inline void diagonals_finish(Diagonals &d, size_t slots) {
    d.max_abs_sum = 0;
    for (size_t j = 0; j < slots; ++j) {
        double t = 0;
        for (size_t k = 0; k < d.steps.size(); ++k) t += std::fabs(d.values[k * slots + j]);
        d.max_abs_sum = std::fmax(d.max_abs_sum, t);
    }
}

// The diagonals of `doc` into `out`; the returned string is empty on success and the reason otherwise.
inline std::string parse_diagonals(const Json &doc, size_t slots, Diagonals &out) {
    Diagonals d;
    try {
        const Json &list = doc.at("diagonals");
        if (!list.is_array() || list.a.empty()) return "diagonals: not a non-empty array";
        if (list.a.size() > LINTRANS_MAX_DIAGONALS) return "diagonals: more than " + std::to_string(LINTRANS_MAX_DIAGONALS) + " entries";
        d.values.assign(list.a.size() * slots, 0.0);
        for (size_t k = 0; k < list.a.size(); ++k) {
            const Json &e = list.a[k];
            const long long step = e.at("step").as_int();
            if (step <= -(1ll << 30) || step >= (1ll << 30)) return "diagonals: step " + std::to_string(step) + " is out of range";
            const Json &vals = e.at("values");
            if (!vals.is_array()) return "diagonals: the values of step " + std::to_string(step) + " are not an array";
            if (vals.a.size() > slots)
                return "diagonals: step " + std::to_string(step) + " has " + std::to_string(vals.a.size()) + " values, the ring has " +
                       std::to_string(slots) + " slots";
            for (size_t j = 0; j < vals.a.size(); ++j) {
                const double v = vals.a[j].as_double();
                if (!std::isfinite(v)) return "diagonals: a value of step " + std::to_string(step) + " is not finite";
                d.values[k * slots + j] = v;
            }
            d.steps.push_back((int32_t)step);
        }
    } catch (const std::exception &e) {
        return std::string("diagonals: not a list of {step, values} (") + e.what() + ")";
    }
    diagonals_finish(d, slots);
    out = std::move(d);
    return "";
}

// The 2n - 1 masked diagonals of the n x n matrix of `doc`, steps -(n - 1) .. n - 1 in that order.
inline std::string block_diagonals(const Json &doc, size_t slots, Diagonals &out) {
    Diagonals d;
    try {
        const Json &m = doc.at("matrix");
        if (!m.is_array() || m.a.empty()) return "--block: matrix is not a non-empty array of rows";
        const size_t n = m.a.size();
        if ((n & (n - 1)) || n > slots)
            return "--block: the matrix has " + std::to_string(n) + " rows; a power of two of at most " + std::to_string(slots) + " is needed";
        std::vector<double> M(n * n);
        for (size_t i = 0; i < n; ++i) {
            const Json &row = m.a[i];
            if (!row.is_array() || row.a.size() != n) return "--block: row " + std::to_string(i) + " does not have " + std::to_string(n) + " entries";
            for (size_t c = 0; c < n; ++c) {
                M[i * n + c] = row.a[c].as_double();
                if (!std::isfinite(M[i * n + c])) return "--block: an entry of row " + std::to_string(i) + " is not finite";
            }
        }
        const long long nn = (long long)n;
        d.values.assign((2 * n - 1) * slots, 0.0);
        for (long long r = -(nn - 1); r <= nn - 1; ++r) {
            const size_t k = (size_t)(r + nn - 1);
            d.steps.push_back((int32_t)r);
            for (size_t j = 0; j < slots; ++j) {
                const long long i = (long long)(j % n), c = i + r;
                if (c >= 0 && c < nn) d.values[k * slots + j] = M[(size_t)i * n + (size_t)c];
            }
        }
    } catch (const std::exception &e) {
        return std::string("--block: not a matrix of numbers (") + e.what() + ")";
    }
    diagonals_finish(d, slots);
    out = std::move(d);
    return "";
}

inline std::string load_diagonals(const std::string &path, bool block, size_t slots, Diagonals &out) {
    Json doc;
    try {
        doc = Json::parse_file(path);
    } catch (const std::exception &) {
        return std::string(block ? "--block" : "diagonals") + ": could not read " + path;
    }
    return block ? block_diagonals(doc, slots, out) : parse_diagonals(doc, slots, out);
}

// The headroom rule of include/mkckks.h: log2(scale * sf * max_j sum_r |diag_r[j]|) < log_q - 1 (|values| <= 1 assumed).
inline std::string diagonals_headroom_error(double log2_scale, double log2_sf, double max_abs_sum, double log_q, unsigned nl) {
    if (max_abs_sum == 0.0) return "";
    const double need = log2_scale + log2_sf + std::log2(max_abs_sum);
    if (need < log_q - 1) return "";
    return "no headroom: the transform needs log2(scale * sf * max sum |diagonal|) = " + std::to_string(need) + " bits below the " +
           std::to_string(log_q - 1) + " of these " + std::to_string(nl) + "-limb ciphertexts";
}

}  // namespace mkh
