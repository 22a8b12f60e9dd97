// bsgs.hpp -- the baby-step giant-step plan of linearTransform --bsgs (include/mkckks.h: mkckks_linear_transform_bsgs_batch).
// Every step r of the diagonals (lintrans.hpp) is reduced to (-slots/2, slots/2] (values of a repeated step are summed)
// and written as r = G + b with b = r mod n1 by the floor modulus, 0 <= b < n1, and G = r - b.  Then
//     out = sum_G rot_G( sum_b p_{G,b} * rot_b(x) ),     p_{G,b}[k] = diag_{G+b}[(k - G) mod slots]
// (the diagonal rolled RIGHT by G: rot_G undoes the roll), and the keys needed are those of the distinct non-zero b and
// the distinct non-zero G: about n1 + n2 where the direct method needs one per step.
// `auto` picks the power of two n1 in [2, 64] with the fewest keys; ties go to the larger n1 (a giant costs a ModDown
// and a ModUp, a baby does not).
// No dependency on the library: built on its own by bsgs_selftest.cpp.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <map>
#include <set>

#include "lintrans.hpp"

namespace mkh {

constexpr uint32_t BSGS_MAX = 64;  // MKCKKS_BSGS_MAX

struct BsgsPlan {
    uint32_t n1 = 0;
    std::vector<int32_t> babies;   // n1 baby steps 0 .. n1 - 1, in the order of the call
    std::vector<int32_t> giants;   // the distinct giant steps, ascending
    std::vector<uint8_t> present;  // [giants][n1]
    std::vector<double> values;    // [giants][n1][slots]: the rolled diagonals (absent entries zero); empty without values
    std::vector<int32_t> key_steps;  // distinct non-zero baby steps (ascending), then distinct non-zero giant steps not among them
    size_t n_babies = 0, n_giants = 0;  // the distinct non-zero ones: the keys
};

inline long long bsgs_reduce_step(long long r, long long slots) {
    long long m = ((r % slots) + slots) % slots;  // [0, slots)
    return m > slots / 2 ? m - slots : m;         // (-slots/2, slots/2]
}

inline long long bsgs_floor_mod(long long r, long long n1) { return ((r % n1) + n1) % n1; }

// (distinct non-zero b) and (distinct non-zero G) of reduced steps under n1
inline void bsgs_counts(const std::set<long long> &steps, uint32_t n1, size_t &nb, size_t &ng, size_t &all_g) {
    std::set<long long> bs, gs;
    for (long long r : steps) {
        const long long b = bsgs_floor_mod(r, n1);
        bs.insert(b);
        gs.insert(r - b);
    }
    all_g = gs.size();
    nb = bs.size() - bs.count(0);
    ng = gs.size() - gs.count(0);
}

inline uint32_t bsgs_auto_n1(const std::set<long long> &steps) {
    uint32_t best = 2;
    size_t best_keys = (size_t)-1;
    for (uint32_t n1 = 2; n1 <= BSGS_MAX; n1 *= 2) {
        size_t nb, ng, all_g;
        bsgs_counts(steps, n1, nb, ng, all_g);
        if (nb + ng <= best_keys) {  // ties: the larger n1
            best_keys = nb + ng;
            best = n1;
        }
    }
    return best;
}

// "<n1>" or "auto" -> n1 (0: auto); the returned string is empty on success and the reason otherwise
inline std::string bsgs_parse_n1(const std::string &arg, uint32_t &n1) {
    if (arg == "auto") {
        n1 = 0;
        return "";
    }
    char *end = nullptr;
    const long v = arg.empty() ? 0 : std::strtol(arg.c_str(), &end, 10);
    if (arg.empty() || *end || v < 1 || v > 1000000) return "--bsgs: '" + arg + "' is neither a baby-step count nor auto";
    n1 = (uint32_t)v;
    return "";
}

// The plan of `d` under n1 (0: auto); with_values = false leaves `values` empty (the key list needs none).
inline std::string bsgs_plan(const Diagonals &d, size_t slots, uint32_t n1, bool with_values, BsgsPlan &out) {
    const long long S = (long long)slots;
    std::map<long long, std::vector<size_t>> by_step;  // reduced step -> the entries of d that have it
    std::set<long long> steps;
    for (size_t k = 0; k < d.steps.size(); ++k) {
        const long long r = bsgs_reduce_step(d.steps[k], S);
        by_step[r].push_back(k);
        steps.insert(r);
    }
    if (steps.empty()) return "--bsgs: no diagonals";
    BsgsPlan p;
    p.n1 = n1 ? n1 : bsgs_auto_n1(steps);
    size_t all_g = 0;
    bsgs_counts(steps, p.n1, p.n_babies, p.n_giants, all_g);
    if (p.n1 > BSGS_MAX || all_g > BSGS_MAX)
        return "--bsgs: a plan of " + std::to_string(p.n1) + " baby steps and " + std::to_string(all_g) +
               " giant steps; at most " + std::to_string(BSGS_MAX) + " of either are supported";
    std::set<long long> gs;
    for (long long r : steps) gs.insert(r - bsgs_floor_mod(r, p.n1));
    for (uint32_t b = 0; b < p.n1; ++b) p.babies.push_back((int32_t)b);
    for (long long G : gs) p.giants.push_back((int32_t)G);
    p.present.assign(p.giants.size() * p.n1, 0);
    if (with_values) p.values.assign(p.giants.size() * p.n1 * slots, 0.0);
    std::set<long long> used_b;
    for (const auto &kv : by_step) {
        const long long r = kv.first, b = bsgs_floor_mod(r, p.n1), G = r - b;
        const size_t t = (size_t)(std::lower_bound(p.giants.begin(), p.giants.end(), (int32_t)G) - p.giants.begin());
        p.present[t * p.n1 + (size_t)b] = 1;
        used_b.insert(b);
        if (!with_values) continue;
        double *dst = p.values.data() + (t * p.n1 + (size_t)b) * slots;
        for (size_t k : kv.second) {
            const double *src = d.values.data() + k * slots;
            for (long long j = 0; j < S; ++j) dst[j] += src[(size_t)bsgs_floor_mod(j - G, S)];
        }
    }
    std::set<long long> listed;
    for (long long b : used_b)
        if (b && listed.insert(b).second) p.key_steps.push_back((int32_t)b);
    for (long long G : gs)
        if (G && listed.insert(G).second) p.key_steps.push_back((int32_t)G);
    out = std::move(p);
    return "";
}

// the line of linearTransform --bsgs-steps: what rotKeyGen --steps takes
inline std::string bsgs_steps_line(const BsgsPlan &p) {
    std::string s = "[lintrans] bsgs n1=" + std::to_string(p.n1) + " babies=" + std::to_string(p.n_babies) +
                    " giants=" + std::to_string(p.n_giants) + " steps=";
    for (size_t k = 0; k < p.key_steps.size(); ++k) s += (k ? "," : "") + std::to_string(p.key_steps[k]);
    return s;
}

}  // namespace mkh
