// weights.hpp -- the --weights option of serverRound / aggregateEncryptedWeights: "w_1,...,w_n", one non-negative number
// per client in argument order, not all zero (sample counts can be passed as they are: they are normalised by their
// sum).  No dependency on the library: built on its own by weights_selftest.cpp.
#pragma once
#include <cerrno>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

namespace mkh {

// The weights of `text`, normalised to sum 1, into `out`; the returned string is empty on success and the reason
// otherwise (what follows "[round] ERROR: ").  n_clients: how many values there must be.
inline std::string parse_weights(const std::string &text, size_t n_clients, std::vector<double> &out) {
    std::vector<double> w;
    size_t pos = 0;
    for (;;) {
        const size_t end = text.find(',', pos);
        const std::string tok = text.substr(pos, end == std::string::npos ? std::string::npos : end - pos);
        // strtod would skip leading blanks and accept "nan", "inf", hexadecimal floats and a trailing rest
        if (tok.empty() || tok.size() > 64 || tok.find_first_not_of("0123456789.eE+-") != std::string::npos)
            return "--weights needs non-negative numbers separated by commas (got \"" + tok.substr(0, 64) + "\")";
        char *rest = nullptr;
        errno = 0;
        const double v = std::strtod(tok.c_str(), &rest);
        if (rest != tok.c_str() + tok.size() || !std::isfinite(v))
            return "--weights needs non-negative numbers separated by commas (got \"" + tok + "\")";
        if (std::signbit(v) && v != 0.0) return "--weights: a weight is negative (" + tok + ")";
        w.push_back(std::fabs(v));
        if (w.size() > n_clients && w.size() > 65536) break;  // a hostile list: the count is wrong anyway
        if (end == std::string::npos) break;
        pos = end + 1;
    }
    if (w.size() != n_clients)
        return "--weights has " + std::to_string(w.size()) + " value(s) for " + std::to_string(n_clients) + " client(s)";
    double top = 0.0;
    for (double v : w) top = std::fmax(top, v);
    if (top == 0.0) return "--weights must not all be zero";
    double sum = 0.0;
    for (double &v : w) {  // by the largest first: the sum of huge counts must not overflow
        v /= top;
        sum += v;
    }
    for (double &v : w) v /= sum;
    out = std::move(w);
    return "";
}

}  // namespace mkh
