// slotweights.hpp -- the --slot-weights option of serverRound / aggregateEncryptedWeights: a plaintext weights_summary
// JSON in the schema encryptModelWeights reads ("layer", "shape", "mean", "std_dev", "values") whose numbers are the
// per-coordinate factors of the aggregate.  It is split and padded exactly as encryptModelWeights splits its input:
// "optimizer/" layers are skipped, mean and std_dev get one slot vector each, the values are cut into batchSize chunks
// and zero padded -- so every aggregated ciphertext finds its slot vector by (layer, shape, field, chunk).  The file
// holds the WHOLE factor: nothing multiplies by 1/n as well.  No dependency on the library: built on its own by
// slotweights_selftest.cpp.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "json.hpp"

namespace mkh {

struct SlotLayer {
    std::string layer;
    Json shape;
    double mean = 0, std_dev = 0;
    std::vector<double> values;
};
struct SlotWeightsFile {
    std::vector<SlotLayer> layers;
    double max_abs = 0;  // over every factor of the file
};

// The factors of `doc` into `out`; the returned string is empty on success and the reason otherwise (what follows
// "[round] ERROR: ").
inline std::string parse_slot_weights(const Json &doc, SlotWeightsFile &out) {
    SlotWeightsFile f;
    try {
        if (!doc.at("weights_summary").is_array()) return "--slot-weights: weights_summary is not an array";
        for (const Json &w : doc.at("weights_summary").a) {
            SlotLayer l;
            l.layer = w.at("layer").as_string();
            if (l.layer.rfind("optimizer/", 0) == 0) continue;
            l.shape = w.at("shape");
            l.mean = w.at("mean").as_double();
            l.std_dev = w.at("std_dev").as_double();
            const Json &vals = w.at("values");
            if (!vals.is_array()) return "--slot-weights: the values of layer " + l.layer + " are not an array";
            l.values.reserve(vals.a.size());
            for (const Json &v : vals.a) l.values.push_back(v.as_double());
            if (!std::isfinite(l.mean) || !std::isfinite(l.std_dev))
                return "--slot-weights: a factor of layer " + l.layer + " is not finite";
            f.max_abs = std::fmax(f.max_abs, std::fmax(std::fabs(l.mean), std::fabs(l.std_dev)));
            for (double v : l.values) {
                if (!std::isfinite(v)) return "--slot-weights: a factor of layer " + l.layer + " is not finite";
                f.max_abs = std::fmax(f.max_abs, std::fabs(v));
            }
            f.layers.push_back(std::move(l));
        }
    } catch (const std::exception &e) {
        return std::string("--slot-weights: not a weights_summary of numbers (") + e.what() + ")";
    }
    out = std::move(f);
    return "";
}
inline std::string load_slot_weights(const std::string &path, SlotWeightsFile &out) {
    Json doc;
    try {
        doc = Json::parse_file(path);
    } catch (const std::exception &) {
        return "--slot-weights: could not read " + path;
    }
    return parse_slot_weights(doc, out);
}

// The slot vector of one aggregated ciphertext into dst[slots] (zero padded): field 0 mean, 1 std_dev, 2 chunk `idx` of
// the values.  n_chunks: value ciphertexts the round's layer has; batch: values per ciphertext (the context's
// batchSize).  Empty on success, else the reason.
inline std::string slot_vector(const SlotWeightsFile &f, const std::string &layer, const Json &shape, int field, size_t idx,
                               size_t n_chunks, size_t batch, double *dst, size_t slots) {
    if (batch == 0 || batch > slots) return "--slot-weights: a batch of " + std::to_string(batch) + " values does not fit the slots";
    const SlotLayer *hit = nullptr;
    bool named = false;
    for (const SlotLayer &l : f.layers) {
        if (l.layer != layer) continue;
        named = true;
        if (l.shape == shape) {
            hit = &l;
            break;
        }
    }
    if (!named) return "--slot-weights: layer " + layer + " of the round is absent from the file";
    if (!hit) return "--slot-weights: layer " + layer + " has another shape in the file";
    const size_t have = hit->values.size() / batch + (hit->values.size() % batch ? 1 : 0);
    if (have != n_chunks)
        return "--slot-weights: layer " + layer + " has " + std::to_string(hit->values.size()) + " value(s) = " +
               std::to_string(have) + " ciphertext(s) in the file, the round has " + std::to_string(n_chunks);
    for (size_t k = 0; k < slots; ++k) dst[k] = 0.0;
    if (field == 0) dst[0] = hit->mean;
    else if (field == 1) dst[0] = hit->std_dev;
    else {
        if (idx >= n_chunks) return "--slot-weights: layer " + layer + " has no chunk " + std::to_string(idx);
        const size_t lo = idx * batch, hi = lo + batch < hit->values.size() ? lo + batch : hit->values.size();
        for (size_t k = lo; k < hi; ++k) dst[k - lo] = hit->values[k];
    }
    return "";
}

// The headroom rule of include/mkckks.h: before the rescale the coefficients are about scale * sf * max|factor| * |values|;
// refuse when not even |values| <= 1 fit the ciphertext's modulus of log_q bits.  An all-zero file needs no room.
inline std::string slot_headroom_error(double log2_scale, double log2_sf, double max_abs, double log_q, unsigned nl) {
    if (max_abs == 0.0) return "";
    const double need = log2_scale + log2_sf + std::log2(max_abs);
    if (need < log_q - 1) return "";
    return "--slot-weights: no headroom: the product needs log2(scale * sf * max|factor|) = " + std::to_string(need) +
           " bits below the " + std::to_string(log_q - 1) + " of these " + std::to_string(nl) + "-limb ciphertexts";
}

}  // namespace mkh
