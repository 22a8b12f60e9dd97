// slotweights_selftest -- stand-alone checks of the --slot-weights host code (slotweights.hpp), built plain and under
// AddressSanitizer + UBSan (make slotweights-asan; driven by tests/test_slot_weights_surface.py):
//   * the mapping from a plaintext weights_summary file to the slot vector of every aggregated ciphertext -- optimizer
//     layers skipped, mean / std_dev in slot 0, values cut into batchSize chunks and zero padded -- on boundary inputs
//     (a last chunk of one value, of exactly batchSize values, no values at all, a batch as large as the slots);
//   * its refusals: an absent layer, another shape, another value count, factors that are not finite, no weights_summary;
//   * the headroom rule on both sides of its bound.
// Needs no device and no library.
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "slotweights.hpp"

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

using mkh::Json;
using mkh::SlotWeightsFile;

static std::string layer_json(const std::string &name, const std::string &shape, const std::string &mean, const std::string &sd,
                              const std::vector<double> &values) {
    std::string t = "{\"layer\": \"" + name + "\", \"shape\": " + shape + ", \"mean\": " + mean + ", \"std_dev\": " + sd + ", \"values\": [";
    for (size_t i = 0; i < values.size(); ++i) {
        char buf[40];
        std::snprintf(buf, sizeof buf, "%s%.17g", i ? ", " : "", values[i]);
        t += buf;
    }
    return t + "]}";
}
static std::string doc_json(const std::vector<std::string> &layers) {
    std::string t = "{\"weights_summary\": [";
    for (size_t i = 0; i < layers.size(); ++i) t += (i ? ", " : "") + layers[i];
    return t + "]}";
}
static std::string parse(const std::string &text, SlotWeightsFile &f) {
    Json doc;
    try {
        doc = Json::parse(text);
    } catch (const std::exception &) {
        return "unparsable";
    }
    return mkh::parse_slot_weights(doc, f);
}

static void check_mapping() {
    std::vector<double> v9;
    for (int i = 0; i < 9; ++i) v9.push_back(1.0 / (i + 1));
    SlotWeightsFile f;
    EXPECT(parse(doc_json({layer_json("dense/kernel", "[3, 3]", "0.25", "-2", v9), layer_json("optimizer/iter", "[]", "1e999", "0", {}),
                           layer_json("dense/bias", "[4]", "1", "0", {0.5, 0.0, 1.0, 1.0 / 3.0}), layer_json("empty", "[0]", "0", "0", {})}),
                 f).empty());
    EXPECT(f.layers.size() == 3 && f.max_abs == 2.0);  // the optimizer layer (and its infinite mean) is skipped
    const Json s33 = Json::parse("[3, 3]"), s4 = Json::parse("[4]"), s0 = Json::parse("[0]");
    const size_t slots = 8;
    std::vector<double> d(slots + 1, 7.0);  // one guard word
    // batch 4: 9 values = chunks of 4, 4, 1
    EXPECT(mkh::slot_vector(f, "dense/kernel", s33, 0, 0, 3, 4, d.data(), slots).empty() && d[0] == 0.25 && d[1] == 0 && d[7] == 0);
    EXPECT(mkh::slot_vector(f, "dense/kernel", s33, 1, 0, 3, 4, d.data(), slots).empty() && d[0] == -2.0 && d[1] == 0);
    EXPECT(mkh::slot_vector(f, "dense/kernel", s33, 2, 0, 3, 4, d.data(), slots).empty() && d[0] == 1.0 && d[3] == 0.25 && d[4] == 0);
    EXPECT(mkh::slot_vector(f, "dense/kernel", s33, 2, 1, 3, 4, d.data(), slots).empty() && d[0] == 0.2 && d[3] == 0.125 && d[4] == 0);
    EXPECT(mkh::slot_vector(f, "dense/kernel", s33, 2, 2, 3, 4, d.data(), slots).empty() && d[0] == 1.0 / 9 && d[1] == 0 && d[7] == 0);
    EXPECT(!mkh::slot_vector(f, "dense/kernel", s33, 2, 3, 3, 4, d.data(), slots).empty());  // no chunk 3
    // a last chunk of exactly batchSize values; a batch as large as the slots; a batch of one
    EXPECT(mkh::slot_vector(f, "dense/bias", s4, 2, 0, 1, 4, d.data(), slots).empty() && d[3] == 1.0 / 3 && d[4] == 0);
    EXPECT(mkh::slot_vector(f, "dense/bias", s4, 2, 0, 1, 8, d.data(), slots).empty() && d[2] == 1.0 && d[4] == 0);
    EXPECT(mkh::slot_vector(f, "dense/bias", s4, 2, 3, 4, 1, d.data(), slots).empty() && d[0] == 1.0 / 3 && d[1] == 0);
    EXPECT(mkh::slot_vector(f, "dense/kernel", s33, 2, 1, 2, 8, d.data(), slots).empty() && d[0] == 1.0 / 9 && d[1] == 0);
    EXPECT(mkh::slot_vector(f, "empty", s0, 0, 0, 0, 4, d.data(), slots).empty() && d[0] == 0);  // mean / std_dev only
    EXPECT(d[slots] == 7.0);
    // refusals, with the messages the hosts print
    EXPECT(mkh::slot_vector(f, "dense/other", s4, 0, 0, 1, 4, d.data(), slots).find("absent from the file") != std::string::npos);
    EXPECT(mkh::slot_vector(f, "optimizer/iter", Json::parse("[]"), 0, 0, 0, 4, d.data(), slots).find("absent") != std::string::npos);
    EXPECT(mkh::slot_vector(f, "dense/bias", s33, 0, 0, 1, 4, d.data(), slots).find("another shape") != std::string::npos);
    EXPECT(mkh::slot_vector(f, "dense/bias", s4, 2, 0, 2, 4, d.data(), slots).find("the round has 2") != std::string::npos);
    EXPECT(mkh::slot_vector(f, "dense/kernel", s33, 0, 0, 2, 4, d.data(), slots).find("9 value(s) = 3 ciphertext(s)") != std::string::npos);
    EXPECT(!mkh::slot_vector(f, "dense/bias", s4, 0, 0, 1, 0, d.data(), slots).empty());   // no batch
    EXPECT(!mkh::slot_vector(f, "dense/bias", s4, 0, 0, 1, 9, d.data(), slots).empty());   // a batch beyond the slots
    EXPECT(d[slots] == 7.0);
    // two layers of one name: the shape decides
    SlotWeightsFile g;
    EXPECT(parse(doc_json({layer_json("w", "[2]", "1", "1", {1, 2}), layer_json("w", "[3]", "2", "2", {3, 4, 5})}), g).empty());
    EXPECT(mkh::slot_vector(g, "w", Json::parse("[3]"), 2, 0, 1, 4, d.data(), slots).empty() && d[2] == 5.0 && g.max_abs == 5.0);
    std::printf("ok mapping\n");
}

static void check_parser() {
    SlotWeightsFile f;
    EXPECT(parse("{\"weights_summary\": []}", f).empty() && f.layers.empty() && f.max_abs == 0.0);
    EXPECT(!parse("{}", f).empty() && !parse("[]", f).empty() && !parse("{\"weights_summary\": 3}", f).empty());
    EXPECT(!parse(doc_json({"{\"layer\": \"a\", \"shape\": [1], \"mean\": 1, \"std_dev\": 1}"}), f).empty());          // no values
    EXPECT(!parse(doc_json({"{\"layer\": \"a\", \"shape\": [1], \"mean\": \"1\", \"std_dev\": 1, \"values\": []}"}), f).empty());
    EXPECT(!parse(doc_json({"{\"layer\": \"a\", \"shape\": [1], \"mean\": 1, \"std_dev\": 1, \"values\": [1, \"x\"]}"}), f).empty());
    EXPECT(!parse(doc_json({"{\"layer\": \"a\", \"shape\": [1], \"mean\": 1, \"std_dev\": 1, \"values\": 1}"}), f).empty());
    EXPECT(!parse(doc_json({"{\"layer\": 5, \"shape\": [1], \"mean\": 1, \"std_dev\": 1, \"values\": []}"}), f).empty());
    // factors that are not finite: 1e999 reads as infinity
    EXPECT(parse(doc_json({layer_json("a", "[1]", "1e999", "0", {1})}), f).find("not finite") != std::string::npos);
    EXPECT(parse(doc_json({layer_json("a", "[1]", "0", "-1e999", {1})}), f).find("not finite") != std::string::npos);
    EXPECT(parse(doc_json({"{\"layer\": \"a\", \"shape\": [1], \"mean\": 0, \"std_dev\": 0, \"values\": [1, 1e999]}"}), f).find("not finite") !=
           std::string::npos);
    EXPECT(!parse(doc_json({"{\"layer\": \"a\", \"shape\": [1], \"mean\": NaN, \"std_dev\": 0, \"values\": []}"}), f).empty());
    EXPECT(f.layers.empty());  // a refused file leaves the output as it was
    EXPECT(mkh::load_slot_weights("/nonexistent/slot-weights.json", f).find("could not read") != std::string::npos);
    // large and tiny factors are factors
    EXPECT(parse(doc_json({layer_json("a", "[2]", "1e300", "5e-324", {-1e308, 0})}), f).empty() && f.max_abs == 1e308);
    std::printf("ok parser\n");
}

static void check_headroom() {
    // about the reference's shape: log2(scale * sf) = 99 against 159 bits of Q: room for factors below 2^59
    const double log_q = 159.0;
    EXPECT(mkh::slot_headroom_error(59.0, 40.0, 1.0, log_q, 4).empty());
    EXPECT(mkh::slot_headroom_error(59.0, 40.0, std::ldexp(1.0, 58), log_q, 4).empty());
    EXPECT(!mkh::slot_headroom_error(59.0, 40.0, std::ldexp(1.0, 59), log_q, 4).empty());   // need == log_q - 1: refused
    EXPECT(mkh::slot_headroom_error(59.0, 40.0, std::ldexp(1.0, 59) * 0.999, log_q, 4).empty());
    EXPECT(mkh::slot_headroom_error(59.0, 40.0, 1e308, log_q, 4).find("no headroom") != std::string::npos);
    // small factors give room back; an all-zero file needs none
    EXPECT(!mkh::slot_headroom_error(80.0, 40.0, 1.0, 120.0, 2).empty());
    EXPECT(mkh::slot_headroom_error(80.0, 40.0, std::ldexp(1.0, -2), 120.0, 2).empty());
    EXPECT(mkh::slot_headroom_error(80.0, 40.0, 0.0, 10.0, 1).empty());
    EXPECT(mkh::slot_headroom_error(80.0, 40.0, 5e-324, 120.0, 2).empty());
    std::printf("ok headroom\n");
}

int main() {
    check_mapping();
    check_parser();
    check_headroom();
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("ok slotweights selftest\n");
    return 0;
}
