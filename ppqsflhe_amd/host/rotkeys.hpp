// rotkeys.hpp -- the rotation-key file of rotKeyGen / slotSum: the Galois keys a server needs for its rotations and slot
// sums, in one file.  Upstream keeps them in the CryptoContext's EvalAutomorphismKeyMap (cc->EvalRotateKeyGen /
// cc->EvalSumKeyGen, serialised by SerializeEvalAutomorphismKey); the reference calls none of them.
// Layout: BlobHeader (kind 9, limbs = D, parts = 2 beta, slots = number of entries), then per entry one u64 holding the
// Galois element g followed by the key u64[beta][2][D][N] of mkckks_galois_keygen(g).  Nothing in the file is secret.
#pragma once
#include <map>

#include "hostlib.hpp"

namespace mkh {

enum : uint32_t { KIND_ROTKEYS = 9 };

struct RotKeys {
    std::map<uint32_t, std::vector<uint64_t>> keys;  // Galois element -> key
};

// kind: KIND_ROTKEYS, or the rotation-key share's (evalkeys.hpp: one party's part of a joint key's keys, same layout)
inline void write_rot_keys(const std::string &path, const RotKeys &rk, uint32_t ring_dim, uint32_t limbs, uint32_t parts,
                           uint32_t kind = KIND_ROTKEYS) {
    BlobHeader h{};
    std::memcpy(h.magic, "MKCK", 4);
    h.version = 1; h.kind = kind; h.ring_dim = ring_dim; h.limbs = limbs; h.parts = parts;
    h.slots = (uint32_t)rk.keys.size();
    std::unique_ptr<FILE, FileCloser> f(std::fopen(path.c_str(), "wb"));
    if (!f) throw std::runtime_error("cannot write " + path);
    bool ok = std::fwrite(&h, sizeof h, 1, f.get()) == 1;
    for (const auto &kv : rk.keys) {
        const uint64_t g = kv.first;
        ok = ok && std::fwrite(&g, 8, 1, f.get()) == 1 && std::fwrite(kv.second.data(), 8, kv.second.size(), f.get()) == kv.second.size();
    }
    if (!ok) throw std::runtime_error("cannot write " + path);
}

// the error text, empty on success
inline std::string read_rot_keys(const std::string &path, uint32_t ring_dim, uint32_t limbs, uint32_t parts, RotKeys &out,
                                 uint32_t kind = KIND_ROTKEYS) {
    std::unique_ptr<FILE, FileCloser> f(std::fopen(path.c_str(), "rb"));
    if (!f) return "cannot open rotation keys " + path;
    BlobHeader h{};
    if (std::fread(&h, sizeof h, 1, f.get()) != 1 || std::memcmp(h.magic, "MKCK", 4) || h.version != 1 || h.kind != kind) {
        // one party's share of a joint key's rotation keys (kind 11, evalkeys.hpp) used as a key would give noise
        if (kind == KIND_ROTKEYS && !std::memcmp(h.magic, "MKCK", 4) && h.version == 1 && h.kind == 11)
            return path + " is a rotation-key share, not a rotation-key file (fuseEvalKeys sums the parties' shares into one)";
        return path + " is not a rotation-key file";
    }
    if (h.ring_dim != ring_dim || h.limbs != limbs || h.parts != parts) return "rotation keys do not match the CryptoContext";
    if (h.slots > 64) return "rotation-key file claims " + std::to_string(h.slots) + " entries (at most 64)";
    const size_t words = (size_t)parts * limbs * ring_dim;
    out.keys.clear();
    for (uint32_t i = 0; i < h.slots; ++i) {
        uint64_t g = 0;
        if (std::fread(&g, 8, 1, f.get()) != 1) return "rotation-key file is truncated";
        if (!(g & 1) || g >= 2ull * ring_dim) return "rotation-key file holds the invalid Galois element " + std::to_string(g);
        std::vector<uint64_t> &key = out.keys[(uint32_t)g];
        if (!key.empty()) return "rotation-key file holds Galois element " + std::to_string(g) + " twice";
        key.resize(words);
        if (std::fread(key.data(), 8, words, f.get()) != words) return "rotation-key file is truncated";
    }
    if (std::fgetc(f.get()) != EOF) return "rotation-key file has bytes after its last entry";
    return "";
}

// a decimal integer with optional sign, |v| < 2^30; false on anything else
inline bool parse_step(const std::string &v, int32_t &out) {
    const size_t start = (!v.empty() && (v[0] == '-' || v[0] == '+')) ? 1 : 0;
    if (v.size() == start || v.size() - start > 9 || v.find_first_not_of("0123456789", start) != std::string::npos) return false;
    out = (int32_t)std::atol(v.c_str());
    return true;
}

// the rotation steps of a slot sum over `span` slots: 1, 2, 4, ... below span
inline std::vector<int32_t> sum_steps(uint32_t span) {
    std::vector<int32_t> r;
    for (uint32_t st = 1; st < span; st <<= 1) r.push_back((int32_t)st);
    return r;
}

}  // namespace mkh
