// evalkeys.hpp -- the container kinds and the matching rules of the collective evaluation keys (rotKeyGen --share,
// relinKeyGen --share, fuseEvalKeys).  Upstream: MultiEvalAtIndexKeyGen / MultiEvalSumKeyGen +
// MultiAddEvalAutomorphismKeys, and MultiKeySwitchGen + MultiAddEvalKeys + MultiMultEvalKey + MultiAddEvalMultKeys; the
// reference calls none of them.
// A share travels in the container of the key it becomes, under a kind of its own, so that a lone share is refused by
// name where a key is asked for (a share used as a key gives noise and no error):
//   kind 11 rotation-key share       layout of the rotation-key file (rotkeys.hpp, kind 9): entries (g, key)
//   kind 12 relinearisation-key share  layout of the eval-key container (hostlib.hpp): one key u64[beta][2][D][N]
// Sums (fuseEvalKeys): re-encryption keys (kind 4) -> a re-encryption key (the round-1 key K1); kind 11 -> kind 9, entries
// matched by g; kind 12 -> kind 10.  No dependency on the library: built on its own by evalkeys_selftest.cpp.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "product.hpp"

namespace mkh {

enum : uint32_t { KIND_ROTKEY_SHARE = 11, KIND_RELIN_SHARE = 12 };

// the fields of a container header that fuseEvalKeys compares, and the Galois elements of a rotation-key share in
// file order
struct EvkMeta {
    uint32_t kind = 0, ring_dim = 0, limbs = 0, parts = 0, entries = 0;
    std::vector<uint64_t> elements;
};

inline bool is_rot_kind(uint32_t kind) { return kind == 9 || kind == KIND_ROTKEY_SHARE; }

// the kind of the sum of containers of `kind`; 0: not summable
inline uint32_t fused_kind(uint32_t kind) {
    switch (kind) {
    case 4: return 4;
    case KIND_ROTKEY_SHARE: return 9;
    case KIND_RELIN_SHARE: return KIND_RELIN_KEY;
    default: return 0;
    }
}

// empty when a container of `kind` can be an input of fuseEvalKeys, else the refusal
inline std::string fuse_kind_error(const std::string &path, uint32_t kind) {
    if (fused_kind(kind)) return "";
    if (kind == 9 || kind == KIND_RELIN_KEY) return path + " is " + key_kind_name(kind) + ", a finished key, not a share";
    return path + " is " + key_kind_name(kind) + ", not a share of an evaluation key";
}

// the bytes a container with these header fields must have (48-byte header; rotation entries carry their element)
inline uint64_t evk_file_bytes(const EvkMeta &m) {
    const uint64_t key = (uint64_t)m.parts * m.limbs * m.ring_dim * 8;
    return 48 + (is_rot_kind(m.kind) ? (uint64_t)m.entries * (8 + key) : key);
}

// empty when share `b` (file pb) can be added to share `a` (file pa), else the refusal naming the file and the field
inline std::string fuse_mismatch(const std::string &pa, const EvkMeta &a, const std::string &pb, const EvkMeta &b) {
    if (a.kind != b.kind) return pb + ": kind differs from " + pa + " (" + key_kind_name(b.kind) + " beside " + key_kind_name(a.kind) + ")";
    auto field = [&](const char *name, uint32_t x, uint32_t y) {
        return pb + ": " + name + " differs from " + pa + " (" + std::to_string(y) + " beside " + std::to_string(x) + ")";
    };
    if (a.ring_dim != b.ring_dim) return field("ring dimension N", a.ring_dim, b.ring_dim);
    if (a.limbs != b.limbs) return field("limb count D", a.limbs, b.limbs);
    if (a.parts != b.parts) return field("digit count beta", a.parts / 2, b.parts / 2);
    if (!is_rot_kind(a.kind)) return "";
    std::vector<uint64_t> ea = a.elements, eb = b.elements;
    std::sort(ea.begin(), ea.end());
    std::sort(eb.begin(), eb.end());
    for (uint64_t g : ea)
        if (!std::binary_search(eb.begin(), eb.end(), g)) return pb + ": Galois element " + std::to_string(g) + " of " + pa + " is missing";
    for (uint64_t g : eb)
        if (!std::binary_search(ea.begin(), ea.end(), g)) return pb + ": Galois element " + std::to_string(g) + " is not in " + pa;
    return "";
}

// a rotation-key share's own elements: odd, below 2N, none twice; empty when fine
inline std::string elements_error(const std::string &path, const EvkMeta &m) {
    if (m.entries > 64) return path + ": claims " + std::to_string(m.entries) + " entries (at most 64)";
    if (m.elements.size() != m.entries) return path + ": is truncated";
    std::vector<uint64_t> e = m.elements;
    std::sort(e.begin(), e.end());
    for (size_t i = 0; i < e.size(); ++i) {
        if (!(e[i] & 1) || e[i] >= 2ull * m.ring_dim) return path + ": holds the invalid Galois element " + std::to_string(e[i]);
        if (i && e[i] == e[i - 1]) return path + ": holds Galois element " + std::to_string(e[i]) + " twice";
    }
    return "";
}

}  // namespace mkh
