// keyshare.hpp -- Shamir shares of a secret key for t-of-n threshold decryption (shareKey, combineKeyShares,
// partialDecrypt --parties; include/mkckks.h "t-of-n threshold decryption").
//
// Key-share blob (KIND_KEYSHARE = 7): BlobHeader with limbs = L, parts = 1 and level, noise_deg, scale, slots, reserved
// all 0, then the 16-byte trailer {uint32 n_parties, threshold, from_party, to_party}, then the payload u64[L][N] in
// EVALUATION format: 48 + 16 + 8 L N bytes, one blob per file, raw.  from_party = i >= 1: the share f_i(to_party) that
// dealer i made for party to_party; from_party = 0: the combined share sigma_to = sum_i f_i(to_party).
//
// A key-share file is a SECRET and arrives from another party: nothing in it is trusted.  decode_keyshare() checks the
// structure against the ring and the limb count of the CryptoContext before it sizes anything; validate_keyshare()
// checks 1 <= threshold <= n_parties <= MKCKKS_MAX_PARTIES, the party indices, and that every word is below its
// modulus.  Neither needs a device.
#pragma once
#include "hostlib.hpp"

namespace mkh {

enum : uint32_t { KIND_KEYSHARE = 7 };

struct KeyShareTrailer {
    uint32_t n_parties, threshold, from_party, to_party;
};
static_assert(sizeof(KeyShareTrailer) == 16, "key-share trailer layout");

struct KeyShare {
    uint32_t n_parties = 0, threshold = 0, from_party = 0, to_party = 0;
    std::vector<uint64_t> data;  // [L][N]
};

inline size_t keyshare_bytes(uint32_t ring_dim, uint32_t limbs) {
    return sizeof(BlobHeader) + sizeof(KeyShareTrailer) + (size_t)limbs * ring_dim * 8;
}

inline std::string encode_keyshare(const KeyShare &ks, uint32_t ring_dim, uint32_t limbs) {
    BlobHeader h{};
    std::memcpy(h.magic, "MKCK", 4);
    h.version = 1; h.kind = KIND_KEYSHARE; h.ring_dim = ring_dim; h.limbs = limbs; h.parts = 1;
    const KeyShareTrailer t{ks.n_parties, ks.threshold, ks.from_party, ks.to_party};
    std::string bin(sizeof h + sizeof t + ks.data.size() * 8, '\0');
    std::memcpy(&bin[0], &h, sizeof h);
    std::memcpy(&bin[sizeof h], &t, sizeof t);
    if (!ks.data.empty()) std::memcpy(&bin[sizeof h + sizeof t], ks.data.data(), ks.data.size() * 8);
    return bin;
}

// limbs: L of the CryptoContext
inline KeyShare decode_keyshare(const std::string &bin, uint32_t ring_dim, uint32_t limbs) {
    if (bin.size() < sizeof(BlobHeader)) throw std::runtime_error("key-share blob too short");
    BlobHeader h;
    std::memcpy(&h, bin.data(), sizeof h);
    if (std::memcmp(h.magic, "MKCK", 4) || h.version != 1 || h.kind != KIND_KEYSHARE)
        throw std::runtime_error("not a mkckks key-share blob");
    if (h.ring_dim != ring_dim || h.limbs != limbs || h.parts != 1)
        throw std::runtime_error("key share does not match the CryptoContext");
    if (h.level || h.noise_deg || h.scale != 0 || h.slots || h.reserved)
        throw std::runtime_error("key share: unused header fields must be 0");
    if (bin.size() < sizeof h + sizeof(KeyShareTrailer)) throw std::runtime_error("key-share blob: truncated trailer");
    const size_t words = (size_t)limbs * ring_dim;  // the context's own sizes
    if (bin.size() != sizeof h + sizeof(KeyShareTrailer) + words * 8) throw std::runtime_error("key-share blob has the wrong size");
    KeyShareTrailer t;
    std::memcpy(&t, bin.data() + sizeof h, sizeof t);
    KeyShare ks;
    ks.n_parties = t.n_parties; ks.threshold = t.threshold; ks.from_party = t.from_party; ks.to_party = t.to_party;
    ks.data.resize(words);
    std::memcpy(ks.data.data(), bin.data() + sizeof h + sizeof t, words * 8);
    return ks;
}

// moduli: the L moduli of Q
inline void validate_keyshare(const KeyShare &ks, uint32_t N, const std::vector<uint64_t> &moduli) {
    if (ks.n_parties < 1 || ks.n_parties > MKCKKS_MAX_PARTIES) throw std::runtime_error("key share: n_parties outside [1, 64]");
    if (ks.threshold < 1 || ks.threshold > ks.n_parties) throw std::runtime_error("key share: threshold outside [1, n_parties]");
    if (ks.to_party < 1 || ks.to_party > ks.n_parties) throw std::runtime_error("key share: to_party outside [1, n_parties]");
    if (ks.from_party > ks.n_parties) throw std::runtime_error("key share: from_party outside [0, n_parties]");
    if (ks.data.size() != moduli.size() * (size_t)N) throw std::runtime_error("key share: wrong payload size");
    for (size_t i = 0; i < moduli.size(); ++i) {
        const uint64_t q = moduli[i];
        const uint64_t *p = &ks.data[i * N];
        uint64_t bad = 0;
        for (uint32_t k = 0; k < N; ++k) bad |= (uint64_t)(p[k] >= q);
        if (bad) throw std::runtime_error("key share: residue not below its modulus");
    }
}

inline KeyShare decode_keyshare_checked(const std::string &bin, uint32_t N, const std::vector<uint64_t> &moduli) {
    KeyShare ks = decode_keyshare(bin, N, (uint32_t)moduli.size());
    validate_keyshare(ks, N, moduli);
    return ks;
}

// device-free look at a key file: does its header say "key share"?
inline bool looks_like_keyshare(const std::string &path) {
    FilePtr fp(std::fopen(path.c_str(), "rb"));
    if (!fp) return false;
    BlobHeader h{};
    return std::fread(&h, 1, sizeof h, fp.get()) == sizeof h && !std::memcmp(h.magic, "MKCK", 4) && h.kind == KIND_KEYSHARE;
}

// at most one byte more than a key share of this context has: a larger file is refused by its size, not read
inline std::string read_keyshare_file(const std::string &path, uint32_t N, uint32_t limbs) {
    FilePtr fp(std::fopen(path.c_str(), "rb"));
    if (!fp) throw std::runtime_error("Could not open key-share file: " + path);
    std::string bin(keyshare_bytes(N, limbs) + 1, '\0');
    bin.resize(std::fread(&bin[0], 1, bin.size(), fp.get()));
    return bin;
}

inline void write_keyshare_file(const std::string &path, const KeyShare &ks, uint32_t N, uint32_t limbs) {
    const std::string bin = encode_keyshare(ks, N, limbs);
    FilePtr fp(std::fopen(path.c_str(), "wb"));
    if (!fp || std::fwrite(bin.data(), 1, bin.size(), fp.get()) != bin.size())
        throw std::runtime_error("Failed to open output file: " + path);
}

// "i,j,..." -> distinct 1-based party indices within [1, MKCKKS_MAX_PARTIES]; false on anything else
inline bool parse_parties(const std::string &v, std::vector<uint32_t> &out) {
    out.clear();
    size_t pos = 0;
    while (true) {
        const size_t end = v.find(',', pos);
        const std::string tok = v.substr(pos, end == std::string::npos ? std::string::npos : end - pos);
        if (tok.empty() || tok.size() > 2 || tok.find_first_not_of("0123456789") != std::string::npos) return false;
        const uint32_t j = (uint32_t)std::atoi(tok.c_str());
        if (j < 1 || j > MKCKKS_MAX_PARTIES) return false;
        for (uint32_t o : out)
            if (o == j) return false;
        out.push_back(j);
        if (end == std::string::npos) return true;
        pos = end + 1;
    }
}

}  // namespace mkh
