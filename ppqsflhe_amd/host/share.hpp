// share.hpp -- decryption shares of the threshold protocol (keyGen --join, partialDecrypt, fuseDecryptions):
// cc->MultipartyDecryptLead / MultipartyDecryptMain write one per ciphertext, cc->MultipartyDecryptFusion reads n of them.
//
// Share blob (KIND_SHARE): the BlobHeader of the ciphertext it was made from -- limbs = nl, level, noise_deg, scale,
// slots -- with kind = 6, parts = 1 and reserved = the lead flag (1: the share holds c0 + c1 * s, 0: c1 * s alone), then
// the payload u64[nl][N] in COEFFICIENT format: 48 + 8 nl N bytes.  A share file is the ciphertext file's envelope (JSON
// or MKWS) with every ciphertext blob replaced by its share blob.
//
// Shares arrive from the other parties: nothing in a blob is trusted.  decode_share() checks the structure against the
// ring and the limb count of the CryptoContext before it sizes anything; validate_share() checks the header fields and
// that every word is below its modulus (the fusion sums canonical residues lazily).  Neither needs a device.
#pragma once
#include "hostlib.hpp"

namespace mkh {

enum : uint32_t { KIND_SHARE = 6 };

// smudging: partialDecrypt draws the error of ciphertext t from stream t of a fresh OS-drawn key, sigma = 2^bits
constexpr uint32_t SMUDGE_BITS_DEFAULT = HRA_SIGMA_BITS_DEFAULT, SMUDGE_BITS_MIN = 6, SMUDGE_BITS_MAX = 56;
inline bool parse_smudge_bits(const std::string &v, uint32_t &bits) {
    if (v.empty() || v.size() > 2 || v.find_first_not_of("0123456789") != std::string::npos) return false;
    bits = (uint32_t)std::atoi(v.c_str());
    return bits >= SMUDGE_BITS_MIN && bits <= SMUDGE_BITS_MAX;
}

struct Share {
    uint32_t nl = 0, level = 0, noise_deg = 0, slots = 0;
    double scale = 0;
    bool lead = false;
    std::vector<uint64_t> data;  // [nl][N]
};

inline std::string encode_share(const Share &sh, uint32_t ring_dim) {
    BlobHeader h{};
    std::memcpy(h.magic, "MKCK", 4);
    h.version = 1; h.kind = KIND_SHARE; h.ring_dim = ring_dim; h.limbs = sh.nl; h.parts = 1;
    h.level = sh.level; h.noise_deg = sh.noise_deg; h.scale = sh.scale; h.slots = sh.slots;
    h.reserved = sh.lead ? 1 : 0;
    std::string bin(sizeof h + sh.data.size() * 8, '\0');
    std::memcpy(&bin[0], &h, sizeof h);
    if (!sh.data.empty()) std::memcpy(&bin[sizeof h], sh.data.data(), sh.data.size() * 8);
    return raw_blobs() ? bin : Base64Encode(bin);
}

// max_limbs: L of the CryptoContext
inline Share decode_share(const std::string &b64, uint32_t ring_dim, uint32_t max_limbs) {
    const bool raw = b64.size() >= 4 && !std::memcmp(b64.data(), "MKCK", 4);
    const std::string decoded = raw ? std::string() : Base64Decode(b64);
    const std::string &bin = raw ? b64 : decoded;
    if (bin.size() < sizeof(BlobHeader)) throw std::runtime_error("share blob too short");
    BlobHeader h;
    std::memcpy(&h, bin.data(), sizeof h);
    if (std::memcmp(h.magic, "MKCK", 4) || h.version != 1 || h.kind != KIND_SHARE)
        throw std::runtime_error("not a mkckks share blob");
    if (h.ring_dim != ring_dim || h.parts != 1) throw std::runtime_error("share does not match the CryptoContext");
    if (h.limbs < 1 || h.limbs > max_limbs) throw std::runtime_error("share: limb count outside [1, L]");
    if (h.reserved > 1) throw std::runtime_error("share: lead flag must be 0 or 1");
    const size_t words = (size_t)h.limbs * ring_dim;  // limbs <= L: cannot overflow
    if (bin.size() != sizeof h + words * 8) throw std::runtime_error("share blob has the wrong size");
    Share sh;
    sh.nl = h.limbs; sh.level = h.level; sh.noise_deg = h.noise_deg; sh.scale = h.scale; sh.slots = h.slots;
    sh.lead = h.reserved == 1;
    sh.data.resize(words);
    std::memcpy(sh.data.data(), bin.data() + sizeof h, words * 8);
    return sh;
}

// moduli: the L moduli of Q
inline void validate_share(const Share &sh, uint32_t N, const std::vector<uint64_t> &moduli) {
    const uint32_t L = (uint32_t)moduli.size();
    if (sh.nl < 1 || sh.nl > L) throw std::runtime_error("share: limb count outside [1, L]");
    if (sh.level != L - sh.nl) throw std::runtime_error("share: level does not match its limb count");
    if (sh.noise_deg != 1 && sh.noise_deg != 2) throw std::runtime_error("share: noiseScaleDeg must be 1 or 2");
    if (!(sh.scale > 0) || !std::isfinite(sh.scale)) throw std::runtime_error("share: bad scaling factor");
    if (sh.slots > N / 2) throw std::runtime_error("share: slot count exceeds N/2");
    if (sh.data.size() != (size_t)sh.nl * N) throw std::runtime_error("share: wrong payload size");
    for (uint32_t i = 0; i < sh.nl; ++i) {
        const uint64_t q = moduli[i];
        const uint64_t *p = &sh.data[(size_t)i * N];
        uint64_t bad = 0;
        for (uint32_t k = 0; k < N; ++k) bad |= (uint64_t)(p[k] >= q);
        if (bad) throw std::runtime_error("share: residue not below its modulus");
    }
}

inline Share decode_share_checked(const std::string &blob, uint32_t N, const std::vector<uint64_t> &moduli) {
    Share sh = decode_share(blob, N, (uint32_t)moduli.size());
    validate_share(sh, N, moduli);
    return sh;
}

// device-free look at a file that should hold a public key: this project's container for ring dimension N, or a JSON
// document in OpenFHE's nesting (checked in full once the context exists)
inline bool looks_like_public_key(const std::string &path, uint32_t N) {
    FilePtr fp(std::fopen(path.c_str(), "rb"));
    if (!fp) return false;
    BlobHeader h{};
    const size_t got = std::fread(&h, 1, sizeof h, fp.get());
    fp.reset();
    if (got >= 4 && !std::memcmp(h.magic, "MKCK", 4))
        return got == sizeof h && h.version == 1 && h.kind == KIND_PK && h.parts == 2 && h.ring_dim == N;
    try {
        const Json j = Json::parse_file(path);
        return j.contains("value0");
    } catch (const std::exception &) {
        return false;
    }
}

}  // namespace mkh
