// switchshare.hpp -- shares of the collective key switch of a joint-key aggregate to a recipient's public key
// (switchShare, fuseSwitchShares; include/mkckks.h: mkckks_switch_share_batch).
//
// Key-switch share blob (KIND_SWITCH_SHARE = 8): the BlobHeader of the ciphertext it was made from -- level, noise_deg,
// scale, slots; limbs = nl, the limbs the share was made at -- with kind = 8, parts = 2 and reserved = flags (bit 0, lead:
// component 0 holds c0 + c1 * s + b v + e0, else c1 * s + b v + e0; bit 1, rescale: the share was made with --limbs nl - 1
// and the fusion rescales the sum from nl to nl - 1 limbs), then the payload u64[2][nl][N] in EVALUATION format:
// 48 + 16 nl N bytes.  A share file is the aggregate's envelope (JSON or MKWS) with every ciphertext blob replaced by its
// share blob.  The sum of the parties' blobs of one position is an ordinary ciphertext (kind 1) under the recipient's key.
//
// Shares arrive from the other parties: nothing in a blob is trusted.  decode_switch_share() checks the structure against
// the ring and the limb count of the CryptoContext before it sizes anything; validate_switch_share_header() checks the
// header fields.  Neither needs a device.  The words are range-checked where they are summed, on the device
// (mkckks_count_noncanonical); residues_canonical() is the same check on the host.
#pragma once
#include "hostlib.hpp"

namespace mkh {

struct SwitchShare {
    Ciphertext ct;  // nl, level, noise_deg, slots, scale; data [2][nl][N]; never seeded
    bool lead = false;
    bool rescale = false;  // switchShare --limbs nl - 1: fuseSwitchShares closes with Rescale (nl -> nl - 1 limbs)
};

inline std::string encode_switch_share(const SwitchShare &sh, uint32_t ring_dim) {
    BlobHeader h{};
    std::memcpy(h.magic, "MKCK", 4);
    h.version = 1; h.kind = KIND_SWITCH_SHARE; h.ring_dim = ring_dim; h.limbs = sh.ct.nl; h.parts = 2;
    h.level = sh.ct.level; h.noise_deg = sh.ct.noise_deg; h.scale = sh.ct.scale; h.slots = sh.ct.slots;
    h.reserved = (sh.lead ? 1u : 0u) | (sh.rescale ? 2u : 0u);
    std::string bin(sizeof h + sh.ct.data.size() * 8, '\0');
    std::memcpy(&bin[0], &h, sizeof h);
    if (!sh.ct.data.empty()) std::memcpy(&bin[sizeof h], sh.ct.data.data(), sh.ct.data.size() * 8);
    return raw_blobs() ? bin : Base64Encode(bin);
}

// max_limbs: L of the CryptoContext
inline SwitchShare decode_switch_share(const std::string &b64, uint32_t ring_dim, uint32_t max_limbs) {
    const bool raw = b64.size() >= 4 && !std::memcmp(b64.data(), "MKCK", 4);
    const std::string decoded = raw ? std::string() : Base64Decode(b64);
    const std::string &bin = raw ? b64 : decoded;
    if (bin.size() < sizeof(BlobHeader)) throw std::runtime_error("key-switch share blob too short");
    BlobHeader h;
    std::memcpy(&h, bin.data(), sizeof h);
    if (std::memcmp(h.magic, "MKCK", 4) || h.version != 1 || h.kind != KIND_SWITCH_SHARE)
        throw std::runtime_error("not a mkckks key-switch share blob");
    if (h.ring_dim != ring_dim || h.parts != 2) throw std::runtime_error("key-switch share does not match the CryptoContext");
    if (h.limbs < 1 || h.limbs > max_limbs) throw std::runtime_error("key-switch share: limb count outside [1, L]");
    if (h.reserved > 3) throw std::runtime_error("key-switch share: unknown flag bits");
    const size_t words = (size_t)2 * h.limbs * ring_dim;  // limbs <= L: cannot overflow
    if (bin.size() != sizeof h + words * 8) throw std::runtime_error("key-switch share blob has the wrong size");
    SwitchShare sh;
    sh.ct.nl = h.limbs; sh.ct.level = h.level; sh.ct.noise_deg = h.noise_deg; sh.ct.scale = h.scale; sh.ct.slots = h.slots;
    sh.lead = (h.reserved & 1) != 0;
    sh.rescale = (h.reserved & 2) != 0;
    sh.ct.data.resize(words);
    std::memcpy(sh.ct.data.data(), bin.data() + sizeof h, words * 8);
    return sh;
}

// L: the number of moduli of Q
inline void validate_switch_share_header(const SwitchShare &sh, uint32_t N, uint32_t L) {
    const Ciphertext &c = sh.ct;
    if (c.nl < 1 || c.nl > L) throw std::runtime_error("key-switch share: limb count outside [1, L]");
    if (c.level != L - c.nl) throw std::runtime_error("key-switch share: level does not match its limb count");
    if (c.noise_deg != 1 && c.noise_deg != 2) throw std::runtime_error("key-switch share: noiseScaleDeg must be 1 or 2");
    if (!(c.scale > 0) || !std::isfinite(c.scale)) throw std::runtime_error("key-switch share: bad scaling factor");
    if (c.slots > N / 2) throw std::runtime_error("key-switch share: slot count exceeds N/2");
    if (c.data.size() != (size_t)2 * c.nl * N) throw std::runtime_error("key-switch share: wrong payload size");
    if (sh.rescale && (c.nl < 2 || c.noise_deg != 2))
        throw std::runtime_error("key-switch share: the rescale flag needs noiseScaleDeg 2 and at least 2 limbs");
}

// every word of u64[2][nl][N] below its modulus (moduli: at least nl of them)
inline bool residues_canonical(const SwitchShare &sh, uint32_t N, const std::vector<uint64_t> &moduli) {
    uint64_t bad = 0;
    for (uint32_t comp = 0; comp < 2; ++comp)
        for (uint32_t i = 0; i < sh.ct.nl; ++i) {
            const uint64_t q = moduli[i];
            const uint64_t *p = &sh.ct.data[((size_t)comp * sh.ct.nl + i) * N];
            for (uint32_t k = 0; k < N; ++k) bad |= (uint64_t)(p[k] >= q);
        }
    return bad == 0;
}

inline SwitchShare decode_switch_share_checked(const std::string &blob, uint32_t N, uint32_t L) {
    SwitchShare sh = decode_switch_share(blob, N, L);
    validate_switch_share_header(sh, N, L);
    return sh;
}

// --limbs m: a decimal integer in [1, 64]; the range against the aggregate is the caller's
inline bool parse_limbs(const std::string &v, uint32_t &m) {
    if (v.empty() || v.size() > 2 || v.find_first_not_of("0123456789") != std::string::npos) return false;
    m = (uint32_t)std::atoi(v.c_str());
    return m >= 1 && m <= 64;
}

}  // namespace mkh
