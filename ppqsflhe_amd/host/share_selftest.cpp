// share_selftest -- the share-blob parser of share.hpp (decode_share / validate_share) on well-formed and hostile blobs,
// without a device.  Built plain and under AddressSanitizer + UBSan (make share-asan); driven by
// tests/test_threshold_decrypt.py.  Every hostile blob must end in a std::runtime_error -- no crash, no sanitizer report,
// no allocation sized by an unchecked header field.  Exit 0 when every case behaves, 1 otherwise.
#include "share.hpp"
using namespace mkh;

namespace {

constexpr uint32_t N = 64;
const std::vector<uint64_t> MODULI = {1152921504606846577ull, 1099511627689ull, 1099511627473ull};  // sizes of a 60/40/40-bit chain

int failures = 0;

void expect_ok(const char *name, const std::string &blob, const Share &want) {
    try {
        const Share got = decode_share_checked(blob, N, MODULI);
        const bool same = got.nl == want.nl && got.level == want.level && got.noise_deg == want.noise_deg &&
                          got.slots == want.slots && got.scale == want.scale && got.lead == want.lead && got.data == want.data;
        if (!same) {
            ++failures;
            std::cerr << "FAIL " << name << ": round trip differs" << std::endl;
            return;
        }
        std::cout << "ok " << name << std::endl;
    } catch (const std::exception &e) {
        ++failures;
        std::cerr << "FAIL " << name << ": " << e.what() << std::endl;
    }
}

void expect_refused(const char *name, const std::string &blob, const char *why) {
    try {
        decode_share_checked(blob, N, MODULI);
        ++failures;
        std::cerr << "FAIL " << name << ": accepted" << std::endl;
    } catch (const std::runtime_error &e) {
        if (std::string(e.what()).find(why) == std::string::npos) {
            ++failures;
            std::cerr << "FAIL " << name << ": refused with \"" << e.what() << "\", expected \"" << why << "\"" << std::endl;
            return;
        }
        std::cout << "ok " << name << ": " << e.what() << std::endl;
    }
}

Share good_share(uint32_t nl, bool lead) {
    Share sh;
    sh.nl = nl; sh.level = (uint32_t)MODULI.size() - nl; sh.noise_deg = 2; sh.slots = N / 2; sh.scale = 1099511627776.0;
    sh.lead = lead;
    sh.data.resize((size_t)nl * N);
    for (uint32_t i = 0; i < nl; ++i)
        for (uint32_t k = 0; k < N; ++k) sh.data[(size_t)i * N + k] = (MODULI[i] - 1 - k * 977u) % MODULI[i];
    sh.data[0] = MODULI[0] - 1;  // the largest canonical word
    sh.data[1] = 0;
    return sh;
}

std::string with_header(std::string bin, void (*edit)(BlobHeader &)) {
    BlobHeader h;
    std::memcpy(&h, bin.data(), sizeof h);
    edit(h);
    std::memcpy(&bin[0], &h, sizeof h);
    return bin;
}

}  // namespace

int main() {
    raw_blobs() = true;
    for (uint32_t nl = 1; nl <= MODULI.size(); ++nl)
        for (int lead = 0; lead < 2; ++lead) {
            const Share sh = good_share(nl, lead != 0);
            expect_ok("raw round trip", encode_share(sh, N), sh);
            raw_blobs() = false;
            expect_ok("base64 round trip", encode_share(sh, N), sh);
            raw_blobs() = true;
        }
    const Share sh = good_share(2, true);
    const std::string bin = encode_share(sh, N);

    // truncated: inside the header, at the header's end, inside the payload, one byte short
    for (size_t len : {(size_t)0, (size_t)3, (size_t)4, (size_t)20, sizeof(BlobHeader) - 1})
        expect_refused("truncated header", bin.substr(0, len), len < 4 ? "" : "share blob too short");
    for (size_t len : {sizeof(BlobHeader), sizeof(BlobHeader) + 8, bin.size() / 2, bin.size() - 1})
        expect_refused("truncated payload", bin.substr(0, len), "share blob has the wrong size");
    // oversized: trailing bytes, a whole extra limb
    expect_refused("oversized by one byte", bin + std::string(1, '\0'), "share blob has the wrong size");
    expect_refused("oversized by a limb", bin + std::string((size_t)8 * N, '\0'), "share blob has the wrong size");
    // limb counts that must not size an allocation
    expect_refused("zero limbs", with_header(bin, [](BlobHeader &h) { h.limbs = 0; }), "limb count outside [1, L]");
    expect_refused("too many limbs", with_header(bin, [](BlobHeader &h) { h.limbs = 4; }), "limb count outside [1, L]");
    expect_refused("2^32 - 1 limbs", with_header(bin, [](BlobHeader &h) { h.limbs = 0xFFFFFFFFu; }), "limb count outside [1, L]");
    // wrong kind: a ciphertext, a seeded ciphertext, a key, an unknown kind
    {
        Ciphertext ct;
        ct.nl = 2; ct.level = 1; ct.noise_deg = 2; ct.slots = N / 2; ct.scale = sh.scale;
        ct.data.assign((size_t)2 * 2 * N, 1);
        expect_refused("ciphertext blob", encode_ct(ct, N), "not a mkckks share blob");
    }
    for (uint32_t kind : {(uint32_t)KIND_CT_SEEDED, (uint32_t)KIND_PK, (uint32_t)KIND_SK, (uint32_t)KIND_RK, 7u, 0u}) {
        std::string b = bin;
        std::memcpy(&b[8], &kind, 4);
        expect_refused("wrong kind", b, "not a mkckks share blob");
    }
    expect_refused("wrong magic", "MKCX" + bin.substr(4), "");
    expect_refused("wrong version", with_header(bin, [](BlobHeader &h) { h.version = 2; }), "not a mkckks share blob");
    // wrong ring, wrong parts
    expect_refused("wrong ring", with_header(bin, [](BlobHeader &h) { h.ring_dim = 2 * N; }), "does not match the CryptoContext");
    expect_refused("ring 0", with_header(bin, [](BlobHeader &h) { h.ring_dim = 0; }), "does not match the CryptoContext");
    expect_refused("two parts", with_header(bin, [](BlobHeader &h) { h.parts = 2; }), "does not match the CryptoContext");
    // header fields
    expect_refused("lead flag 2", with_header(bin, [](BlobHeader &h) { h.reserved = 2; }), "lead flag must be 0 or 1");
    expect_refused("level", with_header(bin, [](BlobHeader &h) { h.level = 0; }), "level does not match its limb count");
    expect_refused("noise degree", with_header(bin, [](BlobHeader &h) { h.noise_deg = 3; }), "noiseScaleDeg must be 1 or 2");
    expect_refused("scale 0", with_header(bin, [](BlobHeader &h) { h.scale = 0; }), "bad scaling factor");
    expect_refused("scale nan", with_header(bin, [](BlobHeader &h) { h.scale = std::nan(""); }), "bad scaling factor");
    expect_refused("scale inf", with_header(bin, [](BlobHeader &h) { h.scale = INFINITY; }), "bad scaling factor");
    expect_refused("slots", with_header(bin, [](BlobHeader &h) { h.slots = N; }), "slot count exceeds N/2");
    // non-canonical words: q, q + 1 and 2^64 - 1, first and last word of each limb
    for (uint32_t i = 0; i < 2; ++i)
        for (size_t k : {(size_t)0, (size_t)N - 1})
            for (uint64_t v : {MODULI[i], MODULI[i] + 1, ~(uint64_t)0}) {
                std::string b = bin;
                std::memcpy(&b[sizeof(BlobHeader) + ((size_t)i * N + k) * 8], &v, 8);
                expect_refused("non-canonical word", b, "residue not below its modulus");
            }
    // base64 forms: garbage, and a valid encoding of a truncated blob
    expect_refused("bad base64", "!!!not base64!!!", "");
    expect_refused("base64 of a short blob", Base64Encode(bin.substr(0, 30)), "share blob too short");
    expect_refused("empty", "", "");

    if (failures) {
        std::cerr << failures << " case(s) failed" << std::endl;
        return 1;
    }
    std::cout << "ok share selftest" << std::endl;
    return 0;
}
