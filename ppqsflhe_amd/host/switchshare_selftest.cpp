// switchshare_selftest -- the key-switch share parser of switchshare.hpp (decode_switch_share, validate_switch_share_header,
// residues_canonical, parse_limbs) on well-formed and hostile blobs, without a device.  Built plain and under
// AddressSanitizer + UBSan (make switchshare-asan); driven by tests/test_key_switch_shares.py.  Every hostile blob must end
// in a std::runtime_error -- no crash, no sanitizer report, no allocation sized by an unchecked header field.  Exit 0 when
// every case behaves, 1 otherwise.
#include "share.hpp"
#include "switchshare.hpp"
using namespace mkh;

namespace {

constexpr uint32_t N = 64;
const std::vector<uint64_t> MODULI = {1152921504606846577ull, 1099511627689ull, 1099511627473ull};  // sizes of a 60/40/40-bit chain
const uint32_t L = (uint32_t)MODULI.size();

int failures = 0;

void expect_ok(const char *name, const std::string &blob, const SwitchShare &want) {
    try {
        const SwitchShare got = decode_switch_share_checked(blob, N, L);
        const bool same = got.ct.nl == want.ct.nl && got.ct.level == want.ct.level && got.ct.noise_deg == want.ct.noise_deg &&
                          got.ct.slots == want.ct.slots && got.ct.scale == want.ct.scale && got.lead == want.lead && got.rescale == want.rescale &&
                          got.ct.data == want.ct.data && !got.ct.seeded && residues_canonical(got, N, MODULI);
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
        decode_switch_share_checked(blob, N, L);
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

void expect(const char *name, bool ok) {
    if (!ok) {
        ++failures;
        std::cerr << "FAIL " << name << std::endl;
        return;
    }
    std::cout << "ok " << name << std::endl;
}

SwitchShare good_share(uint32_t nl, bool lead, bool rescale = false) {
    SwitchShare sh;
    sh.ct.nl = nl; sh.ct.level = L - nl; sh.ct.noise_deg = 2; sh.ct.slots = N / 2; sh.ct.scale = 1099511627776.0;
    sh.lead = lead;
    sh.rescale = rescale;
    sh.ct.data.resize((size_t)2 * nl * N);
    for (uint32_t comp = 0; comp < 2; ++comp)
        for (uint32_t i = 0; i < nl; ++i)
            for (uint32_t k = 0; k < N; ++k)
                sh.ct.data[((size_t)comp * nl + i) * N + k] = (MODULI[i] - 1 - (k + 31 * comp) * 977u) % MODULI[i];
    sh.ct.data[0] = MODULI[0] - 1;  // the largest canonical word
    sh.ct.data[1] = 0;
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
    for (uint32_t nl = 1; nl <= L; ++nl)
        for (int lead = 0; lead < 2; ++lead) {
            const SwitchShare sh = good_share(nl, lead != 0);
            expect_ok("raw round trip", encode_switch_share(sh, N), sh);
            raw_blobs() = false;
            expect_ok("base64 round trip", encode_switch_share(sh, N), sh);
            raw_blobs() = true;
            if (nl >= 2) expect_ok("rescale flag round trip", encode_switch_share(good_share(nl, lead != 0, true), N), good_share(nl, lead != 0, true));
        }
    const SwitchShare sh = good_share(2, true);
    const std::string bin = encode_switch_share(sh, N);

    // truncated: inside the header, at the header's end, inside the payload, one byte short
    for (size_t len : {(size_t)0, (size_t)3, (size_t)4, (size_t)20, sizeof(BlobHeader) - 1})
        expect_refused("truncated header", bin.substr(0, len), len < 4 ? "" : "key-switch share blob too short");
    for (size_t len : {sizeof(BlobHeader), sizeof(BlobHeader) + 8, bin.size() / 2, bin.size() - 1})
        expect_refused("truncated payload", bin.substr(0, len), "key-switch share blob has the wrong size");
    // oversized: trailing bytes, a whole extra limb
    expect_refused("oversized by one byte", bin + std::string(1, '\0'), "key-switch share blob has the wrong size");
    expect_refused("oversized by a limb", bin + std::string((size_t)8 * N, '\0'), "key-switch share blob has the wrong size");
    // limb counts that must not size an allocation
    expect_refused("zero limbs", with_header(bin, [](BlobHeader &h) { h.limbs = 0; }), "limb count outside [1, L]");
    expect_refused("too many limbs", with_header(bin, [](BlobHeader &h) { h.limbs = 4; }), "limb count outside [1, L]");
    expect_refused("2^32 - 1 limbs", with_header(bin, [](BlobHeader &h) { h.limbs = 0xFFFFFFFFu; }), "limb count outside [1, L]");
    expect_refused("2^31 limbs", with_header(bin, [](BlobHeader &h) { h.limbs = 0x80000000u; }), "limb count outside [1, L]");
    // wrong kind: a ciphertext, a decryption share, a seeded ciphertext, a key, a key share, an unknown kind
    {
        Ciphertext ct;
        ct.nl = 2; ct.level = 1; ct.noise_deg = 2; ct.slots = N / 2; ct.scale = sh.ct.scale;
        ct.data.assign((size_t)2 * 2 * N, 1);
        expect_refused("ciphertext blob", encode_ct(ct, N), "not a mkckks key-switch share blob");
        Share ds;
        ds.nl = 2; ds.level = 1; ds.noise_deg = 2; ds.slots = N / 2; ds.scale = sh.ct.scale;
        ds.data.assign((size_t)2 * N, 1);
        expect_refused("decryption share blob", encode_share(ds, N), "not a mkckks key-switch share blob");
        // and the other way round: a key-switch share is neither a ciphertext nor a decryption share
        try {
            decode_ct(bin, N);
            expect("key-switch share refused as a ciphertext", false);
        } catch (const std::runtime_error &) {
            expect("key-switch share refused as a ciphertext", true);
        }
        try {
            decode_share(bin, N, L);
            expect("key-switch share refused as a decryption share", false);
        } catch (const std::runtime_error &) {
            expect("key-switch share refused as a decryption share", true);
        }
    }
    for (uint32_t kind : {(uint32_t)KIND_CT_SEEDED, (uint32_t)KIND_PK, (uint32_t)KIND_SK, (uint32_t)KIND_RK, 7u, 9u, 0u}) {
        std::string b = bin;
        std::memcpy(&b[8], &kind, 4);
        expect_refused("wrong kind", b, "not a mkckks key-switch share blob");
    }
    expect_refused("wrong magic", "MKCX" + bin.substr(4), "");
    expect_refused("wrong version", with_header(bin, [](BlobHeader &h) { h.version = 2; }), "not a mkckks key-switch share blob");
    // wrong ring, wrong parts
    expect_refused("wrong ring", with_header(bin, [](BlobHeader &h) { h.ring_dim = 2 * N; }), "does not match the CryptoContext");
    expect_refused("ring 0", with_header(bin, [](BlobHeader &h) { h.ring_dim = 0; }), "does not match the CryptoContext");
    expect_refused("one part", with_header(bin, [](BlobHeader &h) { h.parts = 1; }), "does not match the CryptoContext");
    expect_refused("three parts", with_header(bin, [](BlobHeader &h) { h.parts = 3; }), "does not match the CryptoContext");
    // header fields
    expect_refused("flag bits 4", with_header(bin, [](BlobHeader &h) { h.reserved = 4; }), "unknown flag bits");
    expect_refused("flag bits 2^31", with_header(bin, [](BlobHeader &h) { h.reserved = 0x80000000u; }), "unknown flag bits");
    expect_refused("rescale at degree 1", with_header(bin, [](BlobHeader &h) { h.reserved = 3; h.noise_deg = 1; }), "the rescale flag needs");
    expect_refused("rescale of one limb", with_header(encode_switch_share(good_share(1, true), N), [](BlobHeader &h) { h.reserved = 2; }),
                   "the rescale flag needs");
    expect_refused("level", with_header(bin, [](BlobHeader &h) { h.level = 0; }), "level does not match its limb count");
    expect_refused("noise degree", with_header(bin, [](BlobHeader &h) { h.noise_deg = 3; }), "noiseScaleDeg must be 1 or 2");
    expect_refused("scale 0", with_header(bin, [](BlobHeader &h) { h.scale = 0; }), "bad scaling factor");
    expect_refused("scale nan", with_header(bin, [](BlobHeader &h) { h.scale = std::nan(""); }), "bad scaling factor");
    expect_refused("scale inf", with_header(bin, [](BlobHeader &h) { h.scale = INFINITY; }), "bad scaling factor");
    expect_refused("slots", with_header(bin, [](BlobHeader &h) { h.slots = N; }), "slot count exceeds N/2");
    // non-canonical words: q, q + 1 and 2^64 - 1, first and last word of each limb of both components
    {
        bool all = true;
        for (uint32_t comp = 0; comp < 2; ++comp)
            for (uint32_t i = 0; i < 2; ++i)
                for (size_t k : {(size_t)0, (size_t)N - 1})
                    for (uint64_t v : {MODULI[i], MODULI[i] + 1, ~(uint64_t)0}) {
                        SwitchShare b = sh;
                        b.ct.data[((size_t)comp * 2 + i) * N + k] = v;
                        all = all && !residues_canonical(b, N, MODULI);
                    }
        expect("non-canonical word", all && residues_canonical(sh, N, MODULI));
    }
    // base64 forms: garbage, and a valid encoding of a truncated blob
    expect_refused("bad base64", "!!!not base64!!!", "");
    expect_refused("base64 of a short blob", Base64Encode(bin.substr(0, 30)), "key-switch share blob too short");
    expect_refused("empty", "", "");
    // --limbs
    {
        uint32_t m = 99;
        bool ok = parse_limbs("1", m) && m == 1 && parse_limbs("12", m) && m == 12 && parse_limbs("64", m) && m == 64;
        for (const char *bad : {"", "0", "00", "65", "100", "-1", "+1", "1x", " 1", "1.0"}) ok = ok && !parse_limbs(bad, m);
        expect("parse_limbs", ok);
    }

    if (failures) {
        std::cerr << failures << " case(s) failed" << std::endl;
        return 1;
    }
    std::cout << "ok switchshare selftest" << std::endl;
    return 0;
}
