// keyshare_selftest -- the key-share parser of keyshare.hpp (decode_keyshare / validate_keyshare) on well-formed and hostile
// blobs, and mkckks_lagrange_at_zero on a host-only context against unsigned __int128 arithmetic; no device.  Built
// plain and under AddressSanitizer + UBSan (make keyshare-asan); driven by tests/test_key_sharing.py.  Every hostile blob
// must end in a std::runtime_error -- no crash, no sanitizer report, no allocation sized by an unchecked field.  Exit 0
// when every case behaves, 1 otherwise.
#include "keyshare.hpp"
using namespace mkh;

namespace {

constexpr uint32_t N = 64;
const std::vector<uint64_t> MODULI = {1152921504606846577ull, 1099511627689ull, 1099511627473ull};  // sizes of a 60/40/40-bit chain
const uint32_t L = (uint32_t)MODULI.size();
constexpr size_t HEAD = sizeof(BlobHeader), TRAIL = sizeof(KeyShareTrailer);

int failures = 0;

void fail(const char *name, const std::string &why) {
    ++failures;
    std::cerr << "FAIL " << name << ": " << why << std::endl;
}

void expect_ok(const char *name, const std::string &blob, const KeyShare &want) {
    try {
        const KeyShare got = decode_keyshare_checked(blob, N, MODULI);
        if (got.n_parties != want.n_parties || got.threshold != want.threshold || got.from_party != want.from_party ||
            got.to_party != want.to_party || got.data != want.data)
            return fail(name, "round trip differs");
        std::cout << "ok " << name << std::endl;
    } catch (const std::exception &e) {
        fail(name, e.what());
    }
}

void expect_refused(const char *name, const std::string &blob, const char *why) {
    try {
        decode_keyshare_checked(blob, N, MODULI);
        fail(name, "accepted");
    } catch (const std::runtime_error &e) {
        if (std::string(e.what()).find(why) == std::string::npos)
            return fail(name, std::string("refused with \"") + e.what() + "\", expected \"" + why + "\"");
        std::cout << "ok " << name << ": " << e.what() << std::endl;
    }
}

KeyShare good(uint32_t n, uint32_t t, uint32_t from, uint32_t to) {
    KeyShare ks;
    ks.n_parties = n; ks.threshold = t; ks.from_party = from; ks.to_party = to;
    ks.data.resize((size_t)L * N);
    for (uint32_t i = 0; i < L; ++i)
        for (uint32_t k = 0; k < N; ++k) ks.data[(size_t)i * N + k] = (MODULI[i] - 1 - k * 977u) % MODULI[i];
    ks.data[0] = MODULI[0] - 1;  // the largest canonical word
    ks.data[1] = 0;
    return ks;
}

std::string with_header(std::string bin, void (*edit)(BlobHeader &)) {
    BlobHeader h;
    std::memcpy(&h, bin.data(), sizeof h);
    edit(h);
    std::memcpy(&bin[0], &h, sizeof h);
    return bin;
}
std::string with_trailer(std::string bin, void (*edit)(KeyShareTrailer &)) {
    KeyShareTrailer t;
    std::memcpy(&t, bin.data() + HEAD, sizeof t);
    edit(t);
    std::memcpy(&bin[HEAD], &t, sizeof t);
    return bin;
}

typedef unsigned __int128 u128;
uint64_t powmod(uint64_t a, uint64_t e, uint64_t q) {
    uint64_t r = 1;
    for (a %= q; e; e >>= 1, a = (uint64_t)((u128)a * a % q))
        if (e & 1) r = (uint64_t)((u128)r * a % q);
    return r;
}

// lambda of set[a] at 0 mod the prime q, in 128-bit arithmetic (inverse by Fermat)
uint64_t lagrange_ref(const std::vector<uint32_t> &set, size_t a, uint64_t q) {
    u128 num = 1, den = 1;
    for (size_t b = 0; b < set.size(); ++b) {
        if (b == a) continue;
        num = num * set[b] % q;
        den = den * ((u128)q + set[b] - set[a]) % q;
    }
    return (uint64_t)(num * powmod((uint64_t)den, q - 2, q) % q);
}

void lagrange_cases() {
    mkckks_params p{};
    p.log_n = 12; p.mult_depth = 2; p.scaling_bits = 40; p.first_bits = 60; p.dnum = 2; p.aux_bits = 60; p.extra_bits = 20;
    p.device = -1;
    mkckks_ctx *ctx = nullptr;
    if (mkckks_ctx_create(&p, &ctx) != MKCKKS_OK) return fail("lagrange context", mkckks_last_error());
    mkckks_info info{};
    mkckks_ctx_info(ctx, &info);
    std::vector<uint64_t> moduli(info.num_q + info.num_p);
    mkckks_ctx_moduli(ctx, moduli.data());
    const std::vector<std::vector<uint32_t>> sets = {{1}, {1, 2}, {2, 5, 64}};
    const char *names[] = {"lagrange {1}", "lagrange {1,2}", "lagrange {2,5,64}"};
    for (size_t s = 0; s < sets.size(); ++s) {
        const std::vector<uint32_t> &set = sets[s];
        std::vector<uint64_t> out(set.size() * info.num_q, ~(uint64_t)0);
        if (mkckks_lagrange_at_zero(ctx, set.data(), (uint32_t)set.size(), out.data()) != MKCKKS_OK) {
            fail(names[s], mkckks_last_error());
            continue;
        }
        bool same = true;
        for (size_t a = 0; a < set.size(); ++a)
            for (uint32_t l = 0; l < info.num_q; ++l) same = same && out[a * info.num_q + l] == lagrange_ref(set, a, moduli[l]);
        if (same) std::cout << "ok " << names[s] << std::endl;
        else fail(names[s], "differs from 128-bit arithmetic");
    }
    std::vector<uint64_t> out(4 * info.num_q);
    const uint32_t dup[] = {3, 7, 3}, zero[] = {0, 1}, big[] = {1, 65};
    const bool refused = mkckks_lagrange_at_zero(ctx, dup, 3, out.data()) == MKCKKS_E_INVALID &&
                         mkckks_lagrange_at_zero(ctx, zero, 2, out.data()) == MKCKKS_E_INVALID &&
                         mkckks_lagrange_at_zero(ctx, big, 2, out.data()) == MKCKKS_E_INVALID &&
                         mkckks_lagrange_at_zero(ctx, dup, 0, out.data()) == MKCKKS_E_INVALID;
    if (refused) std::cout << "ok lagrange duplicates refused" << std::endl;
    else fail("lagrange duplicates refused", "a bad party set was accepted");
    mkckks_ctx_destroy(ctx);
}

}  // namespace

int main() {
    for (uint32_t from : {0u, 1u, 3u}) {
        const KeyShare ks = good(3, 2, from, 2);
        expect_ok("round trip", encode_keyshare(ks, N, L), ks);
    }
    {
        const KeyShare ks = good(64, 64, 64, 64);
        expect_ok("round trip at 64 parties", encode_keyshare(ks, N, L), ks);
    }
    const KeyShare ks = good(3, 2, 1, 3);
    const std::string bin = encode_keyshare(ks, N, L);

    for (size_t len : {(size_t)0, (size_t)3, (size_t)20, HEAD - 1}) expect_refused("truncated header", bin.substr(0, len), "key-share blob too short");
    for (size_t len : {HEAD, HEAD + 1, HEAD + TRAIL - 1}) expect_refused("truncated trailer", bin.substr(0, len), "truncated trailer");
    for (size_t len : {HEAD + TRAIL, HEAD + TRAIL + 8, bin.size() / 2, bin.size() - 1})
        expect_refused("truncated payload", bin.substr(0, len), "key-share blob has the wrong size");
    expect_refused("oversized by one byte", bin + std::string(1, '\0'), "key-share blob has the wrong size");
    expect_refused("oversized by a limb", bin + std::string((size_t)8 * N, '\0'), "key-share blob has the wrong size");
    // wrong kinds: a decryption share (kind 6) with its own layout, and the other kinds on this blob
    {
        BlobHeader h{};
        std::memcpy(h.magic, "MKCK", 4);
        h.version = 1; h.kind = 6; h.ring_dim = N; h.limbs = L; h.parts = 1; h.noise_deg = 2; h.scale = 1099511627776.0; h.slots = N / 2;
        std::string b(HEAD + (size_t)L * N * 8, '\1');
        std::memcpy(&b[0], &h, sizeof h);
        expect_refused("share blob of kind 6", b, "not a mkckks key-share blob");
    }
    for (uint32_t kind : {(uint32_t)KIND_CT, (uint32_t)KIND_SK, 6u, 8u, 0u}) {
        std::string b = bin;
        std::memcpy(&b[8], &kind, 4);
        expect_refused("wrong kind", b, "not a mkckks key-share blob");
    }
    expect_refused("wrong magic", "MKCX" + bin.substr(4), "not a mkckks key-share blob");
    expect_refused("wrong version", with_header(bin, [](BlobHeader &h) { h.version = 2; }), "not a mkckks key-share blob");
    expect_refused("wrong ring", with_header(bin, [](BlobHeader &h) { h.ring_dim = 2 * N; }), "does not match the CryptoContext");
    expect_refused("ring 0", with_header(bin, [](BlobHeader &h) { h.ring_dim = 0; }), "does not match the CryptoContext");
    expect_refused("fewer limbs", with_header(bin, [](BlobHeader &h) { h.limbs = 2; }), "does not match the CryptoContext");
    expect_refused("2^32 - 1 limbs", with_header(bin, [](BlobHeader &h) { h.limbs = 0xFFFFFFFFu; }), "does not match the CryptoContext");
    expect_refused("two parts", with_header(bin, [](BlobHeader &h) { h.parts = 2; }), "does not match the CryptoContext");
    expect_refused("level set", with_header(bin, [](BlobHeader &h) { h.level = 1; }), "unused header fields must be 0");
    expect_refused("scale nan", with_header(bin, [](BlobHeader &h) { h.scale = std::nan(""); }), "unused header fields must be 0");
    expect_refused("reserved set", with_header(bin, [](BlobHeader &h) { h.reserved = 1; }), "unused header fields must be 0");
    // the trailer
    expect_refused("n_parties 0", with_trailer(bin, [](KeyShareTrailer &t) { t.n_parties = 0; }), "n_parties outside [1, 64]");
    expect_refused("n_parties 65", with_trailer(bin, [](KeyShareTrailer &t) { t.n_parties = 65; }), "n_parties outside [1, 64]");
    expect_refused("threshold 0", with_trailer(bin, [](KeyShareTrailer &t) { t.threshold = 0; }), "threshold outside [1, n_parties]");
    expect_refused("threshold > n_parties", with_trailer(bin, [](KeyShareTrailer &t) { t.threshold = 4; }),
                   "threshold outside [1, n_parties]");
    expect_refused("to_party 0", with_trailer(bin, [](KeyShareTrailer &t) { t.to_party = 0; }), "to_party outside [1, n_parties]");
    expect_refused("to_party > n_parties", with_trailer(bin, [](KeyShareTrailer &t) { t.to_party = 4; }),
                   "to_party outside [1, n_parties]");
    expect_refused("from_party > n_parties", with_trailer(bin, [](KeyShareTrailer &t) { t.from_party = 0xFFFFFFFFu; }),
                   "from_party outside [0, n_parties]");
    // non-canonical words: q, q + 1 and 2^64 - 1, first and last word of each limb
    for (uint32_t i = 0; i < L; ++i)
        for (size_t k : {(size_t)0, (size_t)N - 1})
            for (uint64_t v : {MODULI[i], MODULI[i] + 1, ~(uint64_t)0}) {
                std::string b = bin;
                std::memcpy(&b[HEAD + TRAIL + ((size_t)i * N + k) * 8], &v, 8);
                expect_refused("non-canonical word", b, "residue not below its modulus");
            }
    expect_refused("empty", "", "key-share blob too short");
    // --parties lists
    {
        std::vector<uint32_t> v;
        const bool ok = parse_parties("1,3", v) && v == std::vector<uint32_t>{1, 3} && parse_parties("64", v) && !parse_parties("", v) &&
                        !parse_parties("1,,2", v) && !parse_parties("1,2,", v) && !parse_parties("0,1", v) && !parse_parties("65", v) &&
                        !parse_parties("2,2", v) && !parse_parties("1;2", v) && !parse_parties("-1", v) && !parse_parties("100", v);
        if (ok) std::cout << "ok parties list" << std::endl;
        else fail("parties list", "parse_parties misjudged a list");
    }
    lagrange_cases();

    if (failures) {
        std::cerr << failures << " case(s) failed" << std::endl;
        return 1;
    }
    std::cout << "ok keyshare selftest" << std::endl;
    return 0;
}
