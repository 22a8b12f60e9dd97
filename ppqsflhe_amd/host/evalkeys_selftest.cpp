// evalkeys_selftest -- the kinds and the matching rules of the collective evaluation keys (evalkeys.hpp) as a
// stand-alone program without the library; built plain and under -fsanitize=address,undefined (Makefile), run by
// tests/test_collective_keys_surface.py.
#include <cstdio>

#include "evalkeys.hpp"
using namespace mkh;

static int failures = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                           \
        }                                                         \
    } while (0)

static EvkMeta meta(uint32_t kind, std::vector<uint64_t> el = {}) {
    EvkMeta m;
    m.kind = kind; m.ring_dim = 1024; m.limbs = 8; m.parts = 4; m.entries = (uint32_t)el.size();
    m.elements = std::move(el);
    return m;
}

int main() {
    // what sums to what
    CHECK(fused_kind(4) == 4 && fused_kind(KIND_ROTKEY_SHARE) == 9 && fused_kind(KIND_RELIN_SHARE) == KIND_RELIN_KEY);
    for (uint32_t k : {0u, 1u, 2u, 3u, 5u, 6u, 7u, 8u, 9u, 10u, 13u, 0xFFFFFFFFu}) CHECK(fused_kind(k) == 0);
    CHECK(KIND_ROTKEY_SHARE == 11 && KIND_RELIN_SHARE == 12 && KIND_RELIN_KEY == 10);
    // names: a share offered as a key is refused by name
    CHECK(key_kind_name(11) == "a rotation-key share" && key_kind_name(12) == "a relinearisation-key share");
    CHECK(relin_kind_error("s", 12) == "s is a relinearisation-key share, not a relinearisation key (relinKeyGen writes one)");
    CHECK(relin_kind_error("s", 11).find("a rotation-key share") != std::string::npos);
    CHECK(key_kind_name(4) == "a re-encryption key" && key_kind_name(9) == "a rotation-key file");
    // inputs of fuseEvalKeys
    CHECK(fuse_kind_error("f", 4).empty() && fuse_kind_error("f", 11).empty() && fuse_kind_error("f", 12).empty());
    CHECK(fuse_kind_error("f", 9) == "f is a rotation-key file, a finished key, not a share");
    CHECK(fuse_kind_error("f", 10) == "f is a relinearisation key, a finished key, not a share");
    CHECK(fuse_kind_error("f", 2) == "f is a public key, not a share of an evaluation key");
    CHECK(fuse_kind_error("f", 3).find("a secret key") != std::string::npos);
    CHECK(fuse_kind_error("f", 77).find("a container of kind 77") != std::string::npos);
    // sizes
    CHECK(evk_file_bytes(meta(4)) == 48 + 4ull * 8 * 1024 * 8 && evk_file_bytes(meta(12)) == evk_file_bytes(meta(4)));
    CHECK(evk_file_bytes(meta(11, {5, 25, 625})) == 48 + 3 * (8 + 4ull * 8 * 1024 * 8));
    CHECK(evk_file_bytes(meta(11)) == 48);
    EvkMeta big = meta(11, {5});
    big.ring_dim = 1u << 17; big.limbs = 64; big.parts = 128; big.entries = 64;  // no 32-bit overflow
    CHECK(evk_file_bytes(big) == 48 + 64ull * (8 + 128ull * 64 * (1u << 17) * 8));
    // matching, field by field, in the order kind, N, D, beta, elements
    const EvkMeta a = meta(12);
    EvkMeta b = a;
    CHECK(fuse_mismatch("a", a, "b", b).empty());
    b.kind = 4;
    CHECK(fuse_mismatch("a", a, "b", b) == "b: kind differs from a (a re-encryption key beside a relinearisation-key share)");
    b.ring_dim = 2048;
    CHECK(fuse_mismatch("a", a, "b", b).find("kind differs") != std::string::npos);
    b = a; b.ring_dim = 2048;
    CHECK(fuse_mismatch("a", a, "b", b) == "b: ring dimension N differs from a (2048 beside 1024)");
    b = a; b.limbs = 9;
    CHECK(fuse_mismatch("a", a, "b", b) == "b: limb count D differs from a (9 beside 8)");
    b = a; b.parts = 6;
    CHECK(fuse_mismatch("a", a, "b", b) == "b: digit count beta differs from a (3 beside 2)");
    b = a; b.entries = 7;  // entries and elements play no role outside rotation shares
    CHECK(fuse_mismatch("a", a, "b", b).empty());
    // sets of Galois elements: order does not matter, membership does
    const EvkMeta r = meta(11, {5, 25, 625});
    CHECK(fuse_mismatch("a", r, "b", meta(11, {625, 5, 25})).empty());
    CHECK(fuse_mismatch("a", r, "b", meta(11, {5, 25})) == "b: Galois element 625 of a is missing");
    CHECK(fuse_mismatch("a", r, "b", meta(11, {5, 25, 625, 3})) == "b: Galois element 3 is not in a");
    CHECK(fuse_mismatch("a", r, "b", meta(11, {5, 25, 627})) == "b: Galois element 625 of a is missing");
    CHECK(fuse_mismatch("a", meta(11), "b", meta(11)).empty());
    CHECK(fuse_mismatch("a", meta(11), "b", meta(11, {5})) == "b: Galois element 5 is not in a");
    // a share's own elements
    CHECK(elements_error("f", r).empty() && elements_error("f", meta(11)).empty());
    CHECK(elements_error("f", meta(11, {5, 4})) == "f: holds the invalid Galois element 4");
    CHECK(elements_error("f", meta(11, {2048})).find("invalid Galois element 2048") != std::string::npos);
    CHECK(elements_error("f", meta(11, {2049})).find("invalid") != std::string::npos && elements_error("f", meta(11, {2047})).empty());
    CHECK(elements_error("f", meta(11, {5, 25, 5})) == "f: holds Galois element 5 twice");
    EvkMeta t = r;
    t.entries = 4;
    CHECK(elements_error("f", t) == "f: is truncated");
    t.entries = 65;
    CHECK(elements_error("f", t) == "f: claims 65 entries (at most 64)");
    if (failures) {
        std::printf("evalkeys selftest: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("evalkeys selftest ok\n");
    return 0;
}
