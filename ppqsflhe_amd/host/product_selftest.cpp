// product_selftest -- the header bookkeeping of cipherProduct (product.hpp) as a stand-alone program without the
// library; built plain and under -fsanitize=address,undefined (Makefile), run by tests/test_product_surface.py.
#include <cstdio>

#include "product.hpp"
using namespace mkh;

static int failures = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                           \
        }                                                         \
    } while (0)

int main() {
    // a fresh ciphertext at the reference parameters: 4 limbs, level 0, scale 2^80, noiseScaleDeg 2
    ProductMeta fresh;
    fresh.nl = 4; fresh.level = 0; fresh.noise_deg = 2; fresh.slots = 8192; fresh.scale = std::ldexp(1.0, 80);
    const double q3 = 1099511480321.0;  // a 40-bit modulus
    ProductMeta a;
    CHECK(product_rescale(fresh, q3, a).empty());
    CHECK(a.nl == 3 && a.level == 1 && a.noise_deg == 1 && a.slots == 8192 && a.scale == fresh.scale / q3);
    // the chain down to one limb, then the refusal
    ProductMeta m = fresh, next;
    for (uint32_t nl = 4; nl >= 2; --nl) {
        CHECK(m.nl == nl);
        CHECK(product_rescale(m, q3, next).empty());
        CHECK(next.nl == nl - 1 && next.level == m.level + 1);
        m = next;
        m.noise_deg = 2;
    }
    CHECK(m.nl == 1);
    CHECK(product_rescale(m, q3, next) == "noiseScaleDeg-2 operand has no limb left to rescale");
    m.nl = 0;
    CHECK(!product_rescale(m, q3, next).empty());
    CHECK(!product_rescale(fresh, 0.0, next).empty() && !product_rescale(fresh, std::nan(""), next).empty());
    // agreement, field by field, in the order limbs, level, scale, noiseScaleDeg, slots
    ProductMeta b = a;
    CHECK(product_mismatch(a, b).empty());
    b.nl = 2;
    CHECK(product_mismatch(a, b) == "limbs" && product_mismatch(b, a) == "limbs");
    b.level = 2;
    CHECK(product_mismatch(a, b) == "limbs");
    b = a; b.level = 2;
    CHECK(product_mismatch(a, b) == "level");
    b = a; b.scale = std::nextafter(a.scale, 0.0);
    CHECK(product_mismatch(a, b) == "scale");
    b = a; b.noise_deg = 2;
    CHECK(product_mismatch(a, b) == "noiseScaleDeg");
    b = a; b.slots = 4096;
    CHECK(product_mismatch(a, b) == "slots");
    b.scale = 1.0;
    CHECK(product_mismatch(a, b) == "scale");
    // the result: limbs, level and slots kept, scale S^2, noiseScaleDeg 2
    const ProductMeta r = product_result(a, a);
    CHECK(r.nl == 3 && r.level == 1 && r.slots == 8192 && r.noise_deg == 2 && r.scale == a.scale * a.scale);
    ProductMeta c = a;
    c.scale = 3.0;
    CHECK(product_result(a, c).scale == a.scale * 3.0);
    // headroom: S^2 is about 2^80.0; three limbs of 60 + 40 + 40 bits hold it, one 60-bit limb does not
    CHECK(product_has_headroom(r, 140.0, 1.0) && product_has_headroom(r, 140.0, 1024.0));
    CHECK(!product_has_headroom(r, 60.0, 1.0) && !product_has_headroom(r, 81.0, 1.0) && product_has_headroom(r, 82.0, 1.0));
    CHECK(!product_has_headroom(r, 82.0, 2.0));
    // key kinds
    CHECK(relin_kind_error("k", KIND_RELIN_KEY).empty());
    CHECK(relin_kind_error("k", 4) == "k is a re-encryption key, not a relinearisation key (relinKeyGen writes one)");
    CHECK(relin_kind_error("k", 9) == "k is a rotation-key file, not a relinearisation key (relinKeyGen writes one)");
    CHECK(relin_kind_error("k", 2).find("a public key") != std::string::npos);
    CHECK(relin_kind_error("k", 3).find("a secret key") != std::string::npos);
    CHECK(relin_kind_error("k", 77).find("a container of kind 77") != std::string::npos);
    CHECK(relin_kind_error("k", 0xFFFFFFFFu).find("4294967295") != std::string::npos);
    if (failures) {
        std::printf("product selftest: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("product selftest ok\n");
    return 0;
}
