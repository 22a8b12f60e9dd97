// product.hpp -- the header bookkeeping of cipherProduct (cc->EvalMult(ct, ct)) and the key kind of relinKeyGen.
// A ciphertext header carries limbs, level (dropped limbs), scale, noiseScaleDeg and slots.  Upstream's EvalMult under
// FLEXIBLEAUTOEXT first rescales a noiseScaleDeg-2 operand (every fresh ciphertext is one), multiplies operands that agree
// in all five fields, and returns limbs and level of the (rescaled) operands, scale S_a * S_b, noiseScaleDeg 2.
// The relinearisation key travels in the eval-key container (hostlib.hpp BlobHeader) under a kind of its own, so a
// re-encryption key or a rotation-key file is refused where a relinearisation key is asked for, and the reverse (their
// readers ask for their own kind).  No dependency on the library: built on its own by product_selftest.cpp.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

namespace mkh {

enum : uint32_t { KIND_RELIN_KEY = 10 };

struct ProductMeta {
    uint32_t nl = 0, level = 0, noise_deg = 0, slots = 0;
    double scale = 0;
};

// what a key container of `kind` is called in messages (kinds of hostlib.hpp, rotkeys.hpp, evalkeys.hpp and this file)
inline std::string key_kind_name(uint32_t kind) {
    switch (kind) {
    case 2: return "a public key";
    case 3: return "a secret key";
    case 4: return "a re-encryption key";
    case 9: return "a rotation-key file";
    case KIND_RELIN_KEY: return "a relinearisation key";
    case 11: return "a rotation-key share";         // evalkeys.hpp: one party's part of a joint key's keys; fuseEvalKeys
    case 12: return "a relinearisation-key share";  // sums all parties' shares into the key
    default: return "a container of kind " + std::to_string(kind);
    }
}
// empty when `kind` is the relinearisation key's, else the refusal
inline std::string relin_kind_error(const std::string &path, uint32_t kind) {
    if (kind == KIND_RELIN_KEY) return "";
    return path + " is " + key_kind_name(kind) + ", not a relinearisation key (relinKeyGen writes one)";
}

// the operand after mkckks_rescale_batch; the error text (empty on success) when it cannot be rescaled
inline std::string product_rescale(const ProductMeta &in, double q_last, ProductMeta &out) {
    if (in.nl < 2) return "noiseScaleDeg-2 operand has no limb left to rescale";
    if (!(q_last > 1)) return "bad modulus";
    out = in;
    out.nl = in.nl - 1;
    out.level = in.level + 1;
    out.scale = in.scale / q_last;
    out.noise_deg = in.noise_deg - 1;
    return "";
}

// the first header field in which the operands differ, empty when they agree
inline std::string product_mismatch(const ProductMeta &a, const ProductMeta &b) {
    if (a.nl != b.nl) return "limbs";
    if (a.level != b.level) return "level";
    if (a.scale != b.scale) return "scale";
    if (a.noise_deg != b.noise_deg) return "noiseScaleDeg";
    if (a.slots != b.slots) return "slots";
    return "";
}

// header of the product of two agreeing noiseScaleDeg-1 operands
inline ProductMeta product_result(const ProductMeta &a, const ProductMeta &b) {
    ProductMeta r = a;
    r.scale = a.scale * b.scale;
    r.noise_deg = a.noise_deg + b.noise_deg;
    return r;
}

// the headroom rule of include/mkckks.h with |values| <= max_abs: log2(S_a S_b max_abs^2) < log2(q_0 ... q_{nl-1}) - 1
inline bool product_has_headroom(const ProductMeta &r, double log2_q, double max_abs) {
    return std::log2(r.scale) + 2 * std::log2(max_abs) < log2_q - 1;
}

}  // namespace mkh
