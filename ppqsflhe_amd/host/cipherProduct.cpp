// cipherProduct -- the slot-wise product of two encrypted-weights files under ONE key:
// `cipherProduct <cc_path> <relinkey> <input_encfile_A> <input_encfile_B> <output_encfile>`.
// cc->EvalMult(ct, ct): an upstream call the reference never makes.  Entries are paired by (layer, shape) as
// aggregateEncryptedWeights pairs them; every pair of ciphertexts (mean / std_dev / values[]) is multiplied and
// relinearised by ONE mkckks_mult_relin_batch.  The operands must agree in limbs, level, scale, noiseScaleDeg and slots;
// noiseScaleDeg-2 operands (every fresh ciphertext) are rescaled first, as upstream's EvalMult does.  The result carries
// limbs and level of the (rescaled) operands, scale S^2, noiseScaleDeg 2 and the operands' slots (product.hpp); it is an
// ordinary ciphertext envelope in the form of input A (JSON or MKWS): slotSum and decryptModelWeights take it unchanged,
// so the encrypted inner product <a, b> is cipherProduct followed by slotSum.  The same path given twice squares
// (two polynomials are read per ciphertext instead of four).
// <relinkey> is the file relinKeyGen wrote for the key the inputs are under; any other key container is refused by kind.
// Header refusals are decided before a device is opened.
#include "hostlib.hpp"
#include "product.hpp"
using namespace mkh;

// the container header of a ciphertext blob (raw or base64) without its payload
static bool peek_ct_header(const std::string &blob, BlobHeader &h) {
    const bool raw = blob.size() >= 4 && !std::memcmp(blob.data(), "MKCK", 4);
    std::string bin;
    if (raw) {
        bin = blob.substr(0, sizeof h);
    } else {
        try {
            bin = Base64Decode(blob.substr(0, 64));  // 64 characters hold the 48 header bytes
        } catch (const std::exception &) {
            return false;
        }
    }
    if (bin.size() < sizeof h) return false;
    std::memcpy(&h, bin.data(), sizeof h);
    return !std::memcmp(h.magic, "MKCK", 4) && h.version == 1 && (h.kind == KIND_CT || h.kind == KIND_CT_SEEDED);
}

static ProductMeta meta_of(const BlobHeader &h) {
    ProductMeta m;
    m.nl = h.limbs; m.level = h.level; m.noise_deg = h.noise_deg; m.slots = h.slots; m.scale = h.scale;
    return m;
}

int main(int argc, char *argv[]) {
    if (argc != 6) {
        std::cerr << "Usage: " << argv[0] << " <cc_path> <relinkey> <input_encfile_A> <input_encfile_B> <output_encfile>" << std::endl;
        return 1;
    }
    const std::string cc_path = argv[1], key_path = argv[2], in_a = argv[3], in_b = argv[4], output_encfile = argv[5];
    const bool square = in_a == in_b;
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[product] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    {
        std::unique_ptr<FILE, FileCloser> f(std::fopen(key_path.c_str(), "rb"));
        BlobHeader h;
        if (!f || std::fread(&h, sizeof h, 1, f.get()) != 1 || std::memcmp(h.magic, "MKCK", 4) || h.version != 1) {
            std::cerr << "[product] ERROR: Failed to load the relinearisation key from " << key_path << std::endl;
            return 1;
        }
        const std::string err = relin_kind_error(key_path, h.kind);
        if (!err.empty()) {
            std::cerr << "[product] ERROR: " << err << std::endl;
            return 1;
        }
    }
    std::vector<Json> files(square ? 1 : 2);
    bool binary = false;  // the output keeps the form of input A
    for (size_t f = 0; f < files.size(); ++f) {
        const std::string &path = f ? in_b : in_a;
        try {
            bool bin = false;
            files[f] = read_envelope(path, &bin);
            if (f == 0) binary = bin;
        } catch (const std::exception &) {
            std::cerr << "[product] ERROR: Could not open input encrypted weights file " << path << std::endl;
            return 1;
        }
    }
    raw_blobs() = binary;
    try {
        Json outputJson;
        const std::vector<AggItem> items = build_agg_items(files, outputJson);
        const size_t B = items.size(), F = files.size();
        ProductMeta op[2];
        for (size_t b = 0; b < B; ++b)
            for (size_t f = 0; f < F; ++f) {
                BlobHeader h;
                if (!peek_ct_header(*items[b].blobs[f], h)) {
                    std::cerr << "[product] ERROR: operand " << (f ? "B" : "A") << " holds a field that is no ciphertext" << std::endl;
                    return 1;
                }
                const ProductMeta m = meta_of(h);
                if (b == 0) op[f] = m;
                const std::string diff = product_mismatch(op[f], m);
                if (!diff.empty()) {
                    std::cerr << "[product] ERROR: the ciphertexts of operand " << (f ? "B" : "A") << " differ in " << diff << std::endl;
                    return 1;
                }
            }
        if (square) op[1] = op[0];
        if (B) {
            const std::string diff = product_mismatch(op[0], op[1]);
            if (!diff.empty()) {
                std::cerr << "[product] ERROR: the operands differ in " << diff << " (EvalMult needs equal limbs, level, scale, "
                          << "noiseScaleDeg and slots)" << std::endl;
                return 1;
            }
            if (op[0].noise_deg != 1 && op[0].noise_deg != 2) {
                std::cerr << "[product] ERROR: ciphertext: noiseScaleDeg must be 1 or 2" << std::endl;
                return 1;
            }
            if (op[0].noise_deg == 2 && op[0].nl < 2) {
                std::cerr << "[product] ERROR: no limb left to rescale: the operands have noiseScaleDeg 2 and " << op[0].nl
                          << " limb(s)" << std::endl;
                return 1;
            }
        }
        if (B) {
            Session s(cc);
            const uint32_t N = s.N(), D = s.D(), beta = s.beta();
            std::vector<uint64_t> rlk;
            if (!read_key_file(key_path, KIND_RELIN_KEY, N, D, 2 * beta, rlk)) {
                std::cerr << "[product] ERROR: the relinearisation key " << key_path << " does not match the CryptoContext" << std::endl;
                return 1;
            }
            std::vector<uint64_t> flat;
            SeedList seeds;
            const Ciphertext first = gather_agg_inputs(items, F, s, flat, seeds);
            uint32_t nl = first.nl;
            uint64_t *d_in = s.to_device(flat.data(), flat.size());
            seeds.expand(s, d_in, nl, 0, F * B);
            ProductMeta m = op[0];
            if (m.noise_deg == 2) {  // EvalMult's ModReduce of both operands, one call over [file][item]
                uint64_t *d_rs = s.alloc<uint64_t>(F * B * (size_t)2 * (nl - 1) * N);
                Session::check(mkckks_rescale_batch(s.ctx(), d_in, d_rs, (uint32_t)(F * B), nl));
                const std::string err = product_rescale(op[0], (double)s.moduli()[nl - 1], m);
                if (!err.empty()) throw std::runtime_error(err);
                d_in = d_rs;
                nl = m.nl;
            }
            const ProductMeta r = product_result(m, m);
            double log_q = 0;
            for (uint32_t i = 0; i < nl; ++i) log_q += std::log2((double)s.moduli()[i]);
            if (!product_has_headroom(r, log_q, 1.0)) {
                std::cerr << "[product] ERROR: no headroom: the product's scale needs log2(S^2) = " << std::log2(r.scale)
                          << " bits below the " << log_q << " bits of its " << nl << " limb(s)" << std::endl;
                return 1;
            }
            const uint64_t *d_rlk = s.to_device(rlk.data(), rlk.size());
            uint64_t *d_a = d_in, *d_b = square ? d_in : d_in + B * (size_t)2 * nl * N;
            Session::check(mkckks_mult_relin_batch(s.ctx(), d_a, d_b, d_rlk, d_a, (uint32_t)B, nl));
            Ciphertext meta;
            meta.nl = r.nl; meta.level = r.level; meta.noise_deg = r.noise_deg; meta.slots = r.slots; meta.scale = r.scale;
            store_agg_items(s, items, d_a, meta, outputJson);
            std::cout << "[product] " << B << " ciphertext product(s)" << (square ? " (squares)" : "") << " on " << nl
                      << " limb(s), scale 2^" << std::log2(r.scale) << "\n";
        }
        try {
            write_envelope(outputJson, output_encfile, binary);
        } catch (const std::exception &) {
            std::cerr << "[product] ERROR: Failed to open output file " << output_encfile << std::endl;
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << "[product] ERROR: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "[product] Ciphertext product completed successfully. Output: " << output_encfile << std::endl;
    return 0;
}
