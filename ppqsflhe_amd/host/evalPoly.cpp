// evalPoly -- a polynomial of every slot of every ciphertext of an encrypted-weights file:
// `evalPoly <cc_path> <relinkey> <input_encfile> <output_encfile> --coeffs c0,c1,...,cd [--max-abs A]`.
// cc->EvalPoly: an upstream call the reference never makes.  p(x) = c0 + c1 x + ... + cd x^d in the power basis,
// 2 <= d <= 63, is applied slot-wise to mean / std_dev / values[] of every layer by ONE mkckks_poly_eval_batch (the fused
// Paterson-Stockmeyer evaluation of include/mkckks.h).  A noiseScaleDeg-2 input (every fresh ciphertext) is rescaled
// first, as cipherProduct does.  The result carries nl_out = nl - depth limbs, level L - nl_out, the standard scale of that
// level and noiseScaleDeg 1 (poly.hpp): an ordinary ciphertext envelope in the input's form, which cipherProduct, slotSum
// and decryptModelWeights take unchanged -- clipping under encryption is cipherProduct -> slotSum -> evalPoly -> cipherProduct.
// Refused: a degree whose plan does not fit the input's limbs (the message names the limbs needed), before a device is
// opened; a --max-abs A (default 1) for which the headroom rule Sigma * sum |c_k| A^k < q_0 ... q_{nl_T-1} / 2 fails.
// `--cheb a,b` reads --coeffs as a Chebyshev series on [a, b], p(x) = sum_k c_k T_k(u) with u the map of [a, b] onto [-1, 1]
// (cc->EvalChebyshevSeries; c_0 is the plain coefficient of T_0), or fits one itself: `--function {invsqrt,sigmoid,tanh,exp}
// --degree d` interpolates at the d + 1 Chebyshev nodes of [a, b] (cc->EvalChebyshevFunction) and prints the coefficients.
// ONE mkckks_cheb_eval_batch; an interval other than [-1, 1] costs one more limb.  --max-abs has no place in this mode:
// |T_k| <= 1 on the interval, so the headroom check is Sigma * sum |m_{j,i}| < q_0 ... q_{nl_T-1} / 2 over the rewritten
// coefficients of poly.hpp; it is always on, decided before anything is uploaded, and printed.
// <relinkey> is the file relinKeyGen wrote for the key the input is under (a joint key's collective one included); any
// other key container is refused by kind.
#include "hostlib.hpp"
#include "poly.hpp"
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

int main(int argc, char *argv[]) {
    auto usage = [&] {
        std::cerr << "Usage: " << argv[0] << " <cc_path> <relinkey> <input_encfile> <output_encfile> --coeffs c0,c1,...,cd [--max-abs A]"
                  << std::endl
                  << "       " << argv[0] << " <cc_path> <relinkey> <input_encfile> <output_encfile> --cheb a,b"
                  << " (--coeffs c0,c1,...,cd | --function {invsqrt,sigmoid,tanh,exp} --degree d)" << std::endl;
        return 1;
    };
    if (argc < 7 || (argc - 5) % 2) return usage();
    const std::string cc_path = argv[1], key_path = argv[2], input_encfile = argv[3], output_encfile = argv[4];
    std::vector<double> coef;
    bool have_coef = false, have_abs = false, cheb = false, have_degree = false;
    double max_abs = 1.0, iv_a = -1.0, iv_b = 1.0;
    std::string function;
    uint32_t fit_degree = 0;
    for (int i = 5; i < argc; i += 2) {
        const std::string o = argv[i];
        if (o == "--coeffs" && !have_coef) {
            const std::string err = parse_coeffs(argv[i + 1], coef);
            if (!err.empty()) {
                std::cerr << "[evalpoly] ERROR: " << err << std::endl;
                return 1;
            }
            have_coef = true;
        } else if (o == "--max-abs" && !have_abs) {
            char *rest = nullptr;
            max_abs = std::strtod(argv[i + 1], &rest);
            if (rest == argv[i + 1] || *rest || !(max_abs > 0) || !std::isfinite(max_abs)) {
                std::cerr << "[evalpoly] ERROR: --max-abs needs a positive number" << std::endl;
                return 1;
            }
            have_abs = true;
        } else if (o == "--cheb" && !cheb) {
            const std::string err = parse_interval(argv[i + 1], iv_a, iv_b);
            if (!err.empty()) {
                std::cerr << "[evalpoly] ERROR: " << err << std::endl;
                return 1;
            }
            cheb = true;
        } else if (o == "--function" && function.empty()) {
            function = argv[i + 1];
            if (function.empty()) return usage();
        } else if (o == "--degree" && !have_degree) {
            char *rest = nullptr;
            const long v = std::strtol(argv[i + 1], &rest, 10);
            if (rest == argv[i + 1] || *rest || v < 0 || v > 1000) {
                std::cerr << "[evalpoly] ERROR: --degree needs a whole number" << std::endl;
                return 1;
            }
            fit_degree = (uint32_t)v;
            have_degree = true;
        } else {
            return usage();
        }
    }
    if (cheb) {
        // a series given or a series fitted, never both; the power basis' --max-abs has no meaning here
        if (have_abs || have_coef == !function.empty() || have_degree != !function.empty()) return usage();
        if (!function.empty()) {
            const std::string err = cheb_function_error(function, fit_degree, iv_a, iv_b);
            if (!err.empty()) {
                std::cerr << "[evalpoly] ERROR: " << err << std::endl;
                return 1;
            }
            coef = cheb_fit(cheb_function(function), iv_a, iv_b, fit_degree);
            char num[40];
            std::cout << "[evalpoly] " << function << " on [" << iv_a << ", " << iv_b << "], degree " << fit_degree << ": series ";
            for (size_t k = 0; k < coef.size(); ++k) {
                std::snprintf(num, sizeof num, "%.17g", coef[k]);
                std::cout << (k ? "," : "") << num;
            }
            std::cout << std::endl;
        }
    } else if (!have_coef || !function.empty() || have_degree) {
        return usage();
    }
    const bool mapped = cheb && cheb_mapped(iv_a, iv_b);
    const uint32_t degree = (uint32_t)coef.size() - 1;
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[evalpoly] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    {
        std::unique_ptr<FILE, FileCloser> f(std::fopen(key_path.c_str(), "rb"));
        BlobHeader h;
        if (!f || std::fread(&h, sizeof h, 1, f.get()) != 1 || std::memcmp(h.magic, "MKCK", 4) || h.version != 1) {
            std::cerr << "[evalpoly] ERROR: Failed to load the relinearisation key from " << key_path << std::endl;
            return 1;
        }
        const std::string err = relin_kind_error(key_path, h.kind);
        if (!err.empty()) {
            std::cerr << "[evalpoly] ERROR: " << err << std::endl;
            return 1;
        }
    }
    std::vector<Json> files(1);
    bool binary = false;  // the output keeps the input's envelope form
    try {
        files[0] = read_envelope(input_encfile, &binary);
    } catch (const std::exception &) {
        std::cerr << "[evalpoly] ERROR: Could not open input encrypted weights file " << input_encfile << std::endl;
        return 1;
    }
    raw_blobs() = binary;
    try {
        Json outputJson;
        const std::vector<AggItem> items = build_agg_items(files, outputJson);
        const size_t B = items.size();
        ProductMeta in;
        for (size_t b = 0; b < B; ++b) {
            BlobHeader h;
            if (!peek_ct_header(*items[b].blobs[0], h)) {
                std::cerr << "[evalpoly] ERROR: the input holds a field that is no ciphertext" << std::endl;
                return 1;
            }
            ProductMeta m;
            m.nl = h.limbs; m.level = h.level; m.noise_deg = h.noise_deg; m.slots = h.slots; m.scale = h.scale;
            if (b == 0) in = m;
            const std::string diff = product_mismatch(in, m);
            if (!diff.empty()) {
                std::cerr << "[evalpoly] ERROR: the ciphertexts of the input differ in " << diff << std::endl;
                return 1;
            }
        }
        if (B) {
            if (in.noise_deg != 1 && in.noise_deg != 2) {
                std::cerr << "[evalpoly] ERROR: ciphertext: noiseScaleDeg must be 1 or 2" << std::endl;
                return 1;
            }
            const uint32_t nl_eval = in.noise_deg == 2 ? (in.nl ? in.nl - 1 : 0) : in.nl;  // after the input's own rescale
            const std::string fit = cheb ? cheb_fit_error(degree, nl_eval, mapped) : poly_fit_error(degree, nl_eval);
            if (!fit.empty()) {
                std::cerr << "[evalpoly] ERROR: " << fit << (in.noise_deg == 2 ? " after the rescale of its noiseScaleDeg-2 form" : "")
                          << std::endl;
                return 1;
            }
            Session s(cc);
            const uint32_t N = s.N(), D = s.D(), beta = s.beta();
            const PolyPlan hp = poly_plan(degree);
            if (cheb) {
                // the headroom of the series, from headers and host tables alone: nothing has been uploaded yet
                const uint32_t nl_T = nl_eval - (mapped ? 1 : 0) - (hp.depth - 2), nl_out = nl_T - 2;
                double log_q = 0, need = 0;
                for (uint32_t i = 0; i < nl_T; ++i) log_q += std::log2((double)s.moduli()[i]);
                const double log_sigma = std::log2(s.sf(s.L() - nl_out, false)) + std::log2((double)s.moduli()[nl_T - 1]) +
                                         std::log2((double)s.moduli()[nl_T - 2]);
                const std::string herr = cheb_headroom_error(cheb_rewrite(coef, hp.B, hp.G), log_sigma, log_q, &need);
                if (!herr.empty()) {
                    std::cerr << "[evalpoly] ERROR: " << herr << std::endl;
                    return 1;
                }
                std::cout << "[evalpoly] headroom: the outer sum needs " << need << " of the " << log_q - 1 << " bits its limbs hold\n";
            }
            std::vector<uint64_t> rlk;
            if (!read_key_file(key_path, KIND_RELIN_KEY, N, D, 2 * beta, rlk)) {
                std::cerr << "[evalpoly] ERROR: the relinearisation key " << key_path << " does not match the CryptoContext" << std::endl;
                return 1;
            }
            std::vector<uint64_t> flat;
            SeedList seeds;
            const Ciphertext first = gather_agg_inputs(items, 1, s, flat, seeds);
            uint32_t nl = first.nl;
            uint64_t *d_in = s.to_device(flat.data(), flat.size());
            seeds.expand(s, d_in, nl, 0, B);
            ProductMeta m = in;
            if (m.noise_deg == 2) {
                uint64_t *d_rs = s.alloc<uint64_t>(B * (size_t)2 * (nl - 1) * N);
                Session::check(mkckks_rescale_batch(s.ctx(), d_in, d_rs, (uint32_t)B, nl));
                const std::string err = product_rescale(in, (double)s.moduli()[nl - 1], m);
                if (!err.empty()) throw std::runtime_error(err);
                d_in = d_rs;
                nl = m.nl;
            }
            struct mkckks_poly_plan plan;
            Session::check(mkckks_poly_plan(s.ctx(), degree, nl - (mapped ? 1 : 0), &plan));
            if (plan.B != hp.B || plan.G != hp.G || plan.depth != hp.depth) throw std::runtime_error("the library's plan differs from poly.hpp's");
            const double s_out = s.sf(s.L() - plan.nl_out, false);
            double log_q = 0;
            for (uint32_t i = 0; i < plan.nl_T; ++i) log_q += std::log2((double)s.moduli()[i]);
            const double log_sigma = std::log2(s_out) + std::log2((double)s.moduli()[plan.nl_T - 1]) + std::log2((double)s.moduli()[plan.nl_T - 2]);
            const std::string herr = cheb ? "" : poly_headroom_error(coef, max_abs, log_sigma, log_q);
            if (!herr.empty()) {
                std::cerr << "[evalpoly] ERROR: " << herr << std::endl;
                return 1;
            }
            const uint64_t *d_rlk = s.to_device(rlk.data(), rlk.size());
            uint64_t *d_out = s.alloc<uint64_t>(B * (size_t)2 * plan.nl_out * N);
            double got_scale = 0;
            if (cheb)
                Session::check(mkckks_cheb_eval_batch(s.ctx(), d_in, d_rlk, coef.data(), degree, iv_a, iv_b, d_out, (uint32_t)B, nl, m.scale,
                                                      &got_scale));
            else
                Session::check(mkckks_poly_eval_batch(s.ctx(), d_in, d_rlk, coef.data(), degree, d_out, (uint32_t)B, nl, m.scale, &got_scale));
            PolyPlan spent = hp;
            spent.depth += mapped ? 1 : 0;
            const ProductMeta r = poly_result(m, spent, got_scale);
            Ciphertext meta;
            meta.nl = r.nl; meta.level = r.level; meta.noise_deg = r.noise_deg; meta.slots = r.slots; meta.scale = r.scale;
            store_agg_items(s, items, d_out, meta, outputJson);
            if (cheb) std::cout << "[evalpoly] Chebyshev series on [" << iv_a << ", " << iv_b << "]" << (mapped ? ", one limb for the map" : "") << "\n";
            std::cout << "[evalpoly] degree " << degree << " on " << B << " ciphertext(s): B " << plan.B << ", G " << plan.G << ", "
                      << plan.n_relin << " relinearisation(s), " << nl << " -> " << r.nl << " limb(s), scale 2^" << std::log2(r.scale) << "\n";
        }
        try {
            write_envelope(outputJson, output_encfile, binary);
        } catch (const std::exception &) {
            std::cerr << "[evalpoly] ERROR: Failed to open output file " << output_encfile << std::endl;
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << "[evalpoly] ERROR: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "[evalpoly] Polynomial evaluation completed successfully. Output: " << output_encfile << std::endl;
    return 0;
}
