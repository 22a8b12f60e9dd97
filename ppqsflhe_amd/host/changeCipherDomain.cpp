// changeCipherDomain -- drop-in for server/src/changeCipherDomain.cpp:
// `changeCipherDomain <cc_path> <rekey_path> <input_encfile> <output_encfile>` (:19-29; caller server_fns.sh:65,79).
// The reference loops cc->ReEncrypt(ct, reKey) over mean / std_dev / values[] of every layer (:61-117); here all
// ciphertexts of the file go to HBM once and are re-encrypted by ONE mkckks_reencrypt_batch call.  Seeded ciphertexts
// (encryptModelWeights --seeded) are accepted per blob: c1 is rebuilt on the device; the output is full ciphertexts.
//   changeCipherDomain <cc_path> <rekey_path|-> <input_encfile> <output_encfile> --limbs <k>
// writes the output at k limbs for a receiver that will only decrypt it (the per-key counterpart of serverRound
// --back-limbs): the first k + 1 limbs of every input ciphertext (which must be at noiseScaleDeg 2 with more than k limbs)
// are re-encrypted and rescaled to k by mkckks_reencrypt_fanout_compact_batch; with "-" as the key there is no key switch
// (mkckks_compress_batch).  Headroom rule for k: include/mkckks.h.
//   ... [--hra <source_pubkey> [--hra-sigma-bits <s>]]
// HRA-secure re-encryption, cc->ReEncrypt(ct, reKey, publicKey) (changeCipherDomain.cpp:74 with upstream's third
// argument): every ciphertext of the file is re-randomised under the public key of the domain the INPUT is in before its
// key switch (mkckks_rerandomize_batch; with --limbs k at the k + 1-limb prefix), errors of sigma = 2^s, s in [6, 56],
// default 20 (the deployment's choice; noise rule in include/mkckks.h).  Two runs on one input write different files.
#include <fstream>

#include "hostlib.hpp"
using namespace mkh;

int main(int argc, char *argv[]) {
    auto usage = [&] {
        std::cerr << "Usage: " << argv[0] << " <cc_path> <rekey_path> <input_encfile> <output_encfile>\n       " << argv[0]
                  << " <cc_path> <rekey_path|-> <input_encfile> <output_encfile> --limbs <k>\n       "
                  << "either form followed by [--hra <source_pubkey> [--hra-sigma-bits <s>]]" << std::endl;
        return 1;
    };
    if (argc < 5) return usage();
    const std::string cc_path = argv[1], rekey_path = argv[2], input_encfile = argv[3], output_encfile = argv[4];
    bool compact = false, hra = false, have_bits = false;
    std::string limbs_arg, hra_pk_path, bits_arg;
    for (int i = 5; i < argc; i += 2) {  // options: every one takes a value, none twice, --limbs first (as before)
        const std::string o = argv[i];
        if (i + 1 >= argc) return usage();
        if (o == "--limbs" && i == 5) {
            compact = true;
            limbs_arg = argv[i + 1];
        } else if (o == "--hra" && !hra) {
            hra = true;
            hra_pk_path = argv[i + 1];
        } else if (o == "--hra-sigma-bits" && hra && !have_bits) {
            have_bits = true;
            bits_arg = argv[i + 1];
        } else {
            return usage();
        }
    }
    uint32_t k_limbs = 0, sigma_bits = HRA_SIGMA_BITS_DEFAULT;
    if (compact) {
        const std::string v = limbs_arg;
        if (v.empty() || v.size() > 6 || v.find_first_not_of("0123456789") != std::string::npos || std::atoi(v.c_str()) < 1) {
            std::cerr << "[recrypt] ERROR: --limbs needs a limb count of at least 1" << std::endl;
            return 1;
        }
        k_limbs = (uint32_t)std::atoi(v.c_str());
    }
    if (have_bits && !parse_hra_sigma_bits(bits_arg, sigma_bits)) {
        std::cerr << "[recrypt] ERROR: --hra-sigma-bits needs an integer in [" << HRA_SIGMA_BITS_MIN << ", "
                  << HRA_SIGMA_BITS_MAX << "]" << std::endl;
        return 1;
    }
    if (hra && !compact && rekey_path == "-") {
        std::cerr << "[recrypt] ERROR: --hra with - as the re-encryption key needs --limbs" << std::endl;
        return 1;
    }
    if (hra && !std::ifstream(hra_pk_path)) {
        std::cerr << "[recrypt] ERROR: Failed to load public key from " << hra_pk_path << std::endl;
        return 1;
    }
    const bool keyed = !(compact && rekey_path == "-");
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[recrypt] ERROR: Failed to load CryptoContext: " << cc_path << std::endl;
        return 1;
    }
    try {
        Session s(cc);
        std::cout << "[recrypt] CryptoContext loaded\n";
        const uint32_t N = s.N();
        std::vector<uint64_t> evk;
        if (keyed && !load_eval_key(s, rekey_path, evk)) {
            std::cerr << "[recrypt] ERROR: Failed to load ReKey from " << rekey_path << std::endl;
            return 1;
        }
        if (keyed) std::cout << "[recrypt] ReKey loaded\n";
        std::vector<uint64_t> hra_pk;
        if (hra && !load_public_key(s, hra_pk_path, hra_pk)) {
            std::cerr << "[recrypt] ERROR: Failed to load public key from " << hra_pk_path << std::endl;
            return 1;
        }
        Json inputJson;
        bool binary = false;  // the output keeps the input's envelope form
        try {
            inputJson = read_envelope(input_encfile, &binary);
            raw_blobs() = binary;
        } catch (const std::exception &) {
            std::cerr << "[recrypt] ERROR: Could not open input encrypted weights file\n";
            return 1;
        }
        const std::vector<CtRef> refs = enumerate_cts(inputJson);
        std::vector<Ciphertext> cts;
        cts.reserve(refs.size());
        for (const CtRef &r : refs) cts.push_back(decode_ct_checked(ct_string(inputJson, r), s));
        Json outputJson = inputJson;  // layer / shape carried over; blobs replaced below
        if (!cts.empty()) {
            const uint32_t nl = cts[0].nl;
            for (const Ciphertext &c : cts)
                if (c.nl != nl) throw std::runtime_error("ciphertexts of one file must share a level");
            if (compact)
                for (const Ciphertext &c : cts)
                    if (c.noise_deg != 2 || c.nl <= k_limbs) {
                        std::cerr << "[recrypt] ERROR: --limbs " << k_limbs << " needs input at noiseScaleDeg 2 with more than "
                                  << k_limbs << " limbs (it has noiseScaleDeg " << c.noise_deg << ", " << c.nl << " limbs)"
                                  << std::endl;
                        return 1;
                    }
            const size_t words = (size_t)2 * nl * N;
            std::vector<uint64_t> flat(cts.size() * words, 0);
            SeedList seeds;
            seeds.resize(cts.size());
            for (size_t i = 0; i < cts.size(); ++i) {
                put_payload(&flat[i * words], cts[i]);
                seeds.set(i, cts[i]);
            }
            uint64_t *d_ct = s.to_device(flat.data(), flat.size());
            seeds.expand(s, d_ct, nl, 0, cts.size());
            size_t owords = words;
            uint32_t nl_in = nl;  // limbs per ciphertext of what the key switch reads
            if (hra) {  // in place at full level; into a packed k + 1-limb prefix with --limbs
                const uint32_t rr_nl = compact ? k_limbs + 1 : nl;
                uint64_t *d_rr = compact ? s.alloc<uint64_t>(cts.size() * 2 * rr_nl * N) : d_ct;
                hra_rerandomize(s, d_ct, s.to_device(hra_pk.data(), hra_pk.size()), s.alloc<uint64_t>(hra_scratch_words(cts.size(), N)),
                                d_rr, (uint32_t)cts.size(), nl, rr_nl, sigma_bits, fresh_key());
                d_ct = d_rr;
                nl_in = rr_nl;
                std::cout << "[recrypt] " << cts.size() << " ciphertexts re-randomised at sigma 2^" << sigma_bits << "\n";
            }
            if (!compact) {
                uint64_t *d_evk = s.to_device(evk.data(), evk.size());
                Session::check(mkckks_reencrypt_batch(s.ctx(), d_ct, d_evk, d_ct, (uint32_t)cts.size(), nl));
                s.to_host(flat.data(), d_ct, flat.size());
            } else {
                owords = (size_t)2 * k_limbs * N;
                uint64_t *d_out = s.alloc<uint64_t>(cts.size() * owords);
                if (keyed) {
                    uint64_t *d_evk = s.to_device(evk.data(), evk.size());
                    Session::check(mkckks_reencrypt_fanout_compact_batch(s.ctx(), d_ct, d_evk, d_out, 1, (uint32_t)cts.size(), nl_in,
                                                                         k_limbs));
                } else {
                    Session::check(mkckks_compress_batch(s.ctx(), d_ct, d_out, (uint32_t)cts.size(), nl_in, k_limbs));
                }
                flat.resize(cts.size() * owords);
                s.to_host(flat.data(), d_out, flat.size());
            }
            for (size_t i = 0; i < cts.size(); ++i) {
                cts[i].data.assign(flat.begin() + i * owords, flat.begin() + (i + 1) * owords);
                cts[i].seeded = false;
                if (compact) {  // header of Rescale(prefix(., k + 1))
                    cts[i].level += nl - k_limbs;
                    cts[i].scale = cts[i].scale / (double)s.moduli()[k_limbs];
                    cts[i].nl = k_limbs;
                    cts[i].noise_deg = 1;
                }
                Json &lay = outputJson["weights_summary"].a[refs[i].layer];
                std::string b64 = encode_ct(cts[i], N);
                if (refs[i].field == 0) lay["mean"] = std::move(b64);
                else if (refs[i].field == 1) lay["std_dev"] = std::move(b64);
                else lay["values"].a[refs[i].idx] = Json(std::move(b64));
            }
        }
        try {
            write_envelope(outputJson, output_encfile, binary);
        } catch (const std::exception &) {
            std::cerr << "[recrypt] ERROR: Failed to open output file\n";
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << "[recrypt] ERROR: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "[recrypt] Re-encryption completed successfully. Output: " << output_encfile << std::endl;
    return 0;
}
