// fuseDecryptions -- the closing step of a threshold decryption: `fuseDecryptions <cc_path> <share_1> ... <share_n> <output_file>`.
// cc->MultipartyDecryptFusion -> mkckks_fuse_shares_batch (the sum of the parties' shares), then exactly the decode of
// decryptModelWeights: mkckks_decode_batch, or mkckks_decode_flood_batch under MKCKKS_DECRYPT_NOISE=flood, and the same
// plaintext JSON.  It needs no key: anyone who holds the n share files of a round can run it.
// Nothing in a share file is trusted (share.hpp).  The program refuses, before it touches the device, unless every blob
// position has exactly one lead share, the files agree in layers, shapes, levels and scales, and every word is below its
// modulus.  What it cannot see: whether the n files are shares of the SAME ciphertext file by n DIFFERENT parties of the
// key chain -- any n - 1 of them, or a foreign one among them, fuse to noise, not to an error.
#include "share.hpp"
using namespace mkh;

int main(int argc, char *argv[]) {
    if (argc < 4) {
        std::cerr << "Usage: " << argv[0] << " <cc_path> <share_1> [<share_2> ...] <output_file>" << std::endl;
        return 1;
    }
    const std::string cc_path = argv[1], output_file = argv[argc - 1];
    const size_t n = (size_t)argc - 3;
    bool flood = false;
    if (const char *e = std::getenv("MKCKKS_DECRYPT_NOISE")) {
        const std::string mode = e;
        if (mode == "flood") {
            flood = true;
        } else if (!mode.empty() && mode != "off") {
            std::cerr << "[fuse] ERROR: MKCKKS_DECRYPT_NOISE must be \"flood\" or \"off\", not \"" << mode << "\"" << std::endl;
            return 1;
        }
    }
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[fuse] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    try {
        // the share files, checked against the CryptoContext file alone (ring dimension and the moduli of Q it lists)
        const uint32_t N = 1u << cc.p.log_n;
        std::vector<Json> docs(n);
        std::vector<std::vector<Share>> shares(n);
        for (size_t p = 0; p < n; ++p) {
            const std::string path = argv[2 + p];
            try {
                docs[p] = read_envelope(path);
            } catch (const std::exception &) {
                std::cerr << "[fuse] ERROR: Could not open share file: " << path << std::endl;
                return 1;
            }
            try {
                for (const CtRef &r : enumerate_cts(docs[p]))
                    shares[p].push_back(decode_share_checked(ct_string(docs[p], r), N, cc.moduli));
            } catch (const std::exception &e) {
                std::cerr << "[fuse] ERROR: " << path << ": " << e.what() << std::endl;
                return 1;
            }
        }
        const size_t B = shares[0].size();
        auto same_layout = [&](size_t p) {
            const Json &a = docs[0].at("weights_summary"), &b = docs[p].at("weights_summary");
            if (a.size() != b.size() || shares[p].size() != B) return false;
            for (size_t l = 0; l < a.size(); ++l)
                if (!(a.at(l).at("layer") == b.at(l).at("layer") && a.at(l).at("shape") == b.at(l).at("shape")) ||
                    a.at(l).at("values").size() != b.at(l).at("values").size())
                    return false;
            for (size_t i = 0; i < B; ++i) {
                const Share &x = shares[0][0], &y = shares[p][i];  // one level and one scale per file, as decryptModelWeights
                if (x.nl != y.nl || x.level != y.level || x.noise_deg != y.noise_deg || x.scale != y.scale || x.slots != y.slots)
                    return false;
            }
            return true;
        };
        for (size_t p = 0; p < n; ++p)
            if (!same_layout(p)) {
                std::cerr << "[fuse] ERROR: " << argv[2 + p] << ": shares differ in layers, shapes, levels or scales" << std::endl;
                return 1;
            }
        for (size_t i = 0; i < B; ++i) {
            size_t leads = 0;
            for (size_t p = 0; p < n; ++p) leads += shares[p][i].lead ? 1 : 0;
            if (leads != 1) {
                std::cerr << "[fuse] ERROR: need exactly one lead share per ciphertext (position " << i << " has " << leads << ")"
                          << std::endl;
                return 1;
            }
        }
        std::cout << "[fuse] " << n << " share file(s) loaded, " << B << " ciphertext position(s)\n";
        std::vector<std::vector<double>> decoded(B);
        if (B) {
            Session s(cc);
            std::cout << "[fuse] CryptoContext loaded\n";
            const uint32_t nl = shares[0][0].nl;
            const double scale = shares[0][0].scale;
            const size_t swords = (size_t)nl * N;
            std::vector<uint64_t> flat(n * B * swords);
            for (size_t p = 0; p < n; ++p)
                for (size_t i = 0; i < B; ++i)
                    std::memcpy(&flat[(p * B + i) * swords], shares[p][i].data.data(), swords * 8);
            uint64_t *d_shares = s.to_device(flat.data(), flat.size());
            uint64_t *d_m = d_shares;  // into shares[0]
            Session::check(mkckks_fuse_shares_batch(s.ctx(), d_shares, d_m, (uint32_t)n, (uint32_t)B, nl));
            const size_t slots = s.slots();
            double *d_vals = s.alloc<double>(B * slots);
            if (flood) {
                const SamplerKey key = fresh_key();
                const int rc = mkckks_decode_flood_batch(s.ctx(), d_m, d_vals, (uint32_t)B, nl, scale, key.bytes, 0, nullptr);
                if (rc == MKCKKS_E_PRECISION) {  // upstream's Decode throws; no output file
                    std::cerr << "[fuse] ERROR: The decryption failed because the approximation error is too high. "
                                 "Check the parameters."
                              << std::endl;
                    return 1;
                }
                Session::check(rc);
            } else {
                Session::check(mkckks_decode_batch(s.ctx(), d_m, d_vals, (uint32_t)B, nl, scale));
            }
            std::vector<double> vals(B * slots);
            s.to_host(vals.data(), d_vals, vals.size());
            for (size_t i = 0; i < B; ++i) decoded[i].assign(vals.begin() + i * slots, vals.begin() + (i + 1) * slots);
        }
        const size_t batch = cc.batch ? cc.batch : N / 2;
        Json plainJson = Json::object();
        plainJson["weights_summary"] = Json::array();
        size_t c = 0;
        for (const Json &encLayer : docs[0].at("weights_summary").a) {  // the document decryptModelWeights writes
            Json plainLayer = Json::object();
            plainLayer["layer"] = encLayer.at("layer");
            plainLayer["shape"] = encLayer.at("shape");
            plainLayer["mean"] = decoded[c++][0];
            plainLayer["std_dev"] = decoded[c++][0];
            size_t expected = 1;
            for (const Json &dim : encLayer.at("shape").a) expected *= (size_t)dim.as_int();
            Json samples = Json::array();
            std::vector<double> all;
            for (size_t k = 0; k < encLayer.at("values").size(); ++k) {
                const std::vector<double> &v = decoded[c++];
                all.insert(all.end(), v.begin(), v.begin() + std::min<size_t>(batch, v.size()));
            }
            if (all.size() > expected) all.resize(expected);  // trim the zero padding
            for (double v : all) samples.push_back(Json(v));
            plainLayer["values"] = samples;
            plainJson["weights_summary"].push_back(plainLayer);
        }
        try {
            plainJson.write_file(output_file);
        } catch (const std::exception &) {
            std::cerr << "[fuse] ERROR: Failed to open output file: " << output_file << std::endl;
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << "[fuse] ERROR: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "[fuse] Fusion completed successfully. Output: " << output_file << std::endl;
    return 0;
}
