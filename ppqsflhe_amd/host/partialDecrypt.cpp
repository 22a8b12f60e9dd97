// partialDecrypt -- one party's step of a threshold decryption under a joint key (keyGen --join):
// `partialDecrypt <cc_path> <privkey_path> <input_encfile> <share_out> [--lead] [--smudge-bits <s>] [--parties i,j,...]`.
// cc->MultipartyDecryptMain / cc->MultipartyDecryptLead (--lead: exactly one party of a round) -> mkckks_partial_decrypt_batch:
// share = INTT(c1 * s_i (+ c0)) + e, with the smudging errors e drawn on the device from a wide Gaussian of sigma = 2^s
// (mkckks_sample_gauss_wide; default s = 20, the deployment's choice: include/mkckks.h has the noise rule) under a fresh
// OS-drawn key that keys nothing else, stream t for ciphertext t.  One share per ciphertext file per party: a second run
// on the same file draws new errors, and two shares of one ciphertext average the smudging away.
// The output is the input's envelope (JSON or MKWS) with every ciphertext blob replaced by a share blob (share.hpp);
// fuseDecryptions sums the parties' files.  Seeded and plain ciphertext blobs are accepted, as in decryptModelWeights.
// t-of-n: when <privkey_path> is a combined key share sigma_j (combineKeyShares; keyshare.hpp), --parties names the set T of
// the parties that decrypt this round -- at least `threshold` distinct indices, the share's own among them -- and the key
// becomes lambda_j^T * sigma_j (mkckks_lagrange_at_zero, one mkckks_combine_key_shares with m = 1); everything after is
// the same.  Every share that is fused must have been made with the same --parties set, or the round fuses to noise.
#include "keyshare.hpp"
#include "share.hpp"
using namespace mkh;

int main(int argc, char *argv[]) {
    auto usage = [&] {
        std::cerr << "Usage: " << argv[0] << " <cc_path> <privkey_path> <input_encfile> <share_out> [--lead] [--smudge-bits <s>]"
                  << " [--parties i,j,...]" << std::endl;
        return 1;
    };
    if (argc < 5) return usage();
    const std::string cc_path = argv[1], privkey_path = argv[2], input_encfile = argv[3], share_out = argv[4];
    bool lead = false, have_bits = false, have_parties = false;
    std::string bits_arg, parties_arg;
    for (int i = 5; i < argc; ++i) {  // none twice
        const std::string o = argv[i];
        if (o == "--lead" && !lead) {
            lead = true;
        } else if (o == "--smudge-bits" && !have_bits && i + 1 < argc) {
            have_bits = true;
            bits_arg = argv[++i];
        } else if (o == "--parties" && !have_parties && i + 1 < argc) {
            have_parties = true;
            parties_arg = argv[++i];
        } else {
            return usage();
        }
    }
    uint32_t bits = SMUDGE_BITS_DEFAULT;
    if (have_bits && !parse_smudge_bits(bits_arg, bits)) {
        std::cerr << "[pdecrypt] ERROR: --smudge-bits needs an integer in [" << SMUDGE_BITS_MIN << ", " << SMUDGE_BITS_MAX << "]"
                  << std::endl;
        return 1;
    }
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[pdecrypt] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    // a combined key share in the place of the secret key: checked against the CryptoContext file alone, before the device
    const bool is_share = looks_like_keyshare(privkey_path);
    std::vector<uint32_t> parties;
    KeyShare ks;
    if (is_share != have_parties) {
        std::cerr << "[pdecrypt] ERROR: " << (is_share ? "a key share needs --parties" : "--parties needs a combined key share, not a secret key")
                  << std::endl;
        return usage();
    }
    if (is_share) {
        if (!parse_parties(parties_arg, parties)) {
            std::cerr << "[pdecrypt] ERROR: --parties needs distinct party indices in [1, " << MKCKKS_MAX_PARTIES << "], comma separated"
                      << std::endl;
            return usage();
        }
        try {
            const uint32_t N = 1u << cc.p.log_n, L = (uint32_t)cc.moduli.size();
            ks = decode_keyshare_checked(read_keyshare_file(privkey_path, N, L), N, cc.moduli);
        } catch (const std::exception &e) {
            std::cerr << "[pdecrypt] ERROR: " << privkey_path << ": " << e.what() << std::endl;
            return 1;
        }
        bool mine = false, in_range = true;
        for (uint32_t j : parties) {
            mine = mine || j == ks.to_party;
            in_range = in_range && j <= ks.n_parties;
        }
        const char *why = ks.from_party != 0               ? "the key share is one dealer's, not a combined share (combineKeyShares)"
                          : !in_range                      ? "--parties names an index above the share's n_parties"
                          : parties.size() < ks.threshold  ? "--parties names fewer parties than the threshold"
                          : !mine                          ? "--parties does not name the key share's own party"
                                                           : nullptr;
        if (why) {
            std::cerr << "[pdecrypt] ERROR: " << why << std::endl;
            return usage();
        }
    }
    try {
        Session s(cc);
        std::cout << "[pdecrypt] CryptoContext loaded\n";
        const uint32_t N = s.N();
        std::vector<uint64_t> sk;
        std::vector<int8_t> sk_t;
        uint64_t *d_sk = nullptr;
        if (is_share) {  // lambda * sigma_j over the L limbs of Q: all that mkckks_partial_decrypt_batch reads of a key
            const uint32_t L = s.L();
            std::vector<uint64_t> lambda(parties.size() * L);
            Session::check(mkckks_lagrange_at_zero(s.ctx(), parties.data(), (uint32_t)parties.size(), lambda.data()));
            size_t a = 0;
            while (parties[a] != ks.to_party) ++a;
            d_sk = s.to_device(ks.data.data(), ks.data.size());
            Session::check(mkckks_combine_key_shares(s.ctx(), d_sk, &lambda[a * L], d_sk, 1, L));
            std::cout << "[pdecrypt] Key share of party " << ks.to_party << " loaded (" << ks.threshold << "-of-" << ks.n_parties << ", "
                      << parties.size() << " parties this round)\n";
        } else {
            if (!load_secret_key(s, privkey_path, sk, sk_t)) {
                std::cerr << "[pdecrypt] ERROR: Failed to load private key from " << privkey_path << std::endl;
                return 1;
            }
            std::cout << "[pdecrypt] Private key loaded\n";
        }
        Json doc;
        bool binary = false;  // the output keeps the input's envelope form
        try {
            doc = read_envelope(input_encfile, &binary);
        } catch (const std::exception &) {
            std::cerr << "[pdecrypt] ERROR: Could not open input file: " << input_encfile << std::endl;
            return 1;
        }
        raw_blobs() = binary;
        std::cout << "[pdecrypt] Encrypted weights loaded\n";
        const std::vector<CtRef> refs = enumerate_cts(doc);
        std::vector<Ciphertext> cts;
        cts.reserve(refs.size());
        for (const CtRef &r : refs) cts.push_back(decode_ct_checked(ct_string(doc, r), s));
        std::vector<std::string> blobs(cts.size());
        if (!cts.empty()) {
            const uint32_t nl = cts[0].nl;
            for (const Ciphertext &c : cts)
                if (c.nl != nl) throw std::runtime_error("ciphertexts of one file must share a level");
            const size_t words = (size_t)2 * nl * N, B = cts.size(), swords = (size_t)nl * N;
            std::vector<uint64_t> flat(B * words, 0);
            SeedList seeds;
            seeds.resize(B);
            for (size_t i = 0; i < B; ++i) {
                put_payload(&flat[i * words], cts[i]);
                seeds.set(i, cts[i]);
            }
            uint64_t *d_ct = s.to_device(flat.data(), flat.size()), *d_share = s.alloc<uint64_t>(B * swords);
            seeds.expand(s, d_ct, nl, 0, B);
            int64_t *d_e = s.alloc<int64_t>(B * (size_t)N);
            const SamplerKey key = fresh_key();  // this run's smudging only
            const double sigma = std::ldexp(1.0, (int)bits);
            for (size_t t = 0; t < B; ++t)
                Session::check(mkckks_sample_gauss_wide(s.ctx(), d_e + t * N, N, sigma, key.bytes, (uint32_t)t));
            if (!is_share) d_sk = s.to_device(sk.data(), sk.size());
            Session::check(mkckks_partial_decrypt_batch(s.ctx(), d_ct, d_sk, d_e, d_share,
                                                        (uint32_t)B, nl, nl, lead ? 1 : 0));
            std::vector<uint64_t> out(B * swords);
            s.to_host(out.data(), d_share, out.size());
            for (size_t i = 0; i < B; ++i) {
                Share sh;
                sh.nl = nl; sh.level = cts[i].level; sh.noise_deg = cts[i].noise_deg; sh.slots = cts[i].slots;
                sh.scale = cts[i].scale;
                sh.lead = lead;
                sh.data.assign(out.begin() + i * swords, out.begin() + (i + 1) * swords);
                blobs[i] = encode_share(sh, N);
            }
        }
        size_t c = 0;
        for_each_ct_field(doc, [&](Json &field) { field = Json(std::move(blobs.at(c++))); });  // the order of enumerate_cts
        std::cout << "[pdecrypt] " << cts.size() << " " << (lead ? "lead " : "") << "share(s), smudged at sigma 2^" << bits << "\n";
        try {
            write_envelope(doc, share_out, binary);
        } catch (const std::exception &) {
            std::cerr << "[pdecrypt] ERROR: Failed to open output file: " << share_out << std::endl;
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << "[pdecrypt] ERROR: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "[pdecrypt] Partial decryption completed successfully. Output: " << share_out << std::endl;
    return 0;
}
