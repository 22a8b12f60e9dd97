// switchShare -- one party's step of the collective key switch of a joint-key aggregate to a RECIPIENT's public key
// ("deliver instead of open"; Mouchet et al., PCKS):
// `switchShare <cc_path> <privkey_path> <recipient_pubkey> <agg_encfile> <share_out> [--lead] [--smudge-bits <s>]
//              [--parties i,j,...] [--limbs <m>]`.
// mkckks_switch_share_batch: share = (c1 * s_i (+ c0) + b v + e0, a v + e1) with (b, a) the recipient's key; the sum of
// the parties' shares (fuseSwitchShares) is a ciphertext under the recipient's key, and nobody on the way sees the
// plaintext.  Randomness, drawn on the device under THREE fresh OS-drawn keys that key nothing else, stream t for
// ciphertext t: v ternary (mkckks_sample_ternary), e0 the smudging error from a wide Gaussian of sigma = 2^s
// (mkckks_sample_gauss_wide; s in [6, 56], default 20: the deployment's choice, as in partialDecrypt), e1 an ordinary
// encryption error of the scheme's sigma = 3.19.  One share per aggregate file per party AND recipient; r recipients of
// one aggregate receive r independently smudged copies of c1 * s_i: add log2(r) / 2 bits of smudging (include/mkckks.h).
// --lead: exactly one party of a round.  --parties: as in partialDecrypt, <privkey_path> is a combined key share sigma_j
// and the key becomes lambda_j^T * sigma_j.  --limbs m, for a recipient that will only decrypt: the delivered ciphertext
// has m limbs (default: all of the aggregate's, as it stands).  For m below the aggregate's limbs this is the compaction of
// changeCipherDomain --limbs / serverRound --back-limbs, in its order: the share is made at the aggregate's first m + 1
// limbs, where the smudging is added at the aggregate's own scale ~ 2^(2p), and fuseSwitchShares closes with the rescale to
// m limbs (the share's header says so) -- a party must not rescale its own share: that would divide the smudging away.
// Headroom, as in INTEGRATION.md "Who picks k" with k = m: q_0 ... q_m / 2 must exceed scale * |values| + noise at the
// aggregate's OWN scale; with a 60-bit q_0 and p-bit limbs m = 1 holds |values| < 2^(58-p).  The program cannot check it,
// the values are encrypted.  The aggregate must stand at noiseScaleDeg 2 for m below its limbs.
// The output is the input's envelope (JSON or MKWS) with every ciphertext blob replaced by a key-switch share blob
// (switchshare.hpp, kind 8).
#include "keyshare.hpp"
#include "share.hpp"
#include "switchshare.hpp"
using namespace mkh;

int main(int argc, char *argv[]) {
    auto usage = [&] {
        std::cerr << "Usage: " << argv[0] << " <cc_path> <privkey_path> <recipient_pubkey> <agg_encfile> <share_out> [--lead]"
                  << " [--smudge-bits <s>] [--parties i,j,...] [--limbs <m>]" << std::endl;
        return 1;
    };
    if (argc < 6) return usage();
    const std::string cc_path = argv[1], privkey_path = argv[2], pubkey_path = argv[3], input_encfile = argv[4], share_out = argv[5];
    bool lead = false, have_bits = false, have_parties = false, have_limbs = false;
    std::string bits_arg, parties_arg, limbs_arg;
    for (int i = 6; i < argc; ++i) {  // none twice
        const std::string o = argv[i];
        if (o == "--lead" && !lead) {
            lead = true;
        } else if (o == "--smudge-bits" && !have_bits && i + 1 < argc) {
            have_bits = true;
            bits_arg = argv[++i];
        } else if (o == "--parties" && !have_parties && i + 1 < argc) {
            have_parties = true;
            parties_arg = argv[++i];
        } else if (o == "--limbs" && !have_limbs && i + 1 < argc) {
            have_limbs = true;
            limbs_arg = argv[++i];
        } else {
            return usage();
        }
    }
    uint32_t bits = SMUDGE_BITS_DEFAULT, limbs = 0;
    if (have_bits && !parse_smudge_bits(bits_arg, bits)) {
        std::cerr << "[kswitch] ERROR: --smudge-bits needs an integer in [" << SMUDGE_BITS_MIN << ", " << SMUDGE_BITS_MAX << "]"
                  << std::endl;
        return 1;
    }
    if (have_limbs && !parse_limbs(limbs_arg, limbs)) {
        std::cerr << "[kswitch] ERROR: --limbs needs an integer in [1, the aggregate's limbs]" << std::endl;
        return 1;
    }
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[kswitch] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    // a combined key share in the place of the secret key: checked against the CryptoContext file alone, before the device
    const bool is_share = looks_like_keyshare(privkey_path);
    std::vector<uint32_t> parties;
    KeyShare ks;
    if (is_share != have_parties) {
        std::cerr << "[kswitch] ERROR: " << (is_share ? "a key share needs --parties" : "--parties needs a combined key share, not a secret key")
                  << std::endl;
        return usage();
    }
    const uint32_t N_cc = 1u << cc.p.log_n;
    if (is_share) {
        if (!parse_parties(parties_arg, parties)) {
            std::cerr << "[kswitch] ERROR: --parties needs distinct party indices in [1, " << MKCKKS_MAX_PARTIES << "], comma separated"
                      << std::endl;
            return usage();
        }
        try {
            const uint32_t L = (uint32_t)cc.moduli.size();
            ks = decode_keyshare_checked(read_keyshare_file(privkey_path, N_cc, L), N_cc, cc.moduli);
        } catch (const std::exception &e) {
            std::cerr << "[kswitch] ERROR: " << privkey_path << ": " << e.what() << std::endl;
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
            std::cerr << "[kswitch] ERROR: " << why << std::endl;
            return usage();
        }
    }
    // the other files, as far as they can be judged without the device
    if (!is_share && !FilePtr(std::fopen(privkey_path.c_str(), "rb"))) {
        std::cerr << "[kswitch] ERROR: Failed to load private key from " << privkey_path << std::endl;
        return 1;
    }
    if (!looks_like_public_key(pubkey_path, N_cc)) {
        std::cerr << "[kswitch] ERROR: Failed to load public key from " << pubkey_path << std::endl;
        return 1;
    }
    Json doc;
    bool binary = false;  // the output keeps the input's envelope form
    try {
        doc = read_envelope(input_encfile, &binary);
    } catch (const std::exception &) {
        std::cerr << "[kswitch] ERROR: Could not open input file: " << input_encfile << std::endl;
        return 1;
    }
    std::vector<Ciphertext> cts;
    try {
        const std::vector<CtRef> refs = enumerate_cts(doc);
        cts.reserve(refs.size());
        for (const CtRef &r : refs) cts.push_back(decode_ct(ct_string(doc, r), N_cc));  // validated once the context exists
        for (const Ciphertext &c : cts)
            if (c.nl != cts[0].nl) throw std::runtime_error("ciphertexts of one file must share a level");
    } catch (const std::exception &e) {
        std::cerr << "[kswitch] ERROR: " << e.what() << std::endl;
        return 1;
    }
    if (have_limbs && !cts.empty() && limbs > cts[0].nl) {
        std::cerr << "[kswitch] ERROR: --limbs " << limbs << " exceeds the aggregate's " << cts[0].nl << " limb(s)" << std::endl;
        return 1;
    }
    // fewer limbs than the aggregate has: the share is made at the m + 1-limb prefix and the fusion rescales to m
    const bool rescale = have_limbs && !cts.empty() && limbs < cts[0].nl;
    if (rescale)
        for (const Ciphertext &c : cts)
            if (c.noise_deg != 2) {
                std::cerr << "[kswitch] ERROR: --limbs " << limbs << " needs input at noiseScaleDeg 2 (it has noiseScaleDeg " << c.noise_deg
                          << ")" << std::endl;
                return 1;
            }
    try {
        Session s(cc);
        std::cout << "[kswitch] CryptoContext loaded\n";
        const uint32_t N = s.N();
        std::vector<uint64_t> sk, pk;
        std::vector<int8_t> sk_t;
        uint64_t *d_sk = nullptr;
        if (is_share) {  // lambda * sigma_j over the L limbs of Q: all that mkckks_switch_share_batch reads of a key
            const uint32_t L = s.L();
            std::vector<uint64_t> lambda(parties.size() * L);
            Session::check(mkckks_lagrange_at_zero(s.ctx(), parties.data(), (uint32_t)parties.size(), lambda.data()));
            size_t a = 0;
            while (parties[a] != ks.to_party) ++a;
            d_sk = s.to_device(ks.data.data(), ks.data.size());
            Session::check(mkckks_combine_key_shares(s.ctx(), d_sk, &lambda[a * L], d_sk, 1, L));
            std::cout << "[kswitch] Key share of party " << ks.to_party << " loaded (" << ks.threshold << "-of-" << ks.n_parties << ", "
                      << parties.size() << " parties this round)\n";
        } else {
            if (!load_secret_key(s, privkey_path, sk, sk_t)) {
                std::cerr << "[kswitch] ERROR: Failed to load private key from " << privkey_path << std::endl;
                return 1;
            }
            std::cout << "[kswitch] Private key loaded\n";
        }
        if (!load_public_key(s, pubkey_path, pk)) {
            std::cerr << "[kswitch] ERROR: Failed to load public key from " << pubkey_path << std::endl;
            return 1;
        }
        std::cout << "[kswitch] Recipient's public key loaded\n";
        raw_blobs() = binary;
        for (const Ciphertext &c : cts) validate_ct(c, s);
        std::cout << "[kswitch] Encrypted weights loaded\n";
        std::vector<std::string> blobs(cts.size());
        uint32_t nl = 0;
        if (!cts.empty()) {
            const uint32_t nl_in = cts[0].nl;
            nl = rescale ? limbs + 1 : nl_in;
            const size_t words = (size_t)2 * nl_in * N, B = cts.size(), swords = (size_t)2 * nl * N;
            std::vector<uint64_t> flat(B * words, 0);
            SeedList seeds;
            seeds.resize(B);
            for (size_t i = 0; i < B; ++i) {
                put_payload(&flat[i * words], cts[i]);
                seeds.set(i, cts[i]);
            }
            uint64_t *d_ct = s.to_device(flat.data(), flat.size()), *d_share = s.alloc<uint64_t>(B * swords);
            seeds.expand(s, d_ct, nl_in, 0, B);
            int8_t *d_v = s.alloc<int8_t>(B * (size_t)N);
            int64_t *d_e0 = s.alloc<int64_t>(B * (size_t)N), *d_e1 = s.alloc<int64_t>(B * (size_t)N);
            int32_t *d_e1n = s.alloc<int32_t>(B * (size_t)N);
            const SamplerKey k_v = fresh_key(), k_e0 = fresh_key(), k_e1 = fresh_key();  // this run's mask only
            const double sigma = std::ldexp(1.0, (int)bits);
            for (size_t t = 0; t < B; ++t) {
                Session::check(mkckks_sample_ternary(s.ctx(), d_v + t * N, N, k_v.bytes, (uint32_t)t));
                Session::check(mkckks_sample_gauss_wide(s.ctx(), d_e0 + t * N, N, sigma, k_e0.bytes, (uint32_t)t));
                Session::check(mkckks_sample_gauss(s.ctx(), d_e1n + t * N, N, 3.19, k_e1.bytes, (uint32_t)t));
            }
            {  // e1 at the scheme's sigma is below the wide sampler's range [2^6, 2^56]: the narrow sampler, widened here
                std::vector<int32_t> e1n(B * (size_t)N);
                s.to_host(e1n.data(), d_e1n, e1n.size());
                std::vector<int64_t> e1(e1n.begin(), e1n.end());
                Session::check(mkckks_upload(s.ctx(), d_e1, e1.data(), e1.size() * sizeof(int64_t)));
            }
            if (!is_share) d_sk = s.to_device(sk.data(), sk.size());
            const uint64_t *d_pk = s.to_device(pk.data(), pk.size());
            Session::check(mkckks_switch_share_batch(s.ctx(), d_ct, d_sk, d_pk, d_v, d_e0, d_e1, d_share, (uint32_t)B, nl_in, nl,
                                                     lead ? 1 : 0));
            std::vector<uint64_t> out(B * swords);
            s.to_host(out.data(), d_share, out.size());
            for (size_t i = 0; i < B; ++i) {
                SwitchShare sh;
                sh.ct.nl = nl; sh.ct.level = s.L() - nl; sh.ct.noise_deg = cts[i].noise_deg; sh.ct.slots = cts[i].slots;
                sh.ct.scale = cts[i].scale;
                sh.lead = lead;
                sh.rescale = rescale;
                sh.ct.data.assign(out.begin() + i * swords, out.begin() + (i + 1) * swords);
                blobs[i] = encode_switch_share(sh, N);
            }
        }
        size_t c = 0;
        for_each_ct_field(doc, [&](Json &field) { field = Json(std::move(blobs.at(c++))); });  // the order of enumerate_cts
        std::cout << "[kswitch] " << cts.size() << " " << (lead ? "lead " : "") << "share(s) at " << nl << " limb(s)"
                  << (rescale ? ", to be rescaled to " + std::to_string(limbs) + " at the fusion" : std::string()) << ", smudged at sigma 2^"
                  << bits << "\n";
        try {
            write_envelope(doc, share_out, binary);
        } catch (const std::exception &) {
            std::cerr << "[kswitch] ERROR: Failed to open output file: " << share_out << std::endl;
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << "[kswitch] ERROR: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "[kswitch] Key-switch share completed successfully. Output: " << share_out << std::endl;
    return 0;
}
