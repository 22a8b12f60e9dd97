// fuseSwitchShares -- the closing step of a collective key switch: `fuseSwitchShares <cc_path> <share_1> ... <share_n> <output_file>`.
// mkckks_eval_sum_batch over the parties' key-switch shares (switchShare; switchshare.hpp): the sum is an ordinary
// ciphertext under the RECIPIENT's key, written as a kind-1 envelope (JSON or MKWS, like the first share file) that
// `decryptModelWeights <cc> <recipient_sk>` opens unchanged; level, scale and noiseScaleDeg are the aggregate's.  Shares
// made with `switchShare --limbs m` below the aggregate's limbs carry the rescale flag: they were made at m + 1 limbs and the
// sum is closed with mkckks_compress_batch (Rescale to m limbs: scale / q_m, noiseScaleDeg 1), the order of the compact
// downlink -- the smudging is divided with the message, not before it was added.  It needs no key and learns nothing: what it sums is masked.
// Nothing in a share file is trusted.  The program refuses (exit 1, nothing written) unless every blob position has
// exactly one lead share, the files agree in layers, shapes, limbs, levels and scales, and every word is below its
// modulus (mkckks_count_noncanonical: the sum adds canonical residues lazily).  What it cannot see: whether the n files
// are shares of the SAME aggregate by the parties of ONE key chain (or one --parties set) for ONE recipient -- anything
// else fuses to noise, not to an error, and exits 0.
#include "switchshare.hpp"
using namespace mkh;

int main(int argc, char *argv[]) {
    if (argc < 4) {
        std::cerr << "Usage: " << argv[0] << " <cc_path> <share_1> [<share_2> ...] <output_file>" << std::endl;
        return 1;
    }
    const std::string cc_path = argv[1], output_file = argv[argc - 1];
    const size_t n = (size_t)argc - 3;
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[fuse] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    try {
        // the share files, checked against the CryptoContext file alone (ring dimension and the number of moduli of Q)
        const uint32_t N = 1u << cc.p.log_n, L = (uint32_t)cc.moduli.size();
        std::vector<Json> docs(n);
        std::vector<std::vector<SwitchShare>> shares(n);
        bool binary = false;
        for (size_t p = 0; p < n; ++p) {
            const std::string path = argv[2 + p];
            try {
                docs[p] = read_envelope(path, p == 0 ? &binary : nullptr);
            } catch (const std::exception &) {
                std::cerr << "[fuse] ERROR: Could not open share file: " << path << std::endl;
                return 1;
            }
            try {
                for (const CtRef &r : enumerate_cts(docs[p]))
                    shares[p].push_back(decode_switch_share_checked(ct_string(docs[p], r), N, L));
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
                const Ciphertext &x = shares[0][0].ct, &y = shares[p][i].ct;  // one level and one scale per file
                if (x.nl != y.nl || x.level != y.level || x.noise_deg != y.noise_deg || x.scale != y.scale || x.slots != y.slots ||
                    shares[0][0].rescale != shares[p][i].rescale)
                    return false;
            }
            return true;
        };
        for (size_t p = 0; p < n; ++p)
            if (!same_layout(p)) {
                std::cerr << "[fuse] ERROR: " << argv[2 + p] << ": shares differ in layers, shapes, limbs, levels or scales" << std::endl;
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
        raw_blobs() = binary;
        std::vector<std::string> blobs(B);
        if (B) {
            Session s(cc);
            std::cout << "[fuse] CryptoContext loaded\n";
            const uint32_t nl = shares[0][0].ct.nl;
            size_t words = (size_t)2 * nl * N;
            std::vector<uint64_t> flat(n * B * words);
            for (size_t p = 0; p < n; ++p)
                for (size_t i = 0; i < B; ++i) {
                    std::memcpy(&flat[(p * B + i) * words], shares[p][i].ct.data.data(), words * 8);
                    std::vector<uint64_t>().swap(shares[p][i].ct.data);
                }
            uint64_t *d_in = s.to_device(flat.data(), flat.size()), *d_out = s.alloc<uint64_t>(B * words);
            uint64_t bad = 0;
            Session::check(mkckks_count_noncanonical(s.ctx(), d_in, (uint32_t)(n * B), nl, &bad));
            if (bad) {
                std::cerr << "[fuse] ERROR: " << bad << " residue(s) not below their modulus" << std::endl;
                return 1;
            }
            Session::check(mkckks_eval_sum_batch(s.ctx(), d_in, d_out, (uint32_t)n, (uint32_t)B, nl));
            const bool rescale = shares[0][0].rescale;  // switchShare --limbs nl - 1: the header of Rescale(., nl)
            const uint32_t out_nl = rescale ? nl - 1 : nl;
            if (rescale) {
                uint64_t *d_small = s.alloc<uint64_t>(B * (size_t)2 * out_nl * N);
                Session::check(mkckks_compress_batch(s.ctx(), d_out, d_small, (uint32_t)B, nl, out_nl));
                d_out = d_small;
                words = (size_t)2 * out_nl * N;
                std::cout << "[fuse] rescaled from " << nl << " to " << out_nl << " limb(s)\n";
            }
            std::vector<uint64_t> out(B * words);
            s.to_host(out.data(), d_out, out.size());
            for (size_t i = 0; i < B; ++i) {
                Ciphertext ct = shares[0][i].ct;  // header fields; the payload was released above
                ct.seeded = false;
                if (rescale) {
                    ct.level += 1;
                    ct.scale = ct.scale / (double)s.moduli()[out_nl];
                    ct.nl = out_nl;
                    ct.noise_deg = 1;
                }
                ct.data.assign(out.begin() + i * words, out.begin() + (i + 1) * words);
                blobs[i] = encode_ct(ct, N);
            }
        }
        Json doc = docs[0];
        size_t c = 0;
        for_each_ct_field(doc, [&](Json &field) { field = Json(std::move(blobs.at(c++))); });  // the order of enumerate_cts
        try {
            write_envelope(doc, output_file, binary);
        } catch (const std::exception &) {
            std::cerr << "[fuse] ERROR: Failed to open output file: " << output_file << std::endl;
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << "[fuse] ERROR: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "[fuse] Key-switch fusion completed successfully. Output: " << output_file << std::endl;
    return 0;
}
