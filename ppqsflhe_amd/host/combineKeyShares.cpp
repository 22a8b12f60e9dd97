// combineKeyShares -- the receiving side of a key sharing: `combineKeyShares <cc_path> <out> <share_1> ... <share_n>`.
// Party j sums the n key shares f_i(j) it received, its own among them (shareKey's <prefix>.<j> of every dealer i), into
// its combined share sigma_j = sum_i f_i(j): one mkckks_combine_key_shares with all weights 1.  The output is a key-share
// file with from_party = 0, which partialDecrypt --parties takes in the place of a secret key; it is a SECRET like its
// inputs.  Nothing in a share file is trusted (keyshare.hpp): the program refuses, before it touches the device, unless
// all shares carry the same (n_parties, threshold, to_party), there are exactly n of them and their from_party values
// are 1 .. n, each once.  What it cannot see: whether the dealers' files belong to one key epoch.
#include "keyshare.hpp"
using namespace mkh;

int main(int argc, char *argv[]) {
    if (argc < 4) {
        std::cerr << "Usage: " << argv[0] << " <cc_path> <out> <share_1> [<share_2> ...]" << std::endl;
        return 1;
    }
    const std::string cc_path = argv[1], out_path = argv[2];
    const size_t m = (size_t)argc - 3;
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[combine] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    try {
        // the share files, checked against the CryptoContext file alone (ring dimension and the moduli of Q it lists)
        const uint32_t N = 1u << cc.p.log_n, L = (uint32_t)cc.moduli.size();
        if (m > MKCKKS_MAX_PARTIES) throw std::runtime_error("more share files than MKCKKS_MAX_PARTIES");
        std::vector<KeyShare> shares;
        for (size_t p = 0; p < m; ++p) {
            const std::string path = argv[3 + p];
            try {
                shares.push_back(decode_keyshare_checked(read_keyshare_file(path, N, L), N, cc.moduli));
            } catch (const std::exception &e) {
                std::cerr << "[combine] ERROR: " << path << ": " << e.what() << std::endl;
                return 1;
            }
        }
        const KeyShare &first = shares[0];
        unsigned long long seen = 0;
        for (size_t p = 0; p < m; ++p) {
            const KeyShare &ks = shares[p];
            if (ks.n_parties != first.n_parties || ks.threshold != first.threshold || ks.to_party != first.to_party)
                throw std::runtime_error(std::string(argv[3 + p]) + ": shares differ in n_parties, threshold or to_party");
            if (ks.from_party == 0) throw std::runtime_error(std::string(argv[3 + p]) + ": already a combined share");
            if (seen >> (ks.from_party - 1) & 1)
                throw std::runtime_error(std::string(argv[3 + p]) + ": two shares of dealer " + std::to_string(ks.from_party));
            seen |= 1ull << (ks.from_party - 1);
        }
        if (m != first.n_parties)
            throw std::runtime_error("need the shares of all " + std::to_string(first.n_parties) + " dealers, got " + std::to_string(m));
        std::cout << "[combine] " << m << " key share(s) for party " << first.to_party << " loaded\n";
        Session s(cc);
        std::cout << "[combine] CryptoContext loaded\n";
        const size_t words = (size_t)L * N;
        std::vector<uint64_t> flat(m * words);
        for (size_t p = 0; p < m; ++p) std::memcpy(&flat[p * words], shares[p].data.data(), words * 8);
        uint64_t *d_in = s.to_device(flat.data(), flat.size());
        const std::vector<uint64_t> ones(m * L, 1);
        Session::check(mkckks_combine_key_shares(s.ctx(), d_in, ones.data(), d_in, (uint32_t)m, L));  // into in[0]
        KeyShare sum;
        sum.n_parties = first.n_parties; sum.threshold = first.threshold; sum.from_party = 0; sum.to_party = first.to_party;
        sum.data.resize(words);
        s.to_host(sum.data.data(), d_in, words);
        try {
            write_keyshare_file(out_path, sum, N, L);
        } catch (const std::exception &) {
            std::cerr << "[combine] ERROR: Failed to open output file: " << out_path << std::endl;
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << "[combine] ERROR: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "[combine] Key shares combined successfully. Output: " << out_path << std::endl;
    return 0;
}
