// shareKey -- the dealer's step of t-of-n threshold decryption, once per key epoch:
// `shareKey <cc_path> <privkey_path> <n_parties> <threshold> <party_index> <out_prefix>`.
// Party <party_index> Shamir-shares its own secret key (keyGen / keyGen --join) among the n parties with threshold t:
// one mkckks_share_key over the L limbs of Q under a fresh OS-drawn key that keys nothing else, and one key-share file
// <out_prefix>.<j> (keyshare.hpp) for every party j = 1 .. n, its own included.  The files are SECRETS: <out_prefix>.<j>
// goes to party j alone, over a private, authenticated channel, which this project does not provide.  The coefficient
// polynomials of the sharing exist on the device only, inside the kernel.  combineKeyShares follows on the receiving side.
#include "keyshare.hpp"
using namespace mkh;

static bool parse_index(const char *v, uint32_t &out) {
    const std::string s = v;
    if (s.empty() || s.size() > 2 || s.find_first_not_of("0123456789") != std::string::npos) return false;
    out = (uint32_t)std::atoi(v);
    return true;
}

int main(int argc, char *argv[]) {
    auto usage = [&] {
        std::cerr << "Usage: " << argv[0] << " <cc_path> <privkey_path> <n_parties> <threshold> <party_index> <out_prefix>" << std::endl;
        return 1;
    };
    if (argc != 7) return usage();
    const std::string cc_path = argv[1], privkey_path = argv[2], out_prefix = argv[6];
    uint32_t n = 0, t = 0, me = 0;
    if (!parse_index(argv[3], n) || !parse_index(argv[4], t) || !parse_index(argv[5], me)) return usage();
    if (t < 1 || t > n || n > MKCKKS_MAX_PARTIES || me < 1 || me > n) {
        std::cerr << "[shareKey] ERROR: need 1 <= threshold <= n_parties <= " << MKCKKS_MAX_PARTIES << " and 1 <= party_index <= n_parties"
                  << std::endl;
        return 1;
    }
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[shareKey] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    try {
        Session s(cc);
        std::cout << "[shareKey] CryptoContext loaded\n";
        const uint32_t N = s.N(), L = s.L();
        std::vector<uint64_t> sk;
        std::vector<int8_t> sk_t;
        if (!load_secret_key(s, privkey_path, sk, sk_t)) {
            std::cerr << "[shareKey] ERROR: Failed to load private key from " << privkey_path << std::endl;
            return 1;
        }
        std::cout << "[shareKey] Private key loaded\n";
        const size_t words = (size_t)L * N;
        uint64_t *d_shares = s.alloc<uint64_t>(n * words);
        const SamplerKey key = fresh_key();  // this sharing only
        Session::check(mkckks_share_key(s.ctx(), s.to_device(sk.data(), sk.size()), d_shares, L, n, t, key.bytes, 0));
        std::vector<uint64_t> out(n * words);
        s.to_host(out.data(), d_shares, out.size());
        for (uint32_t j = 1; j <= n; ++j) {
            KeyShare ks;
            ks.n_parties = n; ks.threshold = t; ks.from_party = me; ks.to_party = j;
            ks.data.assign(out.begin() + (j - 1) * words, out.begin() + j * words);
            const std::string path = out_prefix + "." + std::to_string(j);
            try {
                write_keyshare_file(path, ks, N, L);
            } catch (const std::exception &) {
                std::cerr << "[shareKey] ERROR: Failed to open output file: " << path << std::endl;
                return 1;
            }
        }
        std::cout << "[shareKey] " << n << " key share(s) of party " << me << ", threshold " << t << "\n";
    } catch (const std::exception &e) {
        std::cerr << "[shareKey] ERROR: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "[shareKey] Key sharing completed successfully. Output: " << out_prefix << ".1 .. ." << n << std::endl;
    return 0;
}
