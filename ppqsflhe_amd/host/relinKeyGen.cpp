// relinKeyGen -- the key a server needs to multiply two ciphertexts under ONE key:
// `relinKeyGen <cc.json> <privkey> <pubkey> <relinkey_out>`.
// cc->EvalMultKeyGen(sk) is an upstream call the reference never makes (everything its mains compute is linear in the
// encrypted values).  The relinearisation key is the re-encryption key from s^2 to s (mkckks_relin_keygen), with fresh
// randomness as in REkeyGen / rotKeyGen.  Run by the OWNER of the key the ciphertexts are under (for a server's products:
// the owner of the common-domain key); <pubkey> is that same party's public key.  The file is the eval-key container
// under the kind of product.hpp; it holds no secret.
// A key for a JOINT key (keyGen --join: nobody holds s) is made collectively, in two rounds (include/mkckks.h:
// "collective evaluation keys").  Round 1 is REkeyGen <cc> <own privkey> <joint pubkey> of every party, summed by
// fuseEvalKeys into the round-1 key.  Round 2 is `relinKeyGen <cc.json> <privkey> <key1> <share_out> --share` of every
// party (mkckks_relin_share with fresh errors): a relinearisation-key share (kind 12, evalkeys.hpp), which cipherProduct
// refuses; fuseEvalKeys sums the n shares into the relinearisation key.
#include "hostlib.hpp"
#include "evalkeys.hpp"
using namespace mkh;

static int share_main(const std::string &cc_path, const std::string &sk_path, const std::string &key1_path,
                      const std::string &out_path) {
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[relinkeygen] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    {   // the round-1 key by kind, before a device is opened
        std::unique_ptr<FILE, FileCloser> f(std::fopen(key1_path.c_str(), "rb"));
        BlobHeader h{};
        if (!f || std::fread(&h, sizeof h, 1, f.get()) != 1 || std::memcmp(h.magic, "MKCK", 4) || h.version != 1) {
            std::cerr << "[relinkeygen] ERROR: Failed to load the round-1 key from " << key1_path << std::endl;
            return 1;
        }
        if (h.kind != KIND_RK) {
            std::cerr << "[relinkeygen] ERROR: " << key1_path << " is " << key_kind_name(h.kind)
                      << ", not the round-1 key (a re-encryption key: fuseEvalKeys of the parties' REkeyGen outputs)" << std::endl;
            return 1;
        }
    }
    try {
        Session s(cc);
        const uint32_t N = s.N(), D = s.D(), beta = s.beta();
        std::vector<uint64_t> sk, key1;
        std::vector<int8_t> sk_t;
        if (!load_secret_key(s, sk_path, sk, sk_t)) {
            std::cerr << "[relinkeygen] ERROR: Failed to load private key from " << sk_path << std::endl;
            return 1;
        }
        if (!read_key_file(key1_path, KIND_RK, N, D, 2 * beta, key1)) {
            std::cerr << "[relinkeygen] ERROR: the round-1 key " << key1_path << " does not match the CryptoContext" << std::endl;
            return 1;
        }
        const SamplerKey k_e0 = fresh_key(), k_e1 = fresh_key();  // fresh errors for every share
        int32_t *d_e0 = s.alloc<int32_t>((size_t)beta * N), *d_e1 = s.alloc<int32_t>((size_t)beta * N);
        Session::check(mkckks_sample_gauss(s.ctx(), d_e0, (size_t)beta * N, 3.19, k_e0.bytes, 1));
        Session::check(mkckks_sample_gauss(s.ctx(), d_e1, (size_t)beta * N, 3.19, k_e1.bytes, 2));
        uint64_t *d_key = s.to_device(key1.data(), key1.size());
        Session::check(mkckks_relin_share(s.ctx(), d_key, s.to_device(sk.data(), sk.size()), d_e0, d_e1, d_key));
        s.to_host(key1.data(), d_key, key1.size());
        try {
            write_key_file(out_path, KIND_RELIN_SHARE, N, D, 2 * beta, key1);
        } catch (const std::exception &) {
            std::cerr << "[relinkeygen] ERROR: Failed to save the relinearisation-key share to " << out_path << std::endl;
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << "[relinkeygen] ERROR: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "[relinkeygen] Relinearisation-key share saved to " << out_path << std::endl;
    return 0;
}

int main(int argc, char *argv[]) {
    if (argc == 6 && std::string(argv[5]) == "--share") return share_main(argv[1], argv[2], argv[3], argv[4]);
    if (argc != 5) {
        std::cerr << "Usage: " << argv[0] << " <cc.json> <privkey> <pubkey> <relinkey_out>" << std::endl;
        std::cerr << "       " << argv[0] << " <cc.json> <privkey> <key1> <share_out> --share" << std::endl;
        return 1;
    }
    const std::string cc_path = argv[1], sk_path = argv[2], pk_path = argv[3], out_path = argv[4];
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[relinkeygen] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    try {
        Session s(cc);
        const uint32_t N = s.N(), D = s.D(), beta = s.beta();
        std::vector<uint64_t> sk, pk;
        std::vector<int8_t> sk_t;
        if (!load_secret_key(s, sk_path, sk, sk_t)) {
            std::cerr << "[relinkeygen] ERROR: Failed to load private key from " << sk_path << std::endl;
            return 1;
        }
        if (!load_public_key(s, pk_path, pk)) {
            std::cerr << "[relinkeygen] ERROR: Failed to load public key from " << pk_path << std::endl;
            return 1;
        }
        const SamplerKey k_u = fresh_key(), k_e0 = fresh_key(), k_e1 = fresh_key();
        int8_t *d_u = s.alloc<int8_t>((size_t)beta * N);
        int32_t *d_e0 = s.alloc<int32_t>((size_t)beta * N), *d_e1 = s.alloc<int32_t>((size_t)beta * N);
        Session::check(mkckks_sample_ternary(s.ctx(), d_u, (size_t)beta * N, k_u.bytes, 0));
        Session::check(mkckks_sample_gauss(s.ctx(), d_e0, (size_t)beta * N, 3.19, k_e0.bytes, 1));
        Session::check(mkckks_sample_gauss(s.ctx(), d_e1, (size_t)beta * N, 3.19, k_e1.bytes, 2));
        const size_t key_words = (size_t)beta * 2 * D * N;
        uint64_t *d_evk = s.alloc<uint64_t>(key_words);
        Session::check(mkckks_relin_keygen(s.ctx(), s.to_device(sk_t.data(), N), s.to_device(pk.data(), pk.size()), d_u, d_e0,
                                           d_e1, d_evk));
        std::vector<uint64_t> evk(key_words);
        s.to_host(evk.data(), d_evk, key_words);
        try {
            write_key_file(out_path, KIND_RELIN_KEY, N, D, 2 * beta, evk);
        } catch (const std::exception &) {
            std::cerr << "[relinkeygen] ERROR: Failed to save the relinearisation key to " << out_path << std::endl;
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << "[relinkeygen] ERROR: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "[relinkeygen] Relinearisation key saved to " << out_path << std::endl;
    return 0;
}
