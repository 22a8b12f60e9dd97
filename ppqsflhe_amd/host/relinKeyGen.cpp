// relinKeyGen -- the key a server needs to multiply two ciphertexts under ONE key:
// `relinKeyGen <cc.json> <privkey> <pubkey> <relinkey_out>`.
// cc->EvalMultKeyGen(sk) is an upstream call the reference never makes (everything its mains compute is linear in the
// encrypted values).  The relinearisation key is the re-encryption key from s^2 to s (mkckks_relin_keygen), with fresh
// randomness as in REkeyGen / rotKeyGen.  Run by the OWNER of the key the ciphertexts are under (for a server's products:
// the owner of the common-domain key); <pubkey> is that same party's public key.  A key for a JOINT key (threshold
// decryption) needs a collective protocol and is not generated here.  The file is the eval-key container under the kind
// of product.hpp; it holds no secret.
#include "hostlib.hpp"
#include "product.hpp"
using namespace mkh;

int main(int argc, char *argv[]) {
    if (argc != 5) {
        std::cerr << "Usage: " << argv[0] << " <cc.json> <privkey> <pubkey> <relinkey_out>" << std::endl;
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
