// rotKeyGen -- the keys a server needs to rotate and sum the slots of ciphertexts under ONE key:
// `rotKeyGen <cc.json> <privkey> <pubkey> <rotkeys_out> (--steps r1,r2,... | --sum <span>)`.
// cc->EvalRotateKeyGen(sk, {r...}) / cc->EvalSumKeyGen(sk) are upstream calls the reference never makes (its mains leave
// every slot where the client put it).  For every step r the Galois key of g = 5^r mod 2N is the re-encryption key from
// sigma_g(s) to s (mkckks_galois_keygen); --sum <span> asks for the steps 1, 2, 4, ... below span that slotSum uses.
// Run by the OWNER of the key the ciphertexts are under (for a server's aggregate: the owner of the common-domain key);
// <pubkey> is that same party's public key.  The file holds no secret (rotkeys.hpp).
// Keys for a JOINT key (keyGen --join: nobody holds s) are made collectively: every party runs the same command with
// its OWN private key, the JOINT public key and a trailing `--share`; the file is then a rotation-key share (kind 11,
// evalkeys.hpp), which slotSum refuses, and fuseEvalKeys sums the n parties' shares into the rotation-key file.  The
// flag changes nothing but the container kind.
#include "evalkeys.hpp"
#include "rotkeys.hpp"
using namespace mkh;

int main(int argc, char *argv[]) {
    auto usage = [&] {
        std::cerr << "Usage: " << argv[0] << " <cc.json> <privkey> <pubkey> <rotkeys_out> (--steps r1,r2,... | --sum <span>) [--share]" << std::endl;
        return 1;
    };
    const bool share = argc == 8 && std::string(argv[7]) == "--share";
    if (argc != 7 && !share) return usage();
    const std::string cc_path = argv[1], sk_path = argv[2], pk_path = argv[3], out_path = argv[4], mode = argv[5], arg = argv[6];
    if (mode != "--steps" && mode != "--sum") return usage();
    std::vector<int32_t> steps;
    uint32_t span = 0;
    if (mode == "--steps") {
        size_t pos = 0;
        while (pos <= arg.size()) {
            const size_t comma = std::min(arg.find(',', pos), arg.size());
            int32_t r = 0;
            if (!parse_step(arg.substr(pos, comma - pos), r)) {
                std::cerr << "[rotkeygen] ERROR: --steps needs a comma-separated list of integers" << std::endl;
                return 1;
            }
            steps.push_back(r);
            pos = comma + 1;
        }
    } else {
        int32_t v = 0;
        if (!parse_step(arg, v) || v < 1 || (v & (v - 1))) {
            std::cerr << "[rotkeygen] ERROR: --sum needs a power of two of at least 1" << std::endl;
            return 1;
        }
        span = (uint32_t)v;
    }
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[rotkeygen] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    try {
        Session s(cc);
        const uint32_t N = s.N(), D = s.D(), beta = s.beta();
        if (span > N / 2) {
            std::cerr << "[rotkeygen] ERROR: --sum " << span << " exceeds the " << N / 2 << " slots" << std::endl;
            return 1;
        }
        if (span) steps = sum_steps(span);
        std::vector<uint64_t> sk, pk;
        std::vector<int8_t> sk_t;
        if (!load_secret_key(s, sk_path, sk, sk_t)) {
            std::cerr << "[rotkeygen] ERROR: Failed to load private key from " << sk_path << std::endl;
            return 1;
        }
        if (!load_public_key(s, pk_path, pk)) {
            std::cerr << "[rotkeygen] ERROR: Failed to load public key from " << pk_path << std::endl;
            return 1;
        }
        const int8_t *d_s = s.to_device(sk_t.data(), N);
        const uint64_t *d_pk = s.to_device(pk.data(), pk.size());
        int8_t *d_u = s.alloc<int8_t>((size_t)beta * N);
        int32_t *d_e0 = s.alloc<int32_t>((size_t)beta * N), *d_e1 = s.alloc<int32_t>((size_t)beta * N);
        const size_t key_words = (size_t)beta * 2 * D * N;
        uint64_t *d_evk = s.alloc<uint64_t>(key_words);
        RotKeys rk;
        for (int32_t r : steps) {
            uint32_t g = 0;
            Session::check(mkckks_galois_element(s.ctx(), r, &g));
            if (rk.keys.count(g)) continue;  // steps that agree mod N/2
            const SamplerKey k_u = fresh_key(), k_e0 = fresh_key(), k_e1 = fresh_key();  // fresh randomness per key
            Session::check(mkckks_sample_ternary(s.ctx(), d_u, (size_t)beta * N, k_u.bytes, 0));
            Session::check(mkckks_sample_gauss(s.ctx(), d_e0, (size_t)beta * N, 3.19, k_e0.bytes, 1));
            Session::check(mkckks_sample_gauss(s.ctx(), d_e1, (size_t)beta * N, 3.19, k_e1.bytes, 2));
            Session::check(mkckks_galois_keygen(s.ctx(), d_s, d_pk, d_u, d_e0, d_e1, g, d_evk));
            std::vector<uint64_t> &key = rk.keys[g];
            key.resize(key_words);
            s.to_host(key.data(), d_evk, key_words);
            std::cout << "[rotkeygen] step " << r << ": Galois element " << g << "\n";
        }
        try {
            write_rot_keys(out_path, rk, N, D, 2 * beta, share ? (uint32_t)KIND_ROTKEY_SHARE : (uint32_t)KIND_ROTKEYS);
        } catch (const std::exception &) {
            std::cerr << "[rotkeygen] ERROR: Failed to save rotation keys to " << out_path << std::endl;
            return 1;
        }
        std::cout << "[rotkeygen] " << rk.keys.size() << (share ? " rotation-key share(s) saved to " : " rotation key(s) saved to ")
                  << out_path << std::endl;
    } catch (const std::exception &e) {
        std::cerr << "[rotkeygen] ERROR: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
