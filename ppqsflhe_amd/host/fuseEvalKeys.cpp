// fuseEvalKeys -- sums the parties' shares of a joint key's evaluation keys:
// `fuseEvalKeys <cc.json> <out> <share_1> ... <share_n>` (cc->MultiAddEvalKeys / MultiAddEvalAutomorphismKeys /
// MultiAddEvalMultKeys; mkckks_evk_sum on all D limbs).  All inputs are containers of ONE kind (evalkeys.hpp):
//   re-encryption keys (REkeyGen <cc> <own privkey> <joint pubkey>)  -> a re-encryption key: the round-1 key of relinKeyGen --share
//   rotation-key shares (rotKeyGen ... --share)                       -> the rotation-key file slotSum reads (entries matched by g)
//   relinearisation-key shares (relinKeyGen ... --share)              -> the relinearisation key cipherProduct reads
// ALL n parties of the key epoch must be among the inputs: a sum of fewer is accepted here and gives noise later; the
// program cannot tell.  Mixed kinds, differing N / D / beta, differing sets of g and finished keys are refused, by file
// and field, before a device is opened.  Nothing in the files is secret.
#include "evalkeys.hpp"
#include "rotkeys.hpp"
using namespace mkh;

// header, size and (rotation shares) the Galois elements of one input; the refusal text, empty on success
static std::string read_meta(const std::string &path, EvkMeta &m) {
    std::unique_ptr<FILE, FileCloser> f(std::fopen(path.c_str(), "rb"));
    BlobHeader h{};
    if (!f || std::fread(&h, sizeof h, 1, f.get()) != 1 || std::memcmp(h.magic, "MKCK", 4) || h.version != 1)
        return "Failed to load a key share from " + path;
    m.kind = h.kind; m.ring_dim = h.ring_dim; m.limbs = h.limbs; m.parts = h.parts; m.entries = h.slots;
    const std::string kerr = fuse_kind_error(path, m.kind);
    if (!kerr.empty()) return kerr;
    if (!m.ring_dim || (m.ring_dim & (m.ring_dim - 1)) || m.ring_dim > (1u << 17) || !m.limbs || m.limbs > 64 || !m.parts ||
        (m.parts & 1) || m.parts > 128)
        return path + ": header fields out of range";
    if (is_rot_kind(m.kind) && m.entries > 64) return path + ": claims " + std::to_string(m.entries) + " entries (at most 64)";
    if (std::fseek(f.get(), 0, SEEK_END) != 0) return path + ": not seekable";
    const long size = std::ftell(f.get());
    if (size < 0 || (uint64_t)size != evk_file_bytes(m)) return path + ": size does not match its header";
    if (is_rot_kind(m.kind)) {
        const uint64_t key_bytes = (uint64_t)m.parts * m.limbs * m.ring_dim * 8;
        for (uint32_t i = 0; i < m.entries; ++i) {
            uint64_t g = 0;
            if (std::fseek(f.get(), (long)(48 + i * (8 + key_bytes)), SEEK_SET) != 0 || std::fread(&g, 8, 1, f.get()) != 1)
                return path + ": is truncated";
            m.elements.push_back(g);
        }
        return elements_error(path, m);
    }
    return "";
}

int main(int argc, char *argv[]) {
    if (argc < 4) {
        std::cerr << "Usage: " << argv[0] << " <cc.json> <out> <share_1> ... <share_n>" << std::endl;
        return 1;
    }
    const std::string cc_path = argv[1], out_path = argv[2];
    std::vector<std::string> paths(argv + 3, argv + argc);
    const uint32_t n = (uint32_t)paths.size();
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[fuseevalkeys] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    if (n > MKCKKS_MAX_PARTIES) {
        std::cerr << "[fuseevalkeys] ERROR: " << n << " shares (at most " << MKCKKS_MAX_PARTIES << " parties)" << std::endl;
        return 1;
    }
    std::vector<EvkMeta> metas(n);
    for (uint32_t p = 0; p < n; ++p) {
        std::string err = read_meta(paths[p], metas[p]);
        if (err.empty() && p) err = fuse_mismatch(paths[0], metas[0], paths[p], metas[p]);
        if (!err.empty()) {
            std::cerr << "[fuseevalkeys] ERROR: " << err << std::endl;
            return 1;
        }
    }
    const EvkMeta &m0 = metas[0];
    const bool rot = is_rot_kind(m0.kind);
    try {
        Session s(cc);
        const uint32_t N = s.N(), D = s.D(), beta = s.beta();
        if (m0.ring_dim != N || m0.limbs != D || m0.parts != 2 * beta) {
            std::cerr << "[fuseevalkeys] ERROR: " << paths[0] << " does not match the CryptoContext" << std::endl;
            return 1;
        }
        const size_t key_words = (size_t)beta * 2 * D * N;
        uint64_t *d_in = s.alloc<uint64_t>((size_t)n * key_words);
        std::vector<uint64_t> sum(key_words);
        auto fuse = [&](const std::vector<const uint64_t *> &parts, std::vector<uint64_t> &out) {
            for (uint32_t p = 0; p < n; ++p) Session::check(mkckks_upload(s.ctx(), d_in + (size_t)p * key_words, parts[p], key_words * 8));
            Session::check(mkckks_evk_sum(s.ctx(), d_in, d_in, n, 1));  // onto the first share
            out.resize(key_words);
            s.to_host(out.data(), d_in, key_words);
        };
        if (rot) {
            std::vector<RotKeys> shares(n);
            for (uint32_t p = 0; p < n; ++p) {
                const std::string err = read_rot_keys(paths[p], N, D, 2 * beta, shares[p], KIND_ROTKEY_SHARE);
                if (!err.empty()) {
                    std::cerr << "[fuseevalkeys] ERROR: " << paths[p] << ": " << err << std::endl;
                    return 1;
                }
            }
            RotKeys fused;
            for (const auto &kv : shares[0].keys) {
                std::vector<const uint64_t *> parts;
                for (uint32_t p = 0; p < n; ++p) parts.push_back(shares[p].keys.at(kv.first).data());
                fuse(parts, fused.keys[kv.first]);
            }
            try {
                write_rot_keys(out_path, fused, N, D, 2 * beta);
            } catch (const std::exception &) {
                std::cerr << "[fuseevalkeys] ERROR: Failed to save the rotation keys to " << out_path << std::endl;
                return 1;
            }
            std::cout << "[fuseevalkeys] " << fused.keys.size() << " rotation key(s) of " << n << " parties saved to " << out_path << std::endl;
        } else {
            std::vector<std::vector<uint64_t>> shares(n);
            std::vector<const uint64_t *> parts;
            for (uint32_t p = 0; p < n; ++p) {
                if (!read_key_file(paths[p], m0.kind, N, D, 2 * beta, shares[p])) {
                    std::cerr << "[fuseevalkeys] ERROR: Failed to load a key share from " << paths[p] << std::endl;
                    return 1;
                }
                parts.push_back(shares[p].data());
            }
            fuse(parts, sum);
            try {
                write_key_file(out_path, fused_kind(m0.kind), N, D, 2 * beta, sum);
            } catch (const std::exception &) {
                std::cerr << "[fuseevalkeys] ERROR: Failed to save the key to " << out_path << std::endl;
                return 1;
            }
            std::cout << "[fuseevalkeys] " << (m0.kind == KIND_RK ? "Round-1 key" : "Relinearisation key") << " of " << n
                      << " parties saved to " << out_path << std::endl;
        }
    } catch (const std::exception &e) {
        std::cerr << "[fuseevalkeys] ERROR: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
