// aggregateEncryptedWeights -- drop-in for server/src/aggregateEncryptedWeights.cpp:
// `aggregateEncryptedWeights <cc_path> <client2_encfile> <client1to2_encfile> <output_aggfile>` (:33-43; caller
// server_fns.sh:72).  For every (w2, w1) pair with equal "layer" and "shape" (:68-72): EvalAdd then EvalMult(.,0.5)
// on mean, std_dev and the first min(|v1|,|v2|) value ciphertexts (:80-109).
// n-client generalisation: any number of further encfiles may follow the output path; every
// matching ciphertext is summed with one mkckks_eval_sum_batch and scaled by 1/n_files.  (serverRound does the
// re-encryptions and this aggregation in one program.)  Seeded inputs (encryptModelWeights --seeded) are accepted per
// blob: c1 is rebuilt on the device before the sum.
// --weights w_1,...,w_n (anywhere after <cc_path>): the weighted mean sum_c w_c x_c / sum_c w_c in place of the plain
// one, one non-negative number per input file in argument order (sample counts as they are).  One
// mkckks_eval_wsum_batch (EvalMult(ct, w_c) per file + the EvalAdd chain) and one rescale; the same bytes as serverRound
// --weights with every client marked "-".
// --slot-weights <file> (anywhere after <cc_path>): every coordinate of the aggregate scaled by a factor of its own, read
// from a plaintext weights_summary JSON in the schema encryptModelWeights reads (slotweights.hpp) -- the divisor
// 1 / count_j of a round whose clients cover different coordinates, a per-layer rate, a 0/1 mask.  The file holds the
// whole factor (nothing multiplies by 1/n as well): one mkckks_eval_sum_batch, then EvalMult(ct, plaintext) with one
// rescale last (mkckks_mult_plain_rescale_batch); the same bytes as serverRound --slot-weights with every client marked
// "-".  Not together with --weights (that needs a second rescale and a second level).
#include "hostlib.hpp"
using namespace mkh;

int main(int argc, char *argv[]) {
    std::string weights_text;
    bool have_weights = false;
    std::vector<char *> av(argv, argv + argc);
    for (size_t i = 1; i < av.size(); ++i)
        if (std::string(av[i]) == "--weights") {
            if (i + 1 >= av.size()) {
                std::cerr << "[agg] ERROR: --weights needs a value" << std::endl;
                return 1;
            }
            have_weights = true;
            weights_text = av[i + 1];
            av.erase(av.begin() + i, av.begin() + i + 2);
            break;
        }
    SlotWeights sw;
    for (size_t i = 1; i < av.size(); ++i)
        if (std::string(av[i]) == "--slot-weights") {
            if (i + 1 >= av.size() || !*av[i + 1]) {
                std::cerr << "[agg] ERROR: --slot-weights needs a file" << std::endl;
                return 1;
            }
            if (have_weights) {
                std::cerr << "[agg] ERROR: --slot-weights cannot be combined with --weights" << std::endl;
                return 1;
            }
            sw.path = av[i + 1];
            av.erase(av.begin() + i, av.begin() + i + 2);
            break;
        }
    if (sw.on()) {
        const std::string err = load_slot_weights(sw.path, sw.file);
        if (!err.empty()) {
            std::cerr << "[agg] ERROR: " << err << std::endl;
            return 1;
        }
    }
    argc = (int)av.size();
    argv = av.data();
    if (argc < 5) {
        std::cerr << "Usage: " << argv[0] << " <cc_path> <client2_encfile> <client1to2_encfile> <output_aggfile>" << std::endl;
        return 1;
    }
    const std::string cc_path = argv[1], output_file = argv[4];
    std::vector<std::string> in_paths{argv[2], argv[3]};
    for (int i = 5; i < argc; ++i) in_paths.push_back(argv[i]);
    RoundWeights rw;
    if (have_weights) {
        const std::string err = parse_weights(weights_text, in_paths.size(), rw.w);
        if (!err.empty()) {
            std::cerr << "[agg] ERROR: " << err << std::endl;
            return 1;
        }
    }
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[agg] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    try {
        Session s(cc);
        std::cout << "[agg] CryptoContext loaded\n";
        const uint32_t N = s.N();
        std::vector<Json> files;
        bool binary = false;  // the output keeps the first input's envelope form
        for (const std::string &p : in_paths) {
            bool b = false;
            files.push_back(read_envelope(p, &b));
            if (files.size() == 1) binary = b;
        }
        raw_blobs() = binary;
        const size_t n_files = files.size();

        // one output entry per matching (layer, shape) tuple (aggregateEncryptedWeights.cpp:68-72,115)
        Json outputJson;
        const std::vector<AggItem> items = build_agg_items(files, outputJson);
        if (!items.empty()) {
            std::vector<uint64_t> flat;  // [client][ct][2][nl][N]
            SeedList seeds;
            const Ciphertext first = gather_agg_inputs(items, n_files, s, flat, seeds);
            const size_t B = items.size(), words = (size_t)2 * first.nl * N;
            uint64_t *d_in = s.to_device(flat.data(), flat.size());
            seeds.expand(s, d_in, first.nl, 0, n_files * B);
            uint64_t *d_sum = s.alloc<uint64_t>(B * words);
            const uint64_t *d_slot_pt = nullptr;
            if (sw.on()) {
                std::vector<double> vals;
                std::string err = slot_weights_headroom_error(s, first, sw);
                if (err.empty()) err = slot_weight_values(s, items, outputJson, sw, vals);
                if (!err.empty()) {
                    std::cerr << "[agg] ERROR: " << err << std::endl;
                    return 1;
                }
                uint64_t *d_pt = s.alloc<uint64_t>(B * (size_t)first.nl * N);
                encode_slot_weights(s, vals, B, first, d_pt);
                d_slot_pt = d_pt;
            }
            if (rw.on()) {
                const std::string err = weights_headroom_error(s, first);
                if (!err.empty()) {
                    std::cerr << "[agg] ERROR: " << err << std::endl;
                    return 1;
                }
                Session::check(mkckks_eval_wsum_batch(s.ctx(), d_in, d_sum, (uint32_t)n_files, (uint32_t)B, first.nl, rw.w.data(),
                                                      weights_sf_level(first), 0));
            } else {
                Session::check(mkckks_eval_sum_batch(s.ctx(), d_in, d_sum, (uint32_t)n_files, (uint32_t)B, first.nl));
            }
            finish_aggregate(s, items, d_sum, first, n_files, outputJson, rw.on(), d_slot_pt);
        }
        write_envelope(outputJson, output_file, binary);
    } catch (const std::exception &e) {
        std::cerr << "[agg] ERROR: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "[agg] Aggregation completed successfully. Output: " << output_file << std::endl;
    return 0;
}
