// slotSum -- the sum of the slots of every ciphertext of an envelope, optionally after a per-slot product:
// `slotSum <cc_path> <rotkeys> <input_encfile> <output_encfile> [--span <n>] [--slot-weights <factors.json>]`.
// cc->EvalSum(ct, span) and, with --slot-weights, cc->EvalInnerProduct(ct, plaintext, span): upstream calls the reference
// never makes.  Every ciphertext of the input (mean / std_dev / values[] of every layer) goes to HBM once; one
// mkckks_slot_sum_batch runs the log2(span) rotate-and-add steps (span: a power of two, default all N/2 slots), after
// which slot j holds in[j] + ... + in[j + span - 1] -- with the full span every slot holds the sum of all slots.
// --slot-weights <file> (the schema encryptModelWeights reads; slotweights.hpp): every ciphertext is first multiplied by
// the encoded factors of its coordinates and rescaled (mkckks_mult_plain_rescale_batch; the header bookkeeping of
// aggregateEncryptedWeights --slot-weights), so the output holds the encrypted inner product <values, factors> in every
// slot: the alignment score of an update with a public reference vector.
// <rotkeys> is the file rotKeyGen wrote for the key the input is under; a step it lacks is an error that names the step.
// The output keeps the input's envelope form (JSON or MKWS) and the layers' names and shapes.
#include "rotkeys.hpp"
using namespace mkh;

int main(int argc, char *argv[]) {
    auto usage = [&] {
        std::cerr << "Usage: " << argv[0] << " <cc_path> <rotkeys> <input_encfile> <output_encfile> [--span <n>] [--slot-weights <factors.json>]"
                  << std::endl;
        return 1;
    };
    if (argc < 5 || (argc - 5) % 2) return usage();
    const std::string cc_path = argv[1], keys_path = argv[2], input_encfile = argv[3], output_encfile = argv[4];
    SlotWeights sw;
    bool have_span = false;
    uint32_t span = 0;
    for (int i = 5; i < argc; i += 2) {
        const std::string o = argv[i];
        if (o == "--span" && !have_span) {
            int32_t v = 0;
            if (!parse_step(argv[i + 1], v) || v < 1 || (v & (v - 1))) {
                std::cerr << "[slotsum] ERROR: --span needs a power of two of at least 1" << std::endl;
                return 1;
            }
            have_span = true;
            span = (uint32_t)v;
        } else if (o == "--slot-weights" && !sw.on() && *argv[i + 1]) {
            sw.path = argv[i + 1];
        } else {
            return usage();
        }
    }
    if (sw.on()) {
        const std::string err = load_slot_weights(sw.path, sw.file);
        if (!err.empty()) {
            std::cerr << "[slotsum] ERROR: " << err << std::endl;
            return 1;
        }
    }
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[slotsum] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    try {
        Session s(cc);
        const uint32_t N = s.N(), D = s.D(), beta = s.beta();
        if (!have_span) span = N / 2;
        if (span > N / 2) {
            std::cerr << "[slotsum] ERROR: --span " << span << " exceeds the " << N / 2 << " slots" << std::endl;
            return 1;
        }
        RotKeys rk;
        const std::string kerr = read_rot_keys(keys_path, N, D, 2 * beta, rk);
        if (!kerr.empty()) {
            std::cerr << "[slotsum] ERROR: " << kerr << std::endl;
            return 1;
        }
        const std::vector<int32_t> steps = sum_steps(span);
        const size_t key_words = (size_t)beta * 2 * D * N;
        std::vector<const std::vector<uint64_t> *> step_keys;
        for (int32_t r : steps) {
            uint32_t g = 0;
            Session::check(mkckks_galois_element(s.ctx(), r, &g));
            const auto it = rk.keys.find(g);
            if (it == rk.keys.end()) {
                std::cerr << "[slotsum] ERROR: rotation keys " << keys_path << " have no key for step " << r << " (Galois element " << g
                          << "); --span " << span << " needs the steps 1, 2, 4, ... below it (rotKeyGen --sum " << span << ")" << std::endl;
                return 1;
            }
            step_keys.push_back(&it->second);
        }
        std::vector<Json> files(1);
        bool binary = false;  // the output keeps the input's envelope form
        try {
            files[0] = read_envelope(input_encfile, &binary);
            raw_blobs() = binary;
        } catch (const std::exception &) {
            std::cerr << "[slotsum] ERROR: Could not open input encrypted weights file " << input_encfile << std::endl;
            return 1;
        }
        Json outputJson;
        const std::vector<AggItem> items = build_agg_items(files, outputJson);
        if (!items.empty()) {
            std::vector<uint64_t> flat;
            SeedList seeds;
            const Ciphertext first = gather_agg_inputs(items, 1, s, flat, seeds);
            const size_t B = items.size();
            uint64_t *d_in = s.to_device(flat.data(), flat.size());
            seeds.expand(s, d_in, first.nl, 0, B);
            Ciphertext meta = first;
            if (sw.on()) {
                std::vector<double> vals;
                std::string err = slot_weights_headroom_error(s, first, sw);
                if (err.empty()) err = slot_weight_values(s, items, outputJson, sw, vals);
                if (!err.empty()) {
                    std::cerr << "[slotsum] ERROR: " << err << std::endl;
                    return 1;
                }
                uint64_t *d_pt = s.alloc<uint64_t>(B * (size_t)first.nl * N);
                encode_slot_weights(s, vals, B, first, d_pt);
                const AggResult r = scale_aggregate(s, B, d_in, first, 1, false, d_pt);
                d_in = r.d_out;
                meta = r.meta;
            }
            uint64_t *d_keys = s.alloc<uint64_t>(std::max<size_t>(1, steps.size()) * key_words);
            for (size_t k = 0; k < steps.size(); ++k)
                Session::check(mkckks_upload(s.ctx(), d_keys + k * key_words, step_keys[k]->data(), key_words * sizeof(uint64_t)));
            uint64_t *d_out = s.alloc<uint64_t>(B * (size_t)2 * meta.nl * N);
            Session::check(mkckks_slot_sum_batch(s.ctx(), d_in, d_keys, d_out, (uint32_t)B, meta.nl, span));
            store_agg_items(s, items, d_out, meta, outputJson);
            std::cout << "[slotsum] " << B << " ciphertext(s), span " << span << ", " << steps.size() << " rotation(s) each"
                      << (sw.on() ? ", after the per-slot product" : "") << "\n";
        }
        try {
            write_envelope(outputJson, output_encfile, binary);
        } catch (const std::exception &) {
            std::cerr << "[slotsum] ERROR: Failed to open output file " << output_encfile << std::endl;
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << "[slotsum] ERROR: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "[slotsum] Slot sum completed successfully. Output: " << output_encfile << std::endl;
    return 0;
}
