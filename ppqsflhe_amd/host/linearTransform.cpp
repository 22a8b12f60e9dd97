// linearTransform -- a public linear map applied to every ciphertext of an envelope by the diagonal method:
// `linearTransform <cc_path> <rotkeys> (<diagonals.json> | --block <matrix.json>) <input_encfile> <output_encfile>`.
// EvalLinearTransform with hoisted rotations (cc->EvalFastRotationPrecompute / cc->EvalFastRotation): upstream calls the
// reference never makes.  out[j] = sum_r diag_r[j] * in[(j + r) mod N/2] over the diagonals of the file (lintrans.hpp:
// {"diagonals": [{"step": r, "values": [...]}]}, values zero padded to the N/2 slots; step 0 needs no key), or, with
// --block, the n x n matrix of {"matrix": [[...]]} applied to every aligned n-slot block of the slots.  Every ciphertext
// of the input (mean / std_dev / values[] of every layer) goes to HBM once; the diagonals are encoded over the extended
// basis once (mkckks_encode_ext_batch) and one mkckks_linear_transform_batch runs all rotations on one ModUp per
// ciphertext and closes with one ModDown per component.  The result is rescaled and written with the header bookkeeping of
// aggregateEncryptedWeights --slot-weights (a plaintext product: one rescale on a noiseScaleDeg-2 input, none on a
// noiseScaleDeg-1 input, whose degree rises).
// <rotkeys> is the file rotKeyGen --steps wrote for the key the input is under (a file fuseEvalKeys made of the parties'
// shares works unchanged); a step it lacks is an error that names the step.  The output keeps the input's envelope form
// (JSON or MKWS) and the layers' names and shapes.
// With a trailing `--bsgs <n1|auto>` the transform runs in its baby-step giant-step form (bsgs.hpp;
// mkckks_linear_transform_bsgs_batch): the key file needs the keys of the plan's baby and giant steps only, about
// n1 + n2 where the direct form needs one per diagonal.  `linearTransform <cc_path> --bsgs-steps <n1|auto>
// (<diagonals.json> | --block <matrix.json>)` needs no device and no key file: it prints the plan's steps, the list
// rotKeyGen --steps takes.
#include "bsgs.hpp"
#include "lintrans.hpp"
#include "rotkeys.hpp"
using namespace mkh;

// linearTransform <cc_path> --bsgs-steps <n1|auto> (<diagonals.json> | --block <matrix.json>)
static int bsgs_steps_main(int argc, char *argv[]) {
    const bool block = argc == 6;
    if (block && std::string(argv[4]) != "--block") return -1;
    uint32_t n1 = 0;
    std::string err = bsgs_parse_n1(argv[3], n1);
    CcFile cc;
    if (err.empty()) {
        try {
            cc = read_cc(argv[1]);
        } catch (const std::exception &) {
            std::cerr << "[lintrans] ERROR: Failed to load CryptoContext from " << argv[1] << std::endl;
            return 1;
        }
    }
    Diagonals dg;
    BsgsPlan plan;
    const size_t slots = err.empty() ? (size_t)1 << (cc.p.log_n - 1) : 0;
    if (err.empty()) err = load_diagonals(argv[block ? 5 : 4], block, slots, dg);
    if (err.empty()) err = bsgs_plan(dg, slots, n1, false, plan);
    if (!err.empty()) {
        std::cerr << "[lintrans] ERROR: " << err << std::endl;
        return 1;
    }
    std::cout << bsgs_steps_line(plan) << std::endl;
    return 0;
}

int main(int argc, char *argv[]) {
    auto usage = [&] {
        std::cerr << "Usage: " << argv[0]
                  << " <cc_path> <rotkeys> (<diagonals.json> | --block <matrix.json>) <input_encfile> <output_encfile>"
                     " [--bsgs <n1|auto>]\n       "
                  << argv[0] << " <cc_path> --bsgs-steps <n1|auto> (<diagonals.json> | --block <matrix.json>)" << std::endl;
        return 1;
    };
    if ((argc == 5 || argc == 6) && std::string(argv[2]) == "--bsgs-steps") {
        const int rc = bsgs_steps_main(argc, argv);
        return rc < 0 ? usage() : rc;
    }
    bool bsgs = false;
    uint32_t bsgs_n1 = 0;
    if (argc >= 8 && std::string(argv[argc - 2]) == "--bsgs") {
        const std::string err = bsgs_parse_n1(argv[argc - 1], bsgs_n1);
        if (!err.empty()) {
            std::cerr << "[lintrans] ERROR: " << err << std::endl;
            return 1;
        }
        bsgs = true;
        argc -= 2;
    }
    if (argc != 6 && argc != 7) return usage();
    const bool block = argc == 7;
    if (block && std::string(argv[3]) != "--block") return usage();
    if (!block && std::string(argv[3]).rfind("--", 0) == 0) return usage();
    const std::string cc_path = argv[1], keys_path = argv[2], diag_path = argv[block ? 4 : 3];
    const std::string input_encfile = argv[block ? 5 : 4], output_encfile = argv[block ? 6 : 5];
    if (diag_path.empty()) return usage();
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[lintrans] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    Diagonals dg;
    {
        const std::string err = load_diagonals(diag_path, block, (size_t)1 << (cc.p.log_n - 1), dg);
        if (!err.empty()) {
            std::cerr << "[lintrans] ERROR: " << err << std::endl;
            return 1;
        }
    }
    try {
        Session s(cc);
        const uint32_t N = s.N(), D = s.D(), beta = s.beta(), K = s.K();
        const size_t slots = N / 2, n_rot = dg.steps.size();
        RotKeys rk;
        const std::string kerr = read_rot_keys(keys_path, N, D, 2 * beta, rk);
        if (!kerr.empty()) {
            std::cerr << "[lintrans] ERROR: " << kerr << std::endl;
            return 1;
        }
        const size_t key_words = (size_t)beta * 2 * D * N;
        // the steps whose keys the call reads: the diagonals' own, or (--bsgs) the plan's babies, then its giants
        BsgsPlan plan;
        if (bsgs) {
            const std::string perr = bsgs_plan(dg, slots, bsgs_n1, true, plan);
            if (!perr.empty()) {
                std::cerr << "[lintrans] ERROR: " << perr << std::endl;
                return 1;
            }
        }
        const size_t n1 = plan.babies.size(), n2 = plan.giants.size();
        std::vector<int32_t> key_steps = dg.steps;
        if (bsgs) {
            key_steps = plan.babies;
            key_steps.insert(key_steps.end(), plan.giants.begin(), plan.giants.end());
        }
        const size_t n_keys = key_steps.size();
        std::vector<uint32_t> gs(n_keys);
        std::vector<const std::vector<uint64_t> *> step_keys(n_keys, nullptr);
        for (size_t k = 0; k < n_keys; ++k) {
            Session::check(mkckks_galois_element(s.ctx(), key_steps[k], &gs[k]));
            if (gs[k] == 1) continue;  // no rotation: no key
            if (bsgs && k < n1) {      // a baby no present entry uses is not computed: no key
                bool used = false;
                for (size_t t = 0; t < n2; ++t) used = used || plan.present[t * n1 + k];
                if (!used) continue;
            }
            const auto it = rk.keys.find(gs[k]);
            if (it == rk.keys.end()) {
                std::cerr << "[lintrans] ERROR: rotation keys " << keys_path << " have no key for step " << key_steps[k]
                          << " (Galois element " << gs[k] << "); rotKeyGen --steps makes the keys of the diagonals' steps" << std::endl;
                return 1;
            }
            step_keys[k] = &it->second;
        }
        std::vector<Json> files(1);
        bool binary = false;  // the output keeps the input's envelope form
        try {
            files[0] = read_envelope(input_encfile, &binary);
            raw_blobs() = binary;
        } catch (const std::exception &) {
            std::cerr << "[lintrans] ERROR: Could not open input encrypted weights file " << input_encfile << std::endl;
            return 1;
        }
        Json outputJson;
        const std::vector<AggItem> items = build_agg_items(files, outputJson);
        if (!items.empty()) {
            std::vector<uint64_t> flat;
            SeedList seeds;
            const Ciphertext first = gather_agg_inputs(items, 1, s, flat, seeds);
            const size_t B = items.size();
            const uint32_t nl = first.nl;
            double log_q = 0;
            for (uint32_t i = 0; i < nl; ++i) log_q += std::log2((double)s.moduli()[i]);
            const double sf = s.sf(weights_sf_level(first), false);
            const std::string herr = diagonals_headroom_error(std::log2(first.scale), std::log2(sf), dg.max_abs_sum, log_q, nl);
            if (!herr.empty()) {
                std::cerr << "[lintrans] ERROR: " << herr << std::endl;
                return 1;
            }
            if (first.noise_deg == 2 && nl < 2) throw std::runtime_error("ciphertext has no limb left to rescale");
            uint64_t *d_in = s.to_device(flat.data(), flat.size());
            seeds.expand(s, d_in, nl, 0, B);
            // the diagonals over the extended basis, at the scaling factor of a plaintext product with these ciphertexts
            const std::vector<double> &vals = bsgs ? plan.values : dg.values;  // --bsgs: [n2][n1][slots], absent entries zero
            const size_t n_pts = vals.size() / slots;
            double *d_vals = s.to_device(vals.data(), vals.size());
            uint64_t *d_pts = s.alloc<uint64_t>(n_pts * (size_t)(nl + K) * N);
            Session::check(mkckks_encode_ext_batch(s.ctx(), d_vals, d_pts, (uint32_t)n_pts, nl, sf));
            uint64_t *d_keys = s.alloc<uint64_t>(n_keys * key_words);  // --bsgs: the babies' slots, then the giants'
            for (size_t k = 0; k < n_keys; ++k)
                if (step_keys[k])
                    Session::check(mkckks_upload(s.ctx(), d_keys + k * key_words, step_keys[k]->data(), key_words * sizeof(uint64_t)));
            uint64_t *d_lt = s.alloc<uint64_t>(B * (size_t)2 * nl * N);
            if (bsgs)
                Session::check(mkckks_linear_transform_bsgs_batch(s.ctx(), d_in, d_keys, gs.data(), (uint32_t)n1, d_keys + n1 * key_words,
                                                                  gs.data() + n1, (uint32_t)n2, d_pts, plan.present.data(), d_lt,
                                                                  (uint32_t)B, nl));
            else
                Session::check(mkckks_linear_transform_batch(s.ctx(), d_in, d_keys, d_pts, gs.data(), d_lt, (uint32_t)n_rot, (uint32_t)B, nl));
            // the bookkeeping of a plaintext product (scale_aggregate's --slot-weights rules)
            Ciphertext meta = first;
            uint64_t *d_out = d_lt;
            if (first.noise_deg == 2) {
                d_out = s.alloc<uint64_t>(B * (size_t)2 * (nl - 1) * N);
                Session::check(mkckks_rescale_batch(s.ctx(), d_lt, d_out, (uint32_t)B, nl));
                meta.nl = nl - 1;
                meta.level = first.level + 1;
                meta.scale = first.scale / (double)s.moduli()[nl - 1] * s.sf(meta.level, false);
                meta.noise_deg = 2;
            } else {
                meta.scale = first.scale * s.sf(first.level, false);
                meta.noise_deg = first.noise_deg + 1;
            }
            store_agg_items(s, items, d_out, meta, outputJson);
            std::cout << "[lintrans] " << B << " ciphertext(s), " << n_rot << " diagonal(s) each, " << slots << " slots\n";
            if (bsgs)
                std::cout << "[lintrans] bsgs n1=" << plan.n1 << ": " << plan.n_babies << " baby and " << plan.n_giants
                          << " giant key(s)\n";
        }
        try {
            write_envelope(outputJson, output_encfile, binary);
        } catch (const std::exception &) {
            std::cerr << "[lintrans] ERROR: Failed to open output file " << output_encfile << std::endl;
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << "[lintrans] ERROR: " << e.what() << std::endl;
        return 1;
    }
    std::cout << "[lintrans] Linear transform completed successfully. Output: " << output_encfile << std::endl;
    return 0;
}
