// serverRound -- the server side of one federated round in ONE program.
//
// The reference's server step is a loop of processes (orchestration/server_fns.sh:62-80, orchestration/run.sh:37-43):
//   changeCipherDomain <cc> <rekey_c> <enc_c> <tmp_c>      for every client c that is not in the target key domain
//   aggregateEncryptedWeights <cc> <enc_target> <tmp_...> <out>
// each of which re-loads the CryptoContext, re-parses base64-in-JSON and moves every ciphertext through the host.  Here:
//   serverRound <cc_path> <output_aggfile> <rekey_1|-> <encfile_1> [<rekey_2|-> <encfile_2> ...]
//               [--back <rekey_back_1> <output_encfile_1> [<rekey_back_2> <output_encfile_2> ...]]
// "-" as the re-encryption key marks a client whose ciphertexts already are in the target domain (the reference's
// client 2).  All ciphertexts go to HBM once; the re-encryption of every re-keyed client and the sum over clients is ONE
// mkckks_reencrypt_sum_batch call (cc->ReEncrypt x n at changeCipherDomain.cpp:74 + the EvalAdd chain of
// aggregateEncryptedWeights.cpp:82), then EvalMult(., 1/n) (:83).  The output file is bit-identical to the one the
// per-client programs produce (PRE is deterministic; tests/test_cli_hosts.py).
// After --back: the n-1 re-encryptions of the aggregate into the other clients' key domains (the reference's
// s_changeCipherDomain_c2_c1, server_fns.sh:76-80: changeCipherDomain <cc> <rekey_back_c> <aggfile> <out_c>) -- the
// aggregate stays in HBM, ONE mkckks_reencrypt_fanout_batch over all back keys (which stay resident by file name under
// --rounds); each file equals changeCipherDomain run on <output_aggfile>.  MKCKKS_BACK_LOOP=1: one call per key.
// --back-limbs <k> (after the --back list): every back file is written at k limbs instead of the aggregate's -- what goes
// back is only ever decrypted, so it needs modulus for scale * |value| + noise and no more (include/mkckks.h, headroom
// rule; k is the deployment's choice).  One mkckks_reencrypt_fanout_compact_batch per key group: the aggregate's first
// k + 1 limbs are key-switched and rescaled to k.  With it a back key of "-" names a client that already is in the target
// domain: its file is mkckks_compress_batch of the aggregate.  Each file equals changeCipherDomain ... --limbs <k> run on
// <output_aggfile>; the aggregate file itself is never compacted.
// --hra-back <target_domain_pubkey> [--hra-sigma-bits <s>] (after the --back list): HRA-secure distribution leg,
// cc->ReEncrypt(ct, reKey, publicKey).  The aggregate is re-randomised ONCE per round under the public key of the domain
// it is in (mkckks_rerandomize_batch, errors of sigma = 2^s, s in [6, 56], default 20; fresh OS-drawn key per round) into
// a buffer of its own -- with --back-limbs only its k + 1-limb prefix -- and every keyed back entry is re-encrypted from
// that buffer; all back keys of a round share the one mask, the key-switch noise is per key anyway.  The aggregate file
// and "-" entries are untouched; the public key stays resident by file name.  Back files differ from run to run.
// --weights w_1,...,w_n (anywhere after <output_aggfile>): the weighted mean sum_c w_c x_c / sum_c w_c in place of the plain
// one -- federated averaging by sample count.  One non-negative number per client in argument order, not all zero.  The
// weights ride in what the merged flow reads anyway: the re-encryption keys are scaled once per (key, weight, level) into
// a buffer of their own (mkckks_scale_evk_batch; the unscaled keys stay resident by file name, the scaled copies are
// remade whenever a key's weight or level differs from the one it was scaled with), the sum is
// mkckks_reencrypt_wsum_batch (+ mkckks_eval_wsum_batch for the "-" clients) and ONE mkckks_rescale_batch closes it (for
// noiseScaleDeg-1 inputs: nothing).  The output has the header of the plain mean's; --back, --back-limbs and --hra-back
// work on it as they are.  Refused: a count of weights that is not the count of clients, a negative weight or one that is
// no number, inputs without headroom for the weighted sum (include/mkckks.h).  Without --weights nothing changes.
// --slot-weights <file> (anywhere after <output_aggfile>): every coordinate of the aggregate scaled by a factor of its own
// in place of 1/n -- a plaintext weights_summary JSON in the schema encryptModelWeights reads, split and padded as that
// program splits its input (slotweights.hpp), encoded once and multiplied in by the closing EvalMult with ONE rescale last
// (mkckks_mult_plain_rescale_batch).  Under --rounds the encoded planes stay resident in HBM like the keys (by file name).
// Refused: together with --weights, a missing or unreadable file, a layer of the round the file lacks, another shape or
// value count, a factor that is not finite, inputs without headroom for the largest factor.
// Binary (MKWS) envelopes take the I/O pipeline of iopipe.hpp: files are indexed, not loaded; reader threads fill pinned
// slots, uploads run beside the reads, residues are range-checked on the device, results are written by pwrite() from
// pinned slots.  MKCKKS_SYNC_IO=1 forces the synchronous path (every ciphertext through read_envelope / decode_ct /
// mkckks_upload); both write the same bytes (tests/test_cli_hosts.py).  A "[round] timing" line reports the phases.
// Seeded client ciphertexts (encryptModelWeights --seeded) are accepted per blob on both paths: only c0 is read and
// uploaded, c1 is rebuilt on the device (mkckks_expand_seeded_batch); every output is a full ciphertext.
//   serverRound <cc_path> --rounds <file>
// runs one round per line of <file> (a line = the arguments after <cc_path> above) in ONE process -- what the loop of
// orchestration/run.sh:37-43 does with one process per step: the context, the re-encryption keys (by file name), the
// device arrays, the pinned buffers and the resolved kernels stay from round to round.
#include <fstream>
#include <map>
#include <sstream>

#include "iopipe.hpp"
using namespace mkh;

struct RoundArgs {
    std::string output_file;
    std::vector<std::string> rekey_paths, enc_paths, back_keys, back_outs;
    bool compact = false;     // --back-limbs given
    uint32_t back_limbs = 0;  // its value
    std::string hra_pk;       // --hra-back: public key file of the aggregate's domain (empty: no re-randomisation)
    uint32_t hra_bits = HRA_SIGMA_BITS_DEFAULT;
    bool hra_bits_ok = true;  // false: --hra-sigma-bits was no integer in [6, 56] (reported by run_round)
    bool have_weights = false;  // --weights given
    std::string weights_text;   // its value (judged by run_round, which knows the clients)
    SlotWeights slot;           // --slot-weights: its file, loaded by main before the context
    std::string slot_error;     // --slot-weights without a value or together with --weights (reported by main)
};
// tokens: <output_aggfile> <rekey_1|-> <encfile_1> ... [--back <rekey_back_1> <output_encfile_1> ...]
static bool parse_round(std::vector<std::string> t, RoundArgs &a) {
    bool compact = false;
    uint32_t back_limbs = 0;
    for (size_t i = 1; i < t.size(); ++i)
        if (t[i] == "--back-limbs") {  // one value; taken out before the positional lists are read
            if (i + 1 >= t.size() || t[i + 1].empty() || t[i + 1].size() > 6 ||
                t[i + 1].find_first_not_of("0123456789") != std::string::npos)
                return false;
            compact = true;
            back_limbs = (uint32_t)std::atoi(t[i + 1].c_str());
            t.erase(t.begin() + i, t.begin() + i + 2);
            break;
        }
    bool have_weights = false;
    std::string weights_text;
    for (size_t i = 1; i < t.size(); ++i)
        if (t[i] == "--weights") {  // one value, taken out the same way
            if (i + 1 >= t.size()) return false;
            have_weights = true;
            weights_text = t[i + 1];
            t.erase(t.begin() + i, t.begin() + i + 2);
            break;
        }
    std::string slot_path, slot_error;
    for (size_t i = 1; i < t.size(); ++i)
        if (t[i] == "--slot-weights") {  // one value, taken out the same way; its errors have a line of their own
            const bool has_value = i + 1 < t.size() && !t[i + 1].empty();
            if (has_value) slot_path = t[i + 1];
            else slot_error = "--slot-weights needs a file";
            t.erase(t.begin() + i, t.begin() + i + (i + 1 < t.size() ? 2 : 1));
            break;
        }
    if (!slot_path.empty() && have_weights) slot_error = "--slot-weights cannot be combined with --weights";
    std::string hra_pk;
    uint32_t hra_bits = HRA_SIGMA_BITS_DEFAULT;
    bool hra_bits_ok = true, have_bits = false;
    for (size_t i = 1; i < t.size(); ++i)
        if (t[i] == "--hra-back") {  // one value, taken out the same way
            if (i + 1 >= t.size() || t[i + 1].empty()) return false;
            hra_pk = t[i + 1];
            t.erase(t.begin() + i, t.begin() + i + 2);
            break;
        }
    for (size_t i = 1; i < t.size(); ++i)
        if (t[i] == "--hra-sigma-bits") {
            if (i + 1 >= t.size()) return false;
            have_bits = true;
            hra_bits_ok = parse_hra_sigma_bits(t[i + 1], hra_bits);
            t.erase(t.begin() + i, t.begin() + i + 2);
            break;
        }
    if (have_bits && hra_pk.empty()) return false;
    size_t n_args = t.size();
    for (size_t i = 1; i < t.size(); ++i)
        if (t[i] == "--back") {
            n_args = i;
            break;
        }
    const size_t n_back = t.size() - n_args - (n_args < t.size() ? 1 : 0);
    if (n_args < 3 || (n_args - 1) % 2 != 0 || n_back % 2 != 0 || (n_args < t.size() && n_back == 0)) return false;
    if (compact && n_back == 0) return false;
    if (!hra_pk.empty() && n_back == 0) return false;
    a = RoundArgs{};
    a.hra_pk = hra_pk;
    a.hra_bits = hra_bits;
    a.hra_bits_ok = hra_bits_ok;
    a.compact = compact;
    a.back_limbs = back_limbs;
    a.have_weights = have_weights;
    a.weights_text = weights_text;
    a.slot.path = slot_path;
    a.slot_error = slot_error;
    a.output_file = t[0];
    for (size_t i = 1; i + 1 < n_args; i += 2) {
        a.rekey_paths.push_back(t[i]);
        a.enc_paths.push_back(t[i + 1]);
    }
    for (size_t i = n_args + 1; i + 1 < t.size(); i += 2) {
        a.back_keys.push_back(t[i]);
        a.back_outs.push_back(t[i + 1]);
    }
    return true;
}

struct ServerState {
    explicit ServerState(Session &s) : cache(s) {}
    std::map<std::string, std::vector<uint64_t>> keys;  // re-encryption keys by file name, loaded once per process
    std::map<std::string, std::vector<uint64_t>> pks;   // --hra-back public keys, the same way
    RoundCache cache;
    std::vector<std::string> back_names;  // back keys resident in cache.back_evk, slot by slot (by file name)
    double t_ctx = 0;      // ms: context creation
    size_t n_ct = 0;       // ciphertexts re-encrypted / aggregated so far
};

static const std::vector<uint64_t> *cached_key(Session &s, ServerState &st, const std::string &path) {
    auto it = st.keys.find(path);
    if (it != st.keys.end()) return &it->second;
    std::vector<uint64_t> evk;
    if (!load_eval_key(s, path, evk)) return nullptr;
    return &(st.keys[path] = std::move(evk));
}

static int run_back_leg(Session &s, ServerState &st, const RoundArgs &a, const std::vector<AggItem> &items, const AggResult &agg,
                        const Json &outputJson, bool binary, bool pinned_out, unsigned threads);

// one round; 0 on success, 1 after an "[round] ERROR" line
static int run_round(Session &s, ServerState &st, const RoundArgs &a) {
    const double t_start = now_ms();
    const std::vector<std::string> &rekey_paths = a.rekey_paths, &enc_paths = a.enc_paths;
    const uint32_t N = s.N(), D = s.D(), beta = s.beta();
    const size_t n_clients = enc_paths.size(), evk_words = (size_t)beta * 2 * D * N;
    // clients with a re-encryption key first (their ciphertexts feed mkckks_reencrypt_sum_batch), the others after
    std::vector<size_t> order;
    for (size_t c = 0; c < n_clients; ++c)
        if (rekey_paths[c] != "-") order.push_back(c);
    const size_t n_pre = order.size();
    for (size_t c = 0; c < n_clients; ++c)
        if (rekey_paths[c] == "-") order.push_back(c);
    RoundWeights rw;  // --weights, in device order
    if (a.have_weights) {
        std::vector<double> w;
        const std::string err = parse_weights(a.weights_text, n_clients, w);
        if (!err.empty()) {
            std::cerr << "[round] ERROR: " << err << std::endl;
            return 1;
        }
        for (size_t k = 0; k < n_clients; ++k) rw.w.push_back(w[order[k]]);
    }
    std::vector<const uint64_t *> evk_ptrs;
    std::vector<std::string> evk_names;
    for (size_t k = 0; k < n_pre; ++k) {
        const std::vector<uint64_t> *evk = cached_key(s, st, rekey_paths[order[k]]);
        if (!evk) {
            std::cerr << "[round] ERROR: Failed to load ReKey from " << rekey_paths[order[k]] << std::endl;
            return 1;
        }
        evk_ptrs.push_back(evk->data());
        evk_names.push_back(rekey_paths[order[k]]);
    }
    const double t_keys = now_ms() - t_start;
    std::cout << "[round] " << n_pre << " ReKey(s) loaded\n";
    std::vector<Json> files;
    bool binary = false;  // the output keeps the first input's envelope form
    // binary envelopes: index them (skeleton + blob offsets); anything else goes through read_envelope as before
    const bool want_pipe = !(std::getenv("MKCKKS_SYNC_IO") && std::atoi(std::getenv("MKCKKS_SYNC_IO")) != 0);
    std::vector<EnvelopeIndex> idx(n_clients);
    bool piped = want_pipe;
    const double t_io0 = now_ms();
    for (size_t k = 0; k < n_clients && piped; ++k) {
        try {
            piped = index_envelope(enc_paths[order[k]], idx[k]);
        } catch (const std::exception &) {
            std::cerr << "[round] ERROR: Could not open input encrypted weights file " << enc_paths[order[k]] << std::endl;
            return 1;
        }
    }
    if (piped) {
        binary = true;
        for (size_t k = 0; k < n_clients; ++k) files.push_back(idx[k].doc);
    } else {
        for (size_t k = 0; k < n_clients; ++k) {
            bool b = false;
            try {
                files.push_back(read_envelope(enc_paths[order[k]], &b));
            } catch (const std::exception &) {
                std::cerr << "[round] ERROR: Could not open input encrypted weights file " << enc_paths[order[k]] << std::endl;
                return 1;
            }
            if (k == 0) binary = b;
        }
    }
    raw_blobs() = binary;
    Json outputJson;
    const std::vector<AggItem> items = build_agg_items(files, outputJson);
    AggResult agg;
    const unsigned threads = io_threads();
    bool pinned_out = false;
    // the back leg's arguments are judged before any file is written: the aggregate's shape follows from the first
    // container's header (scale_aggregate's rules)
    for (const std::string &k : a.back_keys)
        if (k == "-" && !a.compact) {
            std::cerr << "[round] ERROR: a back key of - needs --back-limbs" << std::endl;
            return 1;
        }
    if (!a.hra_pk.empty()) {
        if (!a.hra_bits_ok) {
            std::cerr << "[round] ERROR: --hra-sigma-bits needs an integer in [" << HRA_SIGMA_BITS_MIN << ", " << HRA_SIGMA_BITS_MAX
                      << "]" << std::endl;
            return 1;
        }
        if (!st.pks.count(a.hra_pk)) {
            std::vector<uint64_t> pk;
            if (!load_public_key(s, a.hra_pk, pk)) {
                std::cerr << "[round] ERROR: Failed to load public key from " << a.hra_pk << std::endl;
                return 1;
            }
            st.pks[a.hra_pk] = std::move(pk);
        }
    }
    auto first_header = [&] {
        BlobHeader h0{};
        if (piped) {
            const BlobRef &blob0 = idx[0].blobs.at(blob_index(*items[0].blobs[0]));
            if (blob0.size < sizeof(BlobHeader)) throw std::runtime_error("ciphertext blob too short");
            pread_all(idx[0].fd, &h0, sizeof h0, blob0.offset);
        } else {
            const std::string &b = *items[0].blobs[0];
            const bool raw = b.size() >= 4 && !std::memcmp(b.data(), "MKCK", 4);
            const std::string head = raw ? b.substr(0, sizeof h0) : Base64Decode(b.substr(0, sizeof h0 / 3 * 4));
            if (head.size() < sizeof h0) throw std::runtime_error("ciphertext blob too short");
            std::memcpy(&h0, head.data(), sizeof h0);
        }
        return h0;
    };
    if (rw.on() && !items.empty()) {
        const Ciphertext first = meta_of(first_header(), s);
        const std::string err = weights_headroom_error(s, first);
        if (!err.empty()) {
            std::cerr << "[round] ERROR: " << err << std::endl;
            return 1;
        }
        rw.sf_level = weights_sf_level(first);
    }
    const uint64_t *d_slot_pt = nullptr;  // --slot-weights: the encoded factors [B][nl][N], resident from round to round
    if (a.slot.on() && !items.empty()) {
        const Ciphertext first = meta_of(first_header(), s);
        std::vector<double> vals;
        std::string err = slot_weights_headroom_error(s, first, a.slot);
        if (err.empty()) err = slot_weight_values(s, items, outputJson, a.slot, vals);
        if (!err.empty()) {
            std::cerr << "[round] ERROR: " << err << std::endl;
            return 1;
        }
        const size_t pt_words = items.size() * (size_t)first.nl * N;
        const std::string tag = slot_weights_tag(items, outputJson, a.slot, first);
        if (pt_words > st.cache.slot_pt.words) st.cache.slot_tag.clear();  // the array moves: nothing is kept
        uint64_t *d_pt = st.cache.grow(st.cache.slot_pt, pt_words);
        const bool resident = st.cache.slot_tag == tag;
        if (!resident) {
            st.cache.slot_tag.clear();
            encode_slot_weights(s, vals, items.size(), first, d_pt);
            st.cache.slot_tag = tag;
        }
        std::cout << "[round] --slot-weights: " << items.size() << " plaintext(s) " << (resident ? "resident" : "encoded") << "\n";
        d_slot_pt = d_pt;
    }
    if (a.compact) {
        if (a.back_limbs < 1) {
            std::cerr << "[round] ERROR: --back-limbs must be at least 1" << std::endl;
            return 1;
        }
        if (!items.empty()) {
            const BlobHeader h0 = first_header();
            const bool rescale = h0.noise_deg == 2;
            const uint32_t agg_nl = rescale ? h0.limbs - 1 : h0.limbs, agg_deg = rescale ? 2 : h0.noise_deg + 1;
            if (agg_deg != 2) {
                std::cerr << "[round] ERROR: --back-limbs needs the aggregate at noiseScaleDeg 2 (it is at " << agg_deg << ")" << std::endl;
                return 1;
            }
            if (a.back_limbs >= agg_nl) {
                std::cerr << "[round] ERROR: --back-limbs " << a.back_limbs << " is not below the aggregate's " << agg_nl << " limbs"
                          << std::endl;
                return 1;
            }
        }
    }
    if (!items.empty() && piped) {
        RoundPlan plan;
        plan.n_clients = n_clients;
        plan.n_pre = n_pre;
        plan.idx = &idx;
        plan.items = &items;
        plan.evks = evk_ptrs;
        plan.evk_names = &evk_names;
        plan.evk_words = evk_words;
        plan.threads = threads;
        plan.weights = rw;
        plan.slot_pt = d_slot_pt;
        RoundTimes tm;
        agg = run_round_pipeline(s, plan, outputJson, a.output_file, st.cache, tm);
        pinned_out = true;
        const double n_ct = (double)(n_clients * items.size());
        std::cout << "[round] timing: " << n_clients << " clients x " << items.size() << " ciphertexts, chunks of " << tm.chunk
                  << " indices, " << threads << " I/O threads: files to file " << tm.round << " ms -> " << n_ct / tm.round * 1e3
                  << " ciphertexts/s, input " << tm.in_bytes / 1048576.0 << " MiB (" << tm.n_seeded << " seeded ciphertexts) = "
                  << tm.in_bytes / tm.round * 1e-6 << " GB/s (last upload done at " << tm.last_upload << " ms, last download at " << tm.last_download
                  << " ms; reader threads busy " << tm.read_busy << " ms, writer threads " << tm.write_busy
                  << " ms in total); before it: context (HIP start-up, tables; once per process) " << st.t_ctx
                  << " ms, re-encryption key file(s) not yet loaded " << t_keys << " ms, index + buffers + key upload + warm-up "
                  << now_ms() - t_io0 - tm.round << " ms\n";
    } else if (!items.empty()) {
        const size_t B = items.size();
        const size_t n_plain = n_clients - n_pre;
        std::vector<uint64_t> flat;  // [client in `order`][ct][2][nl][N]
        SeedList seeds;              // seeded inputs: c1 rebuilt on the device after the upload of c0
        const Ciphertext first = gather_agg_inputs(items, n_clients, s, flat, seeds);
        const size_t words = (size_t)2 * first.nl * N, blk = B * words;
        // device layout: [re-keyed clients][one slot for their re-encrypted sum][clients already in the domain]:
        // the slot and what follows it are the terms of the final n-ary EvalAdd, no copy in between
        uint64_t *d_all = st.cache.grow(st.cache.all, (n_clients + 1) * blk), *d_slot = d_all + n_pre * blk;
        if (n_pre) Session::check(mkckks_upload(s.ctx(), d_all, flat.data(), n_pre * blk * 8));
        if (n_plain) Session::check(mkckks_upload(s.ctx(), d_slot + blk, flat.data() + n_pre * blk, n_plain * blk * 8));
        const uint32_t nl = first.nl;
        seeds.expand(s, d_all, nl, 0, n_pre * B);
        seeds.expand(s, d_slot + blk, nl, n_pre * B, n_plain * B);
        uint64_t *d_sum = d_slot;
        if (n_pre) {
            uint64_t *d_evk = st.cache.grow(st.cache.evk, n_pre * evk_words);
            st.cache.evk_names.clear();
            for (size_t k = 0; k < n_pre; ++k) Session::check(mkckks_upload(s.ctx(), d_evk + k * evk_words, evk_ptrs[k], evk_words * 8));
            st.cache.evk_names = evk_names;
            if (rw.on()) {  // this path uploads the keys every round, so their scaled copies are made every round
                st.cache.scaled_tag.clear();
                uint64_t *d_evk_s = st.cache.grow(st.cache.evk_scaled, n_pre * evk_words);
                Session::check(mkckks_scale_evk_batch(s.ctx(), d_evk, d_evk_s, (uint32_t)n_pre, rw.w.data(), rw.sf_level));
                Session::check(mkckks_reencrypt_wsum_batch(s.ctx(), d_all, d_evk_s, d_slot, (uint32_t)n_pre, (uint32_t)B, nl,
                                                           rw.w.data(), rw.sf_level));
            } else {
                Session::check(mkckks_reencrypt_sum_batch(s.ctx(), d_all, d_evk, d_slot, (uint32_t)n_pre, (uint32_t)B, nl));
            }
        }
        if (n_plain) {
            const uint64_t *d_terms = n_pre ? d_slot : d_slot + blk;
            d_sum = st.cache.grow(st.cache.sum, blk);
            if (rw.on())  // the slot of the re-keyed clients' sum is term 0 and enters as it is
                Session::check(mkckks_eval_wsum_batch(s.ctx(), d_terms, d_sum, (uint32_t)(n_plain + (n_pre ? 1 : 0)), (uint32_t)B, nl,
                                                      rw.w.data() + n_pre - (n_pre ? 1 : 0), rw.sf_level, n_pre ? 1 : 0));
            else
                Session::check(mkckks_eval_sum_batch(s.ctx(), d_terms, d_sum, (uint32_t)(n_plain + (n_pre ? 1 : 0)), (uint32_t)B, nl));
        }
        agg = finish_aggregate(s, items, d_sum, first, n_clients, outputJson, rw.on(), d_slot_pt);
    }
    if (!pinned_out) write_envelope(outputJson, a.output_file, binary);
    if (int rc = run_back_leg(s, st, a, items, agg, outputJson, binary, pinned_out, threads)) return rc;
    st.n_ct += n_clients * items.size();
    std::cout << "[round] Re-encryption and aggregation completed successfully. Output: " << a.output_file << std::endl;
    return 0;
}

// The distribution leg (--back): the aggregate, still in HBM, re-encrypted into every other client's key domain.  All
// back keys of the round live in ONE device array and the leg is one mkckks_reencrypt_fanout_batch call per group of
// keys (the key-independent half of the key switch runs once per ciphertext instead of once per key).  The keys stay
// resident from round to round by FILE NAME, slot by slot, under the same assumption as the inbound keys: a file that
// keeps its name keeps its content for the life of the process (keys rotated in place need a new process or a new name).
// MKCKKS_BACK_LOOP=1 keeps the per-key loop (one upload + one mkckks_reencrypt_batch per key); both write the same bytes.
static int run_back_leg(Session &s, ServerState &st, const RoundArgs &a, const std::vector<AggItem> &items, const AggResult &agg,
                        const Json &outputJson, bool binary, bool pinned_out, unsigned threads) {
    if (a.back_keys.empty()) return 0;
    const double t_leg = now_ms();
    const uint32_t N = s.N();
    const size_t evk_words = (size_t)s.beta() * 2 * s.D() * N, B = items.size();
    const bool loop = std::getenv("MKCKKS_BACK_LOOP") && std::atoi(std::getenv("MKCKKS_BACK_LOOP")) != 0;
    // --back-limbs k: every file carries k limbs at noiseScaleDeg 1 (the header of Rescale(prefix(., k + 1)))
    const uint32_t k_limbs = a.compact ? a.back_limbs : 0, out_nl = k_limbs ? k_limbs : agg.meta.nl;
    Ciphertext meta = agg.meta;
    if (k_limbs && B) {
        if (agg.meta.noise_deg != 2 || k_limbs >= agg.meta.nl) throw std::runtime_error("--back-limbs does not fit the aggregate");
        meta.level = agg.meta.level + (agg.meta.nl - k_limbs);
        meta.nl = k_limbs;
        meta.noise_deg = 1;
        meta.scale = agg.meta.scale / (double)s.moduli()[k_limbs];
    }
    // entries in order up to the first key that does not load: the files before it are written, then the error (as the
    // loop did); "-" (compact form only) is the client that needs no key switch
    std::vector<const std::vector<uint64_t> *> keys;  // per entry; null for "-"
    for (size_t k = 0; k < a.back_keys.size(); ++k) {
        if (a.back_keys[k] == "-") {
            keys.push_back(nullptr);
            continue;
        }
        const std::vector<uint64_t> *evk = cached_key(s, st, a.back_keys[k]);
        if (!evk) break;
        keys.push_back(evk);
    }
    const size_t n_entries = keys.size();
    std::vector<size_t> real, plain;  // entries with a key / without
    for (size_t k = 0; k < n_entries; ++k) (keys[k] ? real : plain).push_back(k);
    const size_t n_keys = real.size();
    size_t uploaded = 0;
    auto write_one = [&](size_t k, uint64_t *d_back) {
        Json backJson = outputJson;  // layer / shape carried over; blobs replaced below
        if (B) {
            if (pinned_out) {
                write_envelope_from_device(s, *st.cache.ring, items, d_back, meta, backJson, a.back_outs[k], threads);
            } else {
                store_agg_items(s, items, d_back, meta, backJson);
                write_envelope(backJson, a.back_outs[k], binary);
            }
        } else {
            write_envelope(backJson, a.back_outs[k], binary);
        }
        if (keys[k]) std::cout << "[round] aggregate re-encrypted with " << a.back_keys[k] << " -> " << a.back_outs[k] << "\n";
        else std::cout << "[round] aggregate compressed for its own domain -> " << a.back_outs[k] << "\n";
    };
    const size_t words = B * (size_t)2 * out_nl * N;  // one key's output
    // --hra-back: what the keyed entries read is the re-randomised aggregate (its k + 1-limb prefix with --back-limbs),
    // one re-randomisation per round; agg.d_out itself stays as it is
    const uint64_t *d_src = agg.d_out;
    uint32_t src_nl = agg.meta.nl;
    const bool hra = !a.hra_pk.empty();
    if (hra && B && n_keys) {
        const std::vector<uint64_t> &pk = st.pks.at(a.hra_pk);
        if (pk.size() > st.cache.hra_pk.words) st.cache.hra_pk_name.clear();
        uint64_t *d_pk = st.cache.grow(st.cache.hra_pk, pk.size());
        if (st.cache.hra_pk_name != a.hra_pk) {
            st.cache.hra_pk_name.clear();
            Session::check(mkckks_upload(s.ctx(), d_pk, pk.data(), pk.size() * 8));
            st.cache.hra_pk_name = a.hra_pk;
        }
        src_nl = k_limbs ? k_limbs + 1 : agg.meta.nl;
        uint64_t *d_rr = st.cache.grow(st.cache.hra, B * (size_t)2 * src_nl * N);
        hra_rerandomize(s, agg.d_out, d_pk, st.cache.grow(st.cache.hra_rand, hra_scratch_words(B, N)), d_rr, (uint32_t)B,
                        agg.meta.nl, src_nl, a.hra_bits, fresh_key());
        d_src = d_rr;
    }
    if (!loop && B && n_keys) {
        // keys per call: the outputs of one call are bounded (MKCKKS_BACK_MAX_MIB, default 16 GiB) beside the round's buffers
        size_t max_mib = 16384;
        if (const char *e = std::getenv("MKCKKS_BACK_MAX_MIB")) max_mib = (size_t)std::max(1, std::atoi(e));
        const size_t per_call = std::max<size_t>(1, std::min(n_keys, (max_mib << 20) / (words * 8)));
        if (n_keys * evk_words > st.cache.back_evk.words) st.back_names.clear();  // the array moves: nothing is resident
        uint64_t *d_evks = st.cache.grow(st.cache.back_evk, n_keys * evk_words);
        uint64_t *d_back = st.cache.grow(st.cache.back, per_call * words);
        st.back_names.resize(std::max(st.back_names.size(), n_keys));
        for (size_t k = 0; k < n_keys; ++k) {
            if (st.back_names[k] == a.back_keys[real[k]]) continue;  // resident in its slot
            st.back_names[k].clear();
            Session::check(mkckks_upload(s.ctx(), d_evks + k * evk_words, keys[real[k]]->data(), evk_words * 8));
            st.back_names[k] = a.back_keys[real[k]];
            ++uploaded;
        }
        for (size_t k0 = 0; k0 < n_keys; k0 += per_call) {
            const size_t gk = std::min(per_call, n_keys - k0);
            if (k_limbs)
                Session::check(mkckks_reencrypt_fanout_compact_batch(s.ctx(), d_src, d_evks + k0 * evk_words, d_back,
                                                                     (uint32_t)gk, (uint32_t)B, src_nl, k_limbs));
            else
                Session::check(mkckks_reencrypt_fanout_batch(s.ctx(), d_src, d_evks + k0 * evk_words, d_back, (uint32_t)gk,
                                                             (uint32_t)B, src_nl));
            for (size_t k = 0; k < gk; ++k) write_one(real[k0 + k], d_back + k * words);
        }
    } else {
        for (size_t k = 0; k < n_keys; ++k) {  // one key at a time through slot 0 of the key array
            uint64_t *d_back = nullptr;
            if (B) {
                st.back_names.clear();
                d_back = st.cache.grow(st.cache.back, words);
                uint64_t *d_back_evk = st.cache.grow(st.cache.back_evk, evk_words);
                Session::check(mkckks_upload(s.ctx(), d_back_evk, keys[real[k]]->data(), evk_words * 8));
                ++uploaded;
                if (k_limbs)
                    Session::check(mkckks_reencrypt_fanout_compact_batch(s.ctx(), d_src, d_back_evk, d_back, 1, (uint32_t)B,
                                                                         src_nl, k_limbs));
                else
                    Session::check(mkckks_reencrypt_batch(s.ctx(), d_src, d_back_evk, d_back, (uint32_t)B, src_nl));
            }
            write_one(real[k], d_back);
        }
    }
    for (size_t k : plain) {  // the client that already is in the target domain: no key switch, the rescale alone
        uint64_t *d_back = nullptr;
        if (B) {
            d_back = st.cache.grow(st.cache.back, words);
            Session::check(mkckks_compress_batch(s.ctx(), agg.d_out, d_back, (uint32_t)B, agg.meta.nl, k_limbs));
        }
        write_one(k, d_back);
    }
    if (n_entries < a.back_keys.size()) {
        std::cerr << "[round] ERROR: Failed to load ReKey from " << a.back_keys[n_entries] << std::endl;
        return 1;
    }
    const double ms = now_ms() - t_leg;
    std::cout << "[round] back leg: " << n_entries << " keys x " << B << " ciphertexts in " << ms << " ms -> "
              << (double)(n_entries * B) / ms * 1e3 << " ciphertexts/s, " << uploaded << " key(s) uploaded";
    if (k_limbs) std::cout << ", " << k_limbs << " limbs";
    if (hra) std::cout << ", re-randomised at sigma 2^" << a.hra_bits;
    std::cout << "\n";
    return 0;
}

int main(int argc, char *argv[]) {
    auto usage = [&] {
        std::cerr << "Usage: " << argv[0] << " <cc_path> <output_aggfile> <rekey_1|-> <encfile_1> [<rekey_2|-> <encfile_2> ...]"
                  << " [--weights <w_1,...,w_n> | --slot-weights <factors.json>] [--back <rekey_back_1|-> <output_encfile_1> ... [--back-limbs <k>] [--hra-back <target_domain_pubkey> [--hra-sigma-bits <s>]]]\n       " << argv[0]
                  << " <cc_path> --rounds <file with one such argument list (after <cc_path>) per line>" << std::endl;
        return 1;
    };
    if (argc < 4) return usage();
    const std::string cc_path = argv[1];
    std::vector<RoundArgs> rounds;
    if (std::string(argv[2]) == "--rounds") {
        if (argc != 4) return usage();
        std::ifstream f(argv[3]);
        if (!f) {
            std::cerr << "[round] ERROR: Could not open rounds file " << argv[3] << std::endl;
            return 1;
        }
        std::string line;
        while (std::getline(f, line)) {
            std::istringstream ls(line);
            std::vector<std::string> t;
            for (std::string w; ls >> w;) t.push_back(w);
            if (t.empty() || t[0][0] == '#') continue;
            RoundArgs a;
            if (!parse_round(t, a)) {
                std::cerr << "[round] ERROR: malformed round (line " << rounds.size() + 1 << " of " << argv[3] << ")" << std::endl;
                return 1;
            }
            rounds.push_back(std::move(a));
        }
        if (rounds.empty()) return usage();
    } else {
        RoundArgs a;
        if (!parse_round(std::vector<std::string>(argv + 2, argv + argc), a)) return usage();
        rounds.push_back(std::move(a));
    }
    for (RoundArgs &a : rounds) {  // the --slot-weights refusals that need no context come before anything is loaded
        std::string err = a.slot_error;
        if (err.empty() && a.slot.on()) err = load_slot_weights(a.slot.path, a.slot.file);
        if (!err.empty()) {
            std::cerr << "[round] ERROR: " << err << std::endl;
            return 1;
        }
    }
    const double t_start = now_ms();
    CcFile cc;
    try {
        cc = read_cc(cc_path);
    } catch (const std::exception &) {
        std::cerr << "[round] ERROR: Failed to load CryptoContext from " << cc_path << std::endl;
        return 1;
    }
    try {
        Session s(cc);
        ServerState st(s);
        st.t_ctx = now_ms() - t_start;
        std::cout << "[round] CryptoContext loaded\n";
        const double t_rounds = now_ms();
        for (size_t r = 0; r < rounds.size(); ++r) {
            const double t_r = now_ms();
            if (run_round(s, st, rounds[r])) return 1;
            if (rounds.size() > 1)
                std::cout << "[round] round " << r + 1 << " of " << rounds.size() << ": " << now_ms() - t_r << " ms wall\n";
        }
        if (rounds.size() > 1) {
            const double ms = now_ms() - t_rounds;
            std::cout << "[round] " << rounds.size() << " rounds, " << st.n_ct << " ciphertexts in " << ms << " ms wall after the context ("
                      << st.t_ctx << " ms) = " << (double)st.n_ct / ms * 1e3 << " ciphertexts/s, " << (double)st.n_ct / (ms + st.t_ctx) * 1e3
                      << " with it\n";
        }
    } catch (const std::exception &e) {
        std::cerr << "[round] ERROR: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
