// engine.hpp -- device-resident context + batched operations behind the C-ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "modarith.hpp"
#include "ntt_kernels.hpp"
#include "params.hpp"

namespace mk {

constexpr uint32_t SHAMIR_MAX_PARTIES = 64;  // parties of one key sharing: MKCKKS_MAX_PARTIES (capi.cpp asserts it)

struct HipError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
struct NoDevice : std::runtime_error {
    using std::runtime_error::runtime_error;
};
// decode_flood: an item's decryption-noise estimate exceeds the context's precision (log2 sigma > scaling_bits - 5)
struct PrecisionError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define MK_HIP(expr)                                                                              \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            throw mk::HipError(std::string(#expr) + ": " + hipGetErrorString(_e) + " (" __FILE__ \
                               ":" + std::to_string(__LINE__) + ")");                             \
    } while (0)

constexpr int MAX_CONV_IN = 8;    // alpha, K <= 8
constexpr int MAX_CONV_OUT = 40;  // complement limbs of one digit

// device image of one BaseConvTable, passed to k_conv_col by value (constant/SGPR space)
struct DevConv {
    uint32_t n_in, n_out;
    uint32_t src_id[MAX_CONV_IN];     // limb ids of the sources
    uint32_t src_slot[MAX_CONV_IN];   // slot of each source inside the input polynomial
    uint32_t dst_id[MAX_CONV_OUT];    // limb ids of the targets
    uint32_t dst_slot[MAX_CONV_OUT];  // slot of each target inside the output polynomial
    u64 hatinv[MAX_CONV_IN], hatinv_sh[MAX_CONV_IN];
    const u64 *hat;        // device, [n_in][n_out]: [S/s_i]_t
    const double *hat_d;   // device, [n_in][n_out]: the same as doubles (used for fp64-class targets)
    const double *hatq_d;  // device, [n_in][n_out]: [S/s_i]_t / t
    const double *hat30_d;  // device, [2][n_out]: [S/s_0 * 2^30]_t and its quotient by t (packed source 0, fp64-class targets)
};

// Switches of the library (environment variables MKCKKS_*), read once when a context is created.  Defaults are the
// measured best; every non-default value has a parity test (tests/test_gpu_parity.py).
struct Knobs {
    uint32_t chunk = 16;         // MKCKKS_CHUNK: ciphertexts per workspace chunk
    uint32_t fanout_group = 7;   // MKCKKS_FANOUT_GROUP: keys per pass of the fan-out re-encryption (bounds the til / ModDown
                                 // workspace; ModUp is shared by all keys whatever the group; 7 is the best of 1, 2, 4, 7 at both
                                 // measured shapes, profiles/fanout_ab.txt)
    uint32_t qsum_group = 8;     // MKCKKS_QSUM_GROUP: clients per pass of the merged n-client flow (one forward transform of
                                 // the summed ModDown conversions per group: 8 is +2.7 % against 4, 2 is -6.6 %)
    bool cu_affine = true;       // MKCKKS_CU_AFFINE=0: plain XCD-aware placement; default: workgroups that share operand tiles on the same CU (group_member)
    bool generic_ntt = false;    // MKCKKS_GENERIC_NTT=1: LDS-stage kernels for both passes
    bool no_pm = false;          // MKCKKS_NO_PM=1: Shoup butterflies on the integer limbs instead of the pseudo-Mersenne ones
    bool no_fp64 = false;        // MKCKKS_NO_FP64=1: integer arithmetic on every limb
    int q0_walk = 2;             // MKCKKS_Q0_WALK=0/1/auto: the integer-class Q limbs of the merged n-client flow as two kernels
                                 // (k_row3_inner_int + k_row3_tail_once), as one (k_qsum3_int), or chosen per call by grid size
    int plain_fused = 2;         // MKCKKS_PLAIN_FUSED=0/1: mult_plain_rescale as the composition (k_mul_plain + rescale) or fused
                                 // into the rescale's two row passes; default: fused wherever the plain rescale is
                                 // (profiles/slot_weights_ab.txt)
    int icol_conv = -1;          // MKCKKS_ICOL_CONV=0/1/2/3/auto: fp64-class ModUp targets of an all-fp64 digit converted inside the
                                 // inverse column pass of its sources (k_icol_conv); 0: none, 1..3: that many wherever the digit
                                 // has them, default: icol_conv_targets (profiles/icol_conv_ab.txt)
    int relshare_fused = 2;      // MKCKKS_RELSHARE_FUSED=0/1: relin_share as the composition (k_lift + transform + k_fma) or as
                                 // k_relshare_col + k_relshare_row; default: fused wherever the other fused endpoints are
                                 // (profiles/collective_keys_ab.txt)
    int lt_order = 0;            // MKCKKS_LT_ORDER=0/1/2: how k_lt_accum reuses the key and plaintext tiles the ciphertexts of a
                                 // chunk share; 0: the workgroups of one (limb, tile) are neighbours on one XCD, 1: one
                                 // workgroup walks the chunk's ciphertexts, 2: ciphertext-major grid, no reuse intended
                                 // (profiles/linear_transform_ab.txt)
    int poly_fused = 2;          // MKCKKS_POLY_FUSED=0/1: poly_tensor as the composition (eval_wsum per giant index on packed prefix
                                 // copies + tensor_sum + the constant column and term) or as k_poly_tensor; default:
                                 // poly_tensor_fused (profiles/poly_ab.txt)
    int cheb_fused = 2;          // MKCKKS_CHEB_FUSED=0/1: a Chebyshev ladder step before its relinearisation as the composition
                                 // (packed prefix copies + k_tensor + k_wsum_ct / k_poly_add_const) or as k_cheb_tensor;
                                 // default: cheb_step_fused (profiles/cheb_ab.txt)
    int bsgs_fused = 1;          // MKCKKS_BSGS_FUSED=0: linear_transform_bsgs as the composition of k_lt_accum (one rotation, an
                                 // all-ones plaintext) per baby and per giant, k_fma and k_automorph; default: k_bsgs_baby,
                                 // k_bsgs_inner, k_bsgs_giant (profiles/lt_bsgs_ab.txt)
    uint32_t bsgs_ws_mib = 2048; // MKCKKS_BSGS_WS_MIB: cap on the workspace of linear_transform_bsgs (babies, inner sums and
                                 // giant digits are per ciphertext); the chunk shrinks to fit, down to one ciphertext
    static Knobs from_env();
};

// The form the integer-class Q limbs (q_0) of the merged n-client flow take in a call with `tiles` row tiles, `nsel` such
// limbs and `cnt` ciphertext indices: true = one launch of k_qsum3_int, whose workgroup walks the clients of a group;
// false = k_row3_inner_int<.., false> + k_row3_tail_once.  mode 0 / 1 force a form, anything else chooses: the walk is
// serial over the clients, so it pays only where its tiles * nsel * cnt workgroups fill the resident slots of the chip
// (2 per CU x 256 CUs); profiles/q0_walk_ab.txt has the measured sweep.
constexpr uint32_t Q0_WALK_MIN_GRID = 512;
inline bool q0_walk_fused(uint32_t tiles, uint32_t nsel, uint32_t cnt, int mode) {
    if (mode == 0 || mode == 1) return mode == 1;
    return (uint64_t)tiles * nsel * cnt >= Q0_WALK_MIN_GRID;
}

// How many fp64-class targets of a digit with `n_fp` of them k_icol_conv converts inside the inverse column pass of the
// digit's sources, in a call whose k_icol_conv grid (items x such digits x column tiles) is `grid`.  mode 0..3 forces
// that many (as far as the digit has them); anything else chooses: the largest count up to ICOL_CONV_AUTO_MAX that leaves
// k_conv_col2 an even number of targets (no half-empty last workgroup) -- with the shipped maximum of 1 that is the odd
// target of a digit with an odd count -- and none where the grid would not fill the chip: a workgroup walks the digit's
// sources one after the other, like the client walk of q0_walk_fused (profiles/icol_conv_ab.txt).
constexpr uint32_t ICOL_CONV_MAX = 3, ICOL_CONV_AUTO_MAX = 1, ICOL_CONV_MIN_GRID = 2048;  // two and three targets measured no gain
inline uint32_t icol_conv_targets(uint32_t n_fp, uint64_t grid, int mode) {
    if (mode >= 0 && mode <= (int)ICOL_CONV_MAX) return (uint32_t)mode < n_fp ? (uint32_t)mode : n_fp;
    if (grid < ICOL_CONV_MIN_GRID) return 0;
    for (uint32_t nt = ICOL_CONV_AUTO_MAX < n_fp ? ICOL_CONV_AUTO_MAX : n_fp; nt >= 1; --nt)
        if ((n_fp - nt) % 2 == 0) return nt;
    return 0;
}

// The form poly_tensor takes for a (B, G) plan: true = k_poly_tensor, false = the composition.  mode 0 / 1 force a form,
// anything else chooses: the kernel for every plan -- it is 4.6 x to 6.3 x faster on each measured (B, G), which are all
// three instances with G = 2, 3, 4 and 8, the largest plan (8, 8) included (profiles/poly_ab.txt); a plan that measures
// otherwise gets its exception here.
inline bool poly_tensor_fused(uint32_t /*B*/, uint32_t /*G*/, int mode) {
    return mode != 0;
}

// The form a Chebyshev ladder step takes before its relinearisation: true = k_cheb_tensor, false = the composition.  mode
// 0 / 1 force a form, anything else chooses: the kernel on all four instances (square or general, constant or ciphertext
// term) -- it reads each operand once where it is and writes each output once, where the composition adds prefix copies
// and two or three more streaming passes (profiles/cheb_ab.txt); an instance that measures otherwise gets its exception
// here.
inline bool cheb_step_fused(bool /*square*/, bool /*term*/, int mode) {
    return mode != 0;
}

struct PolyOpnd;  // poly_kernels.hpp

class Engine {
public:
    explicit Engine(const ParamSet &ps, int device);
    ~Engine();
    Engine(const Engine &) = delete;
    Engine &operator=(const Engine &) = delete;

    const ParamSet &params() const { return ps_; }
    bool has_device() const { return device_ >= 0; }
    int device() const { return device_; }
    void set_stream(hipStream_t s) { stream_ = s; }
    hipStream_t stream() const { return stream_; }
    void sync();

    void *dev_alloc(size_t bytes);
    void dev_free(void *p);
    void upload(void *d, const void *h, size_t bytes);
    void download(void *h, const void *d, size_t bytes);
    // I/O pipeline of the hosts: pinned host buffers and copies on the context's two copy streams (one per direction,
    // PCIe is full duplex), ordered against the compute stream by fences; every copy gets a ticket the host can poll
    void *host_alloc(size_t bytes);
    void host_free(void *p);
    uint64_t upload_async(void *d, const void *h, size_t bytes);
    uint64_t download_async(void *h, const void *d, size_t bytes);
    bool copy_done(uint64_t ticket);
    void copy_wait(uint64_t ticket);
    void fence_uploads();   // compute stream: wait for every upload enqueued so far
    void fence_compute();   // download stream: wait for all compute enqueued so far
    // residues of ciphertexts u64[n_ct][2][nl][N] that are not below their limb's modulus (0 = all canonical); synchronous
    uint64_t count_noncanonical(const u64 *ct, uint32_t n_ct, uint32_t nl);

    // transforms, in place on u64[n_polys][ext][N]; ext = nl (+K when with_p)
    void ntt_forward(u64 *d, uint32_t n_polys, uint32_t nl, bool with_p);
    void ntt_inverse(u64 *d, uint32_t n_polys, uint32_t nl, bool with_p);

    void eval_add(const u64 *a, const u64 *b, u64 *out, uint32_t n_ct, uint32_t nl);
    void eval_sum(const u64 *in, u64 *out, uint32_t n_clients, uint32_t n_ct, uint32_t nl);
    void rescale(const u64 *in, u64 *out, uint32_t n_ct, uint32_t nl, const std::vector<u64> *factors);
    void mult_const(u64 *ct, uint32_t n_ct, uint32_t nl, const std::vector<u64> &factors);
    // EvalMult(ct, plaintext): pt u64[n_pt][nl][N] EVALUATION, canonical (encode's output); n_pt == n_ct or 1 (shared)
    //   mult_plain:         ct[b][k][i] *= pt[b % n_pt][i] in place
    //   mult_plain_rescale: out u64[n_ct][2][nl-1][N] = Rescale(in * pt); in is not modified, out must not overlap it
    void mult_plain(u64 *ct, const u64 *pt, uint32_t n_ct, uint32_t n_pt, uint32_t nl);
    void mult_plain_rescale(const u64 *in, const u64 *pt, u64 *out, uint32_t n_ct, uint32_t n_pt, uint32_t nl);
    void reduce_mod(u64 *ct, uint32_t n_ct, uint32_t nl, uint32_t n_terms);
    // RCCL exchange of the per-GPU partial sums: shard[b] = (sum over ranks of partial_r[rank * n_ct_shard + b]) mod q,
    // partial u64[n_ranks * n_ct_shard][2][nl][N] on every rank, shard u64[n_ct_shard][2][nl][N] (comm: ncclComm_t)
    void reduce_scatter_sum_mod(void *comm, const u64 *partial, u64 *shard, uint32_t n_ct_shard, uint32_t nl,
                                uint32_t n_ranks);

    // out[b] = sum over clients of ReEncrypt(cts[c][b], evks[c]); cts [C][n_ct][2][nl][N], evks [C][beta][2][D][N]
    void reencrypt_sum(const u64 *cts, const u64 *evks, u64 *out, uint32_t n_clients, uint32_t n_ct, uint32_t nl);
    // weighted aggregation, M_k = trunc(w[k] * sf(sf_level) + 0.5) reduced per limb (w: HOST doubles, read before return):
    //   scale_evk:      out[k] = M_k * in[k] on all D limbs; eval keys [n_keys][beta][2][D][N]; out must not overlap in
    //   reencrypt_wsum: out[b] = sum_c ReEncrypt((M_c * cts[c][b].c0, cts[c][b].c1), evks_scaled[c]), layouts of reencrypt_sum
    //   eval_wsum:      out[b] = sum_k M_k * in[k][b]; first_is_sum: term 0 enters as it is
    void scale_evk(const u64 *in, u64 *out, uint32_t n_keys, const double *w, uint32_t sf_level);
    void reencrypt_wsum(const u64 *cts, const u64 *evks_scaled, u64 *out, uint32_t n_clients, uint32_t n_ct, uint32_t nl,
                        const double *w, uint32_t sf_level);
    void eval_wsum(const u64 *in, u64 *out, uint32_t n_terms, uint32_t n_ct, uint32_t nl, const double *w, uint32_t sf_level,
                   bool first_is_sum);
    // out[k][b] = ReEncrypt(ct[b], evks[k]): ModUp (and, on the fused path, the digits' row transforms) once per
    // ciphertext; ct [n_ct][2][nl][N] read-only, evks [n_keys][beta][2][D][N], out [n_keys][n_ct][2][nl][N]
    void reencrypt_fanout(const u64 *ct, const u64 *evks, u64 *out, uint32_t n_keys, uint32_t n_ct, uint32_t nl);
    // compact forms for ciphertexts that will only be decrypted; both read the first nl_out + 1 limbs of in / ct
    // u64[n_ct][2][nl_in][N] in place (a lower level of the same ciphertext) and write nl_out limbs:
    //   compress:                 out[b]    = Rescale(prefix(in[b]))                       out [n_ct][2][nl_out][N]
    //   reencrypt_fanout_compact: out[k][b] = Rescale(ReEncrypt(prefix(ct[b]), evks[k]))  out [n_keys][n_ct][2][nl_out][N]
    void compress(const u64 *in, u64 *out, uint32_t n_ct, uint32_t nl_in, uint32_t nl_out);
    void reencrypt_fanout_compact(const u64 *ct, const u64 *evks, u64 *out, uint32_t n_keys, uint32_t n_ct, uint32_t nl_in,
                                  uint32_t nl_out);
    void modup(const u64 *c1, u64 *digits, uint32_t n, uint32_t nl);
    void moddown(const u64 *in, u64 *out, uint32_t n, uint32_t nl);
    // accumulate: out[b] += ReEncrypt(ct[b]) (coefficient-wise, mod q) -- the fold into a running aggregate
    void reencrypt(const u64 *ct, const u64 *evk, u64 *out, uint32_t n_ct, uint32_t nl, bool accumulate = false);

    void keygen(const int8_t *s, const u64 *a, const int32_t *e, u64 *pk, u64 *sk);
    void rekeygen(const int8_t *s_old, const u64 *pk_new, const int8_t *u, const int32_t *e0,
                  const int32_t *e1, u64 *evk);
    void encrypt(const u64 *pk, const u64 *pt, const int8_t *v, const int32_t *e0, const int32_t *e1,
                 u64 *ct, uint32_t n_ct, uint32_t nl);
    // re-randomisation before a key switch: out = ct + Enc_pk(0; v, e0, e1) on the first nl limbs of ct
    // u64[n_ct][2][nl_in][N]; v int8[n_ct][N], e0 / e1 int64[n_ct][N] (|e| < 2^62); out u64[n_ct][2][nl][N], may be ct
    // when nl_in == nl
    void rerandomize(const u64 *ct, const u64 *pk, const int8_t *v, const int64_t *e0, const int64_t *e1, u64 *out,
                     uint32_t n_ct, uint32_t nl_in, uint32_t nl);
    // threshold decryption.  keygen_join: pk = (pk_prev[0] + e - pk_prev[1] * s, pk_prev[1]), sk as keygen.
    // partial_decrypt: share[t] = INTT(c1 * sk (+ c0 when lead)) + e[t] on the first nl limbs of ct u64[n_ct][2][nl_in][N];
    // e int64[n_ct][N] (|e| < 2^62); share u64[n_ct][nl][N], COEFFICIENT, canonical.  fuse_shares: m = sum over
    // shares u64[n_parties][n_ct][nl][N]; m may be shares[0]
    void keygen_join(const u64 *pk_prev, const int8_t *s, const int32_t *e, u64 *pk, u64 *sk);
    void partial_decrypt(const u64 *ct, const u64 *sk, const int64_t *e, u64 *share, uint32_t n_ct, uint32_t nl_in,
                         uint32_t nl, bool lead);
    void fuse_shares(const u64 *shares, u64 *m, uint32_t n_parties, uint32_t n_ct, uint32_t nl);
    // collective public-key switch, one party's share: share[t] = (c1 * sk (+ c0 when lead) + pk0 * NTT(v) + NTT(e0),
    // pk1 * NTT(v) + NTT(e1)) on the first nl limbs of ct u64[n_ct][2][nl_in][N]; pk the RECIPIENT's; v, e0, e1 as
    // rerandomize; share u64[n_ct][2][nl][N], EVALUATION, canonical, never ct.  The parties' shares sum to a ciphertext
    // under pk (eval_sum)
    void switch_share(const u64 *ct, const u64 *sk, const u64 *pk, const int8_t *v, const int64_t *e0, const int64_t *e1,
                      u64 *share, uint32_t n_ct, uint32_t nl_in, uint32_t nl, bool lead);
    // t-of-n sharing of a key.  share_key: shares u64[n_parties][nl][N], share p = sk + sum_{k=1}^{t-1} r_k (p+1)^k mod q_i
    // with r_k = sample_uniform(1 poly, nl, Q only) of stream (key32, sid0 + k - 1), never written to memory.
    // combine_key_shares: out u64[nl][N] = sum_{j<m} w[j][i] * in[j][i] mod q_i; w HOST u64[m][nl], canonical; out may be in[0]
    void share_key(const u64 *sk, u64 *shares, uint32_t nl, uint32_t n_parties, uint32_t threshold, const uint8_t *key32,
                   uint32_t sid0);
    void combine_key_shares(const u64 *in, const u64 *w, u64 *out, uint32_t m, uint32_t nl);
    // slot rotations ("rotations and slot sums"; index arithmetic: galois.hpp).  g: odd, below 2N.
    //   automorphism:        out[p][i] = sigma_g(in[p][i]) on u64[n_polys][nl][N], EVALUATION; out never overlaps in
    //   automorphism_secret: out int8[N] = sigma_g(s), COEFFICIENT, signed
    //   galois_keygen:       evk = rekeygen(sigma_g(s), pk, u, e0, e1)
    //   rotate:              out[b] = ReEncrypt(sigma_g(ct[b]), evk)
    //   slot_sum:            out = ct, then out += Rotate(out, 5^(2^k)) with evks[k] for k = 0 .. log2(span) - 1
    void automorphism(const u64 *in, u64 *out, uint32_t n_polys, uint32_t nl, uint32_t g);
    void automorphism_secret(const int8_t *s, int8_t *out, uint32_t g);
    void galois_keygen(const int8_t *s, const u64 *pk, const int8_t *u, const int32_t *e0, const int32_t *e1, uint32_t g,
                       u64 *evk);
    void rotate(const u64 *ct, const u64 *evk, u64 *out, uint32_t n_ct, uint32_t nl, uint32_t g);
    void slot_sum(const u64 *ct, const u64 *evks, u64 *out, uint32_t n_ct, uint32_t nl, uint32_t span);
    // linear transforms by diagonals, double hoisted ("linear transforms"; kernel: lintrans_kernels.hpp)
    //   encode_ext:       encode over the extended basis: pt u64[n][nl+K][N] EVALUATION, Q limbs then P limbs
    //   linear_transform: out[b] = (ModDown(A_b), ModDown(A_a)) with A of lintrans_kernels.hpp; evks u64[n_rot][beta][2][D][N],
    //                     pts u64[n_rot][nl+K][N] shared by the ciphertexts, h_g: n_rot Galois elements on the HOST (1: no
    //                     rotation, its key is never read); one ModUp per ciphertext, one ModDown per component
    void encode_ext(const double *vals, u64 *pt, uint32_t n, uint32_t nl, double scale);
    void linear_transform(const u64 *ct, const u64 *evks, const u64 *pts, const uint32_t *h_g, u64 *out, uint32_t n_rot,
                          uint32_t n_ct, uint32_t nl);
    //   linear_transform_bsgs: the baby-step giant-step form (kernels: bsgs_kernels.hpp; definition: include/mkckks.h):
    //                     bkeys u64[n1][beta][2][D][N], gkeys u64[n2][..], pts u64[n2][n1][nl+K][N], h_gb / h_gg / h_present
    //                     on the HOST; per chunk one ModUp of c1, the babies, the inner sums, one ModDown and one ModUp over
    //                     all keyed giants, the giants, one ModDown per component
    void linear_transform_bsgs(const u64 *ct, const u64 *bkeys, const uint32_t *h_gb, uint32_t n1, const u64 *gkeys,
                               const uint32_t *h_gg, uint32_t n2, const u64 *pts, const uint8_t *h_present, u64 *out,
                               uint32_t n_ct, uint32_t nl);
    // ciphertext products ("ciphertext products"; kernel: tensor_kernels.hpp)
    //   relin_keygen: evk = rekeygen with NTT(s_old) replaced by NTT(s)^2 (the re-encryption key from s^2 to s)
    //   tensor_sum:   out3[b] = sum_t (a0 b0, a0 b1 + a1 b0, a1 b1); a, b u64[n_terms][n_ct][2][nl][N], out3 u64[n_ct][3][nl][N]
    //   relinearize:  out[b] = (d0, d1) + KeySwitch(d2, rlk); out never overlaps in3
    //   mult_relin:   relinearize(tensor_sum(a, b, 1 term)); out may be a or b
    void relin_keygen(const int8_t *s, const u64 *pk, const int8_t *u, const int32_t *e0, const int32_t *e1, u64 *evk);
    void tensor_sum(const u64 *a, const u64 *b, u64 *out3, uint32_t n_terms, uint32_t n_ct, uint32_t nl);
    void relinearize(const u64 *in3, const u64 *rlk, u64 *out, uint32_t n_ct, uint32_t nl);
    void mult_relin(const u64 *a, const u64 *b, const u64 *rlk, u64 *out, uint32_t n_ct, uint32_t nl);
    // polynomial evaluation ("polynomial evaluation"; kernel: poly_kernels.hpp; plan, scales and constants:
    // ParamSet::poly_plan / power_ladder / poly_weights / poly_constants)
    //   powers:      out = z^1 .. z^n_pow, power k packed u64[n_ct][2][nl_k][N] behind power k - 1; z^k =
    //                rescale(mult_relin(z^i, prefix(z^j, nl_i))), i = ceil(k / 2), j = k - i
    //   poly_tensor: the fused outer sum over caller-supplied babies and giants (packed like the output of powers) and
    //                weights w HOST double[G][B]; out3 u64[n_ct][3][nl_T][N]
    //   poly_eval:   powers of x up to y = x^B, powers of y, poly_tensor, relinearize, rescale twice; chunked
    void powers(const u64 *z, const u64 *rlk, u64 *out, uint32_t n_ct, uint32_t nl, uint32_t n_pow);
    void poly_tensor(const u64 *baby, const uint32_t *baby_nl, const u64 *giant, const uint32_t *giant_nl, const double *w,
                     u64 *out3, uint32_t B, uint32_t G, uint32_t n_ct, uint32_t nl_T);
    void poly_eval(const u64 *ct, const u64 *rlk, const double *coef, uint32_t degree, u64 *out, uint32_t n_ct, uint32_t nl,
                   double scale_in);
    // Chebyshev series ("Chebyshev series"; kernels: cheb_kernels.hpp; weights: ParamSet::cheb_weights)
    //   affine:      out = rint(w_mul) * in + (rint(w_add), 0) as exact integers mod q_t; no rescale; out may be in
    //   cheb_tensor: out3 = (2 a0 b0 - M t0, 2 (a0 b1 + a1 b0) - M t1, 2 a1 b1), M = rint(w); a, b, t at nl_a, nl_b, nl_t >= nl
    //                limbs, read in place; t == nullptr is the constant 1; a == b squares
    //   cheb_ladder: out = T_1 .. T_n of u, packed like the output of powers; T_k = rescale(relinearize(cheb_tensor(T_i, T_j,
    //                T_{i-j}))) with i = ceil(k / 2), j = k - i, weight S_i * S_j / S_{i-j}
    //   cheb_eval:   the affine map of [a, b] onto [-1, 1] and its rescale (skipped for (-1, 1)), the ladder on u up to T_B,
    //                the ladder on T_B up to G - 1, cheb_weights, the outer sum of poly_eval, relinearize, rescale twice
    void affine(const u64 *in, u64 *out, uint32_t n_ct, uint32_t nl, double w_mul, double w_add);
    void cheb_tensor(const u64 *a, uint32_t nl_a, const u64 *b, uint32_t nl_b, const u64 *t, uint32_t nl_t, double w, u64 *out3,
                     uint32_t n_ct, uint32_t nl);
    void cheb_ladder(const u64 *u, const u64 *rlk, u64 *out, uint32_t n_ct, uint32_t nl, uint32_t n, double scale_in);
    void cheb_eval(const u64 *ct, const u64 *rlk, const double *coef, uint32_t degree, double a, double b, u64 *out,
                   uint32_t n_ct, uint32_t nl, double scale_in);
    // collective evaluation keys of a joint key ("collective evaluation keys"; kernels: relshare_kernels.hpp)
    //   evk_sum:     out[k] = sum_p in[p][k] on all D limbs; in u64[n_parties][n_keys][beta][2][D][N]; out may be in[0]
    //   relin_share: share[j][c] = key1[j][c] * sk + NTT(e_c[j]) on all D limbs; key1, share u64[beta][2][D][N], sk u64[D][N],
    //                e0 / e1 int32[beta][N] COEFFICIENT; share may be key1
    void evk_sum(const u64 *in, u64 *out, uint32_t n_parties, uint32_t n_keys);
    void relin_share(const u64 *key1, const u64 *sk, const int32_t *e0, const int32_t *e1, u64 *share);
    void lift_ntt(const double *coef, u64 *out, uint32_t n, uint32_t nl);
    void decrypt(const u64 *ct, const u64 *sk, u64 *m, uint32_t n_ct, uint32_t nl);
    // counter-based samplers (ChaCha20 block function under a 256-bit key): element i of stream sid is a pure
    // function of (key, sid, i), independent of launch shape
    void sample_ternary(int8_t *out, size_t count, const uint8_t *key32, uint32_t sid);
    void sample_gauss(int32_t *out, size_t count, double sigma, const uint8_t *key32, uint32_t sid);
    void sample_gauss_wide(int64_t *out, size_t count, double sigma, const uint8_t *key32, uint32_t sid);  // rint(sigma z)
    void sample_uniform(u64 *out, uint32_t items, uint32_t nl, bool with_p, const uint8_t *key32, uint32_t sid);
    void chacha_block(uint32_t *d_out16, const uint8_t *key32, uint32_t counter, const uint32_t nonce[3]);  // KAT hook
    // seeded ciphertexts: a = sample_uniform(1 poly, nl, Q only) of stream (key, sid).  encrypt_seeded: item t of
    // pt u64[n_ct][nl][N] (EVALUATION), e int32[n_ct][N] (COEFFICIENT) -> c0 = pt + NTT(e) - a*s with a of stream
    // (key32, sid0 + t), sk u64[.][N] (first nl limbs).  expand_seeded: c1 of ct u64[n_ct][2][nl][N] in place from
    // the host arrays keys32 [n_ct][32] and sids [n_ct] (read before return)
    void encrypt_seeded(const u64 *sk, const u64 *pt, const int32_t *e, u64 *c0, uint32_t n_ct, uint32_t nl,
                        const uint8_t *key32, uint32_t sid0);
    void expand_seeded(u64 *ct, uint32_t n_ct, uint32_t nl, const uint8_t *keys32, const uint32_t *sids);
    // CKKS canonical embedding on the device: vals [n][N/2] reals <-> plaintexts / decrypted polynomials
    void encode(const double *vals, u64 *pt, uint32_t n, uint32_t nl, double scale);
    void decode(const u64 *m, double *vals, uint32_t n, uint32_t nl, double scale);
    // decode with upstream Decode's noise estimate + flooding (normals: ChaCha20 stream sid under key32); downloads the
    // per-item estimates once, which synchronises the stream; h_log2 (nullable) [n] gets log2 sigma_hat per item.
    // Throws PrecisionError naming the first failing item after all outputs are written.
    void decode_flood(const u64 *m, double *vals, uint32_t n, uint32_t nl, double scale, const uint8_t *key32,
                      uint32_t sid, double *h_log2);

    void host_twiddles(uint32_t limb, bool inverse, std::vector<u64> &out) const;
    // diagnostics: run primitive `op` (arith_probe_kernels.hpp; MKCKKS_OP_* of mkckks.h) once per element on operand
    // planes in u64[n_in][count] -> out u64[n_out][count], modulus q (odd, 2^17 < q < 2^60, need not belong to the
    // context).  Device context: device pointers, device form, on the stream.  device = -1: host pointers, host form;
    // device-only ops throw NoDevice
    void debug_arith(uint32_t op, u64 q, const u64 *in, u64 *out, size_t count);
    // diagnostic builds (-DMK_STAMP=1, MKCKKS_STAMPS=1): copy one region of in-kernel phase stamps (2^20 words) to the
    // host and clear it; 0 words in a product build
    size_t debug_stamps(unsigned long long *h_out, uint32_t region);

private:
    void need_device() const;
    void check_nl(uint32_t nl) const;
    u64 *workspace(size_t words);  // grow-only scratch arena (stream-ordered reuse)
    u64 *chunk_buffer(size_t words);  // a second grow-only buffer: a chunk of ciphertexts that feeds reencrypt_chunk
    void launch_automorph(const u64 *in, u64 *out, size_t rows, uint32_t g);
    u64 *rekey_workspace();  // the key generators' workspace; the source key's transform u64[D][N] is its head
    void rekeygen_from(const u64 *pk_new, const int8_t *u, const int32_t *e0, const int32_t *e1, u64 *evk);
    void launch_tensor(const u64 *a, const u64 *b, size_t term_stride, uint32_t n_terms, u64 *o01, size_t o01_stride, u64 *o2,
                       size_t o2_stride, uint32_t cnt, uint32_t nl);
    void relin_chunk(const u64 *d2, size_t d2_stride, const u64 *rlk, u64 *out, uint32_t cnt, uint32_t nl);
    u64 *poly_buffer(size_t words);  // a third grow-only buffer: the powers and intermediates of a chunk (poly_eval)
    // pw[k] = z^k for k = 2 .. n_pow from pw[1] (1-based; nlk[k] its limbs); scratch: 2 * cnt * 2 * nlk[1] * N words
    void power_ladder_core(u64 *const *pw, const uint32_t *nlk, const u64 *rlk, uint32_t cnt, uint32_t n_pow, u64 *scratch);
    const u64 *poly_table(const double *w, uint32_t B, uint32_t G, uint32_t nl_T);
    size_t poly_tensor_scratch(uint32_t B, uint32_t G, uint32_t cnt, uint32_t nl_T) const;
    void poly_tensor_core(const PolyOpnd *baby, const PolyOpnd *giant, const u64 *table, u64 *out3, uint32_t B, uint32_t G,
                          uint32_t cnt, uint32_t nl_T, u64 *scratch);
    // Chebyshev ladder: the table of a step's weight (cheb_table), the step before its relinearisation (cheb_step_core;
    // scratch: cheb_step_scratch words, none for the kernel) and the ladder on one chunk (sk[k]: the scale of T_k; scratch:
    // cnt * 2 * nlk[1] * N words for the product + cheb_step_scratch(cnt, nlk[1]))
    const u64 *cache_table(const std::string &key, const std::vector<u64> &t);
    const u64 *cheb_table(double w, uint32_t nl);
    size_t cheb_step_scratch(uint32_t cnt, uint32_t nl) const;
    void cheb_step_core(const u64 *a, uint32_t nl_a, const u64 *b, uint32_t nl_b, const u64 *t, uint32_t nl_t, const u64 *table,
                        u64 *o01, size_t o01_stride, u64 *o2, size_t o2_stride, uint32_t cnt, uint32_t nl, u64 *scratch);
    void cheb_ladder_core(u64 *const *pw, const uint32_t *nlk, const double *sk, const u64 *rlk, uint32_t cnt, uint32_t n,
                          u64 *scratch);
    void affine_core(const u64 *in, u64 *out, uint32_t cnt, uint32_t nl, double w_mul, double w_add);
    // p_scaled: the P targets' constants carry ModDown's scale (ParamSet::modup_table_pscaled; the merged n-client flow)
    const DevConv &modup_conv(uint32_t nl, uint32_t part, bool p_scaled = false);
    const DevConv &moddown_conv(uint32_t nl);
    const u64 *limb_vector(const std::string &key, const std::vector<u64> &vals);  // cached small device arrays
    const u64 *garner_table(uint32_t nl);  // CRT interpolation constants of the first nl limbs (decode)
    void ntt_launch(u64 *d, uint32_t n_polys, uint32_t nl, uint32_t ext, bool inverse, const u64 *scale,
                    const u64 *scale_sh);
    void reencrypt_chunk(const u64 *ct, const u64 *evk, u64 *out, uint32_t n_ct, uint32_t nl, bool accumulate);
    const u64 *folded_scale(uint32_t nl);
    const u64 *p_inverse(uint32_t nl);
    void modup_core(const u64 *c1, size_t c1_stride, u64 *coef, u64 *dig, uint32_t cnt, uint32_t nl,
                    bool rows_int_only = false, uint32_t in_group = 0, size_t in_gstride = 0, bool p_scaled = false);
    bool qsum_ok(uint32_t nl) const;
    // wt: weight table of the clients (weighted instance of the two Q-limb kernels), nullptr: the plain sum
    void reencrypt_sum_merged(const u64 *cts, const u64 *evks, u64 *out, uint32_t n_clients, uint32_t n_ct, uint32_t nl,
                              const u64 *wt);
    const u64 *weight_table(const double *w, uint32_t n, uint32_t sf_level);
    const u64 *p_doubles();
    // returns true when the inverse ROW pass of the P limbs was done on the fly into `pc` (ModDown then starts with
    // the inverse column pass)
    bool keyswitch_digits(const u64 *c1, size_t ct_stride, const u64 *evk, u64 *coef, u64 *dig, u64 *til, u64 *pc,
                          uint32_t cnt, uint32_t nl);
    void moddown_core(const u64 *til, u64 *pc, u64 *conv, u64 *out, size_t out_stride, const u64 *add,
                      size_t add_stride, uint32_t cnt, uint32_t nl, bool accumulate, bool p_rows_done = false,
                      uint32_t group = 0, size_t out_gstride = 0);
    void inner_product_all(const u64 *c1, size_t ct_stride, const u64 *evk, const u64 *dig, u64 *til, uint32_t cnt,
                           uint32_t nl, unsigned long long mask);
    bool fanout_fused(uint32_t nl) const;
    // fan-out over ciphertexts whose limbs are in_limbs * N words apart (their first nl are used); compact: the closing
    // rescale to nl - 1 limbs follows the key switch of every group
    void fanout_core(const u64 *ct, uint32_t in_limbs, const u64 *evks, u64 *out, uint32_t n_keys, uint32_t n_ct, uint32_t nl,
                     bool compact);
    const u64 *rescale_consts(uint32_t nl, const std::vector<u64> *factors);
    // ModReduceInternalInPlace on `polys` polynomials of nl limbs, in_limbs * N words apart; out polynomial p (nl - 1
    // limbs) at out + (p / group) * out_gstride + (p % group) * (nl - 1) * N (group 0: p * (nl - 1) * N).
    // d_last [polys][N] and d_tmp [polys][nl - 1][N] are scratch
    void rescale_core(const u64 *in, uint32_t in_limbs, u64 *out, uint32_t polys, uint32_t nl, const u64 *d_c, u64 *d_last,
                      u64 *d_tmp, uint32_t group, size_t out_gstride);
    void moddown_convert(const u64 *til, u64 *pc, u64 *conv, uint32_t cnt, uint32_t nl, bool rows_done);
    int conv_src_mode(const DevConv &cv) const;

    ParamSet ps_;
    int device_ = -1;
    hipStream_t stream_ = nullptr;
    NttTables tabs_{};
    LimbConst *d_limb_ = nullptr;
    u64 *d_tw_ = nullptr, *d_tw_sh_ = nullptr, *d_itw_ = nullptr, *d_itw_sh_ = nullptr;
    unsigned long long *d_stamps_ = nullptr;
    u64 *d_twb_ = nullptr, *d_itwb_ = nullptr;  // packed round-B tables of the row kernels (NttTables::twb)
    std::vector<uint8_t> fp_of_;  // per limb id: 1 = fp64 kernel instance
    // copies: tickets count up from 1; ticket t's completion event is ring slot t % COPY_RING
    static constexpr uint32_t COPY_RING = 64;
    uint64_t enqueue_copy(void *dst, const void *src, size_t bytes, bool up);
    void copy_streams();
    hipStream_t up_stream_ = nullptr, down_stream_ = nullptr;
    hipEvent_t copy_ev_[COPY_RING] = {};
    hipEvent_t ev_fence_ = nullptr;
    uint64_t next_ticket_ = 1, done_ticket_ = 0;  // every ticket <= done_ticket_ is known complete
    bool skip_rows_ = false;  // modup_core: leave the row pass of the converted digits to the fused kernels
    uint32_t *d_rot_ = nullptr;
    void *d_ksi_ = nullptr;
    u64 *ws_ = nullptr;
    size_t ws_words_ = 0;
    Knobs knobs_;
    std::map<std::pair<uint32_t, uint32_t>, DevConv> modup_cache_, modup_ps_cache_;  // plain / P-scaled tables
    std::map<uint32_t, DevConv> moddown_cache_;
    std::map<std::string, u64 *> vec_cache_;
    std::map<std::string, u64 *> wt_cache_;  // weight_table
    u64 *wtmp_ = nullptr;                    // chunk_buffer: a chunk with c0 scaled (reencrypt_wsum), permuted (slot_sum), or d2 (mult_relin)
    size_t wtmp_words_ = 0;
    u64 *poly_buf_ = nullptr;  // poly_buffer
    size_t poly_buf_words_ = 0;
    int8_t *d_gal_s_ = nullptr;  // galois_keygen: sigma_g(s)
    uint32_t *d_lt_g_ = nullptr;  // linear_transform: the call's Galois elements (grow-only)
    size_t lt_g_cap_ = 0;
    std::vector<void *> owned_;
};

}  // namespace mk
