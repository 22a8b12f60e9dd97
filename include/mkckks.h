/*
 * mkckks.h -- C-ABI of libmkckks_hip.so, the MI355X (gfx950) engine for the
 * multikey-CKKS PRE + aggregation hot path of CDACHPCIE25/PPQSFLHE.
 *
 * The reference has no FFI/plugin layer: its hot path is eight C++ main()s that
 * call OpenFHE's CryptoContext.  The drop-in boundary is
 * therefore (1) the CLI/JSON contract, re-created by the C++ hosts under
 * ppqsflhe_amd/host/, and (2) this library, whose entry points replace the
 * OpenFHE calls those mains make.  Each entry point cites the reference
 * call site(s) it stands in for (paths relative to /root/reference).
 *
 * Conventions
 *  - every function returns 0 on success, a negative MKCKKS_E_* code otherwise,
 *    never throws across the ABI; mkckks_last_error() gives the message of the
 *    calling thread's last failure.
 *  - "d_" pointers are DEVICE pointers (HBM) owned by the caller (hipMalloc,
 *    torch tensor data_ptr(), or mkckks_dev_alloc); "h_" pointers are host.
 *  - all work is enqueued on the context's HIP stream (mkckks_set_stream) and is
 *    asynchronous w.r.t. the host unless stated; a context is re-entrant per
 *    (context, stream) pair, not across threads sharing one context.
 *  - polynomials are limb-major uint64: a polynomial over the first nl Q-limbs
 *    is u64[nl][N]; a ciphertext is u64[2][nl][N] (c0 then c1); a batch is
 *    u64[n_ct][2][nl][N]; over QP the limb order is q_0..q_{L-1},p_0..p_{K-1};
 *    a public key is u64[2][D][N] (b then a); an eval (re-encryption) key is
 *    u64[beta][2][D][N] (digit j: b_j then a_j).  EVALUATION format = negacyclic
 *    NTT, natural-order input, bit-reversed output, psi = minimal primitive
 *    2N-th root (what OpenFHE serialises with "f":0).
 */
#ifndef MKCKKS_H
#define MKCKKS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MKCKKS_OK 0
#define MKCKKS_E_INVALID (-1)   /* bad argument / unsupported parameter set   */
#define MKCKKS_E_NODEVICE (-2)  /* no HIP device, or host-only context used   */
#define MKCKKS_E_HIP (-3)       /* HIP runtime error (message has the detail) */
#define MKCKKS_E_NOMEM (-4)
#define MKCKKS_E_INTERNAL (-5)
#define MKCKKS_E_PRECISION (-6)  /* decode: approximation error too high (log2 sigma > scaling_bits - 5) */

typedef struct mkckks_ctx mkckks_ctx;

/* server/config/config_cc.json:2-5 knobs + the ones genCC.cpp leaves at
 * OpenFHE defaults (first mod 60, aux 60, extra 20: CC.json 'ab','eb'). */
typedef struct mkckks_params {
    uint32_t log_n;        /* ring dimension N = 2^log_n (CC.json "rd")            */
    uint32_t mult_depth;   /* MultiplicativeDepth; #Q limbs L = mult_depth + 2     */
    uint32_t scaling_bits; /* ScalingModSize                                       */
    uint32_t first_bits;   /* FirstModSize (60)                                    */
    uint32_t dnum;         /* NumLargeDigits of HYBRID key switching ("dnum")      */
    uint32_t aux_bits;     /* auxiliary prime size ("ab", 60)                      */
    uint32_t extra_bits;   /* FLEXIBLEAUTOEXT extra limb size ("eb", 20)           */
    int32_t device;        /* HIP device ordinal; -1 = host-only (tables, no GPU)  */
} mkckks_params;

typedef struct mkckks_info {
    uint32_t ring_dim, num_q, num_p, alpha, beta, slots;
} mkckks_info;

const char *mkckks_last_error(void);
const char *mkckks_version(void);

/* ---- context -------------------------------------------------------------
 * replaces GenCryptoContext(params)+Enable(...) (server/src/genCC.cpp:68-76)
 * and Serial::DeserializeFromFile(cc) (server/src/changeCipherDomain.cpp:33,
 * aggregateEncryptedWeights.cpp:47 and the client mains): builds Q, P, roots,
 * twiddles and all CRT tables and keeps them resident in HBM.
 * Accepted: log_n 8..17, mult_depth 1..30, 20 <= scaling_bits < first_bits <= 60,
 * aux_bits 30..60, extra_bits 18..30, digit size alpha and #special primes K <= 8.
 * Refused (-1) inside that range: parameters whose moduli are not pairwise
 * distinct -- the extra limb (first prime = 1 mod 2N above 2^(extra_bits-1)) is
 * placed without regard to the scaling limbs and coincides with one whenever
 * extra_bits = scaling_bits + 1, and where such primes are sparse (seen at log_n >= 15
 * with scaling_bits 20..22 and extra_bits <= 20, e.g. log_n 16, 20, 20); such
 * a basis has no CRT and cannot be rescaled. */
int mkckks_ctx_create(const mkckks_params *p, mkckks_ctx **out);
int mkckks_ctx_destroy(mkckks_ctx *c);
int mkckks_ctx_info(const mkckks_ctx *c, mkckks_info *out);
int mkckks_ctx_moduli(const mkckks_ctx *c, uint64_t *h_out /*D*/);
int mkckks_ctx_roots(const mkckks_ctx *c, uint64_t *h_out /*D*/);
/* arithmetic the device kernels use per limb (diagnostics, bench.py's instruction-issue ceiling): 0 = 64-bit integer
 * with Shoup/Harvey butterflies, 1 = fp64 (moduli below 1.25 * 2^50), 2 = 64-bit integer with pseudo-Mersenne
 * butterflies (q = 2^k - c; OpenFHE's 60-bit primes).  Results are the same bits in every class. */
#define MKCKKS_ARITH_INT 0
#define MKCKKS_ARITH_FP64 1
#define MKCKKS_ARITH_PM 2
int mkckks_ctx_arith(const mkckks_ctx *c, uint8_t *h_out /*D*/);
/* CryptoParametersCKKSRNS::GetScalingFactorReal / RealBig (level = #dropped limbs) */
int mkckks_scaling_factor(const mkckks_ctx *c, uint32_t level, int big, double *out);
/* stream: a hipStream_t passed as void* (NULL = default stream) */
int mkckks_set_stream(mkckks_ctx *c, void *hip_stream);
int mkckks_sync(mkckks_ctx *c);

/* ---- device memory helpers (so hosts need no HIP headers) ---------------- */
int mkckks_dev_alloc(mkckks_ctx *c, size_t bytes, void **d_out);
int mkckks_dev_free(mkckks_ctx *c, void *d_ptr);
int mkckks_upload(mkckks_ctx *c, void *d_dst, const void *h_src, size_t bytes);   /* synchronous */
int mkckks_download(mkckks_ctx *c, void *h_dst, const void *d_src, size_t bytes); /* synchronous */

/* ---- I/O pipeline of the server hosts (new; SURVEY.md 8f row f1: "removes the I/O wall") -----------------------
 * The reference's server moves every ciphertext through the host, one at a time and synchronously, between
 * Base64Decode + Serial::Deserialize and cc->ReEncrypt / cc->EvalAdd (server/src/changeCipherDomain.cpp:61-117,
 * aggregateEncryptedWeights.cpp:18-30,54-119).  Here a host reads ciphertext payloads straight into PINNED buffers
 * (mkckks_host_alloc) and enqueues them on the context's upload stream while it reads the next ones; results leave on
 * a download stream (PCIe is full duplex).  Every copy gets a ticket (counting up from 1): mkckks_copy_done polls it,
 * mkckks_copy_wait blocks on it (and on every earlier copy of the same direction).  Ordering against the compute
 * stream is explicit: mkckks_fence_uploads makes the compute stream wait for every upload enqueued so far,
 * mkckks_fence_compute makes the download stream wait for all compute enqueued so far.  Host buffers of an
 * asynchronous copy must be pinned and stay untouched until the copy's ticket is done.  One host thread drives a
 * context (reader threads only fill pinned buffers).
 * mkckks_count_noncanonical: nothing in a client's file is trusted and the kernels assume canonical residues; counts
 * the residues of d_ct u64[n_ct][2][nl][N] that are not below their limb's modulus (synchronous; 0 = accept). */
int mkckks_host_alloc(mkckks_ctx *c, size_t bytes, void **h_out);
int mkckks_host_free(mkckks_ctx *c, void *h_ptr);
int mkckks_upload_async(mkckks_ctx *c, void *d_dst, const void *h_src_pinned, size_t bytes, uint64_t *ticket_out);
int mkckks_download_async(mkckks_ctx *c, void *h_dst_pinned, const void *d_src, size_t bytes, uint64_t *ticket_out);
int mkckks_copy_done(mkckks_ctx *c, uint64_t ticket, int *done_out);
int mkckks_copy_wait(mkckks_ctx *c, uint64_t ticket);
int mkckks_fence_uploads(mkckks_ctx *c);
int mkckks_fence_compute(mkckks_ctx *c);
int mkckks_count_noncanonical(mkckks_ctx *c, const uint64_t *d_ct, uint32_t n_ct, uint32_t nl, uint64_t *h_count);

/* ---- transforms: DCRTPoly::SetFormat (OpenFHE ChineseRemainderTransformFTT)
 * d_polys is u64[n_polys][nl(+K)][N], transformed in place.  with_p != 0 means
 * each polynomial carries the K P-limbs after its nl Q-limbs. */
int mkckks_ntt_forward_batch(mkckks_ctx *c, uint64_t *d_polys, uint32_t n_polys, uint32_t nl, int with_p);
int mkckks_ntt_inverse_batch(mkckks_ctx *c, uint64_t *d_polys, uint32_t n_polys, uint32_t nl, int with_p);

/* ---- cc->EvalAdd(ct1, ct2)  (aggregateEncryptedWeights.cpp:82,91,106) ---- */
int mkckks_eval_add_batch(mkckks_ctx *c, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out,
                          uint32_t n_ct, uint32_t nl);
/* n-client generalisation of the same loop: d_out[b] = sum_k d_in[k][b], d_in is
 * u64[n_clients][n_ct][2][nl][N]. */
int mkckks_eval_sum_batch(mkckks_ctx *c, const uint64_t *d_in, uint64_t *d_out, uint32_t n_clients,
                          uint32_t n_ct, uint32_t nl);

/* ---- cc->EvalMult(ct, operand) on a noiseScaleDeg-2 ciphertext
 * (aggregateEncryptedWeights.cpp:83,92,107: EvalMult(ct_sum, 0.5)): rescale
 * (drop limb nl-1) then multiply by round(operand * sf(level+1)).
 * in u64[n_ct][2][nl][N] at `level` -> out u64[n_ct][2][nl-1][N]. */
int mkckks_rescale_mult_const_batch(mkckks_ctx *c, const uint64_t *d_in, uint64_t *d_out, uint32_t n_ct,
                                    uint32_t nl, double operand);
/* the two halves on their own (ModReduceInternalInPlace / EvalMultCoreInPlace) */
int mkckks_rescale_batch(mkckks_ctx *c, const uint64_t *d_in, uint64_t *d_out, uint32_t n_ct, uint32_t nl);
int mkckks_mult_const_batch(mkckks_ctx *c, uint64_t *d_ct, uint32_t n_ct, uint32_t nl, double operand);

/* ---- cc->EvalMult(ct, plaintext): per-slot aggregation weights ------------------------------------------------------
 * The reference scales its aggregate by one constant (aggregateEncryptedWeights.cpp:82-83: EvalMult(ct_sum, 0.5)); the
 * same call with an encoded plaintext in place of the constant scales every slot by a factor of its own (the divisor
 * 1 / count_j of a round in which clients cover different coordinates, a per-layer rate, a 0/1 mask).
 * d_pt is u64[n_pt][nl][N]: EVALUATION format, canonical residues, as mkckks_encode_batch writes them.  n_pt is n_ct
 * (plaintext b for ciphertext b) or 1 (one plaintext for all); anything else is MKCKKS_E_INVALID, as are null pointers
 * and nl outside [1, L] ([2, L] for the rescaling call).  A zero n_ct is a no-op; host-only context -> MKCKKS_E_NODEVICE.
 * Order: multiply first, ONE rescale last, as in the weighted aggregation below -- the rescale's rounding error is not
 * multiplied by the 2^p-sized plaintext as it is in OpenFHE's rescale-then-EvalMult.
 * Scale: for a noiseScaleDeg-2 input at level = L - nl encode the factors at sf(level + 1) and call
 * mkckks_mult_plain_rescale_batch -- the result has the limbs, level, scale (S_in / q_{nl-1} * sf(level + 1)) and
 * noiseScaleDeg (2) of mkckks_rescale_mult_const_batch(ct, .); for a noiseScaleDeg-1 input encode at sf(level) and call
 * mkckks_mult_plain_batch alone (the bookkeeping of mkckks_mult_const_batch).
 * Headroom: before the rescale the encrypted coefficients are about S_in * sf * max|factor| * |values|, so
 * log2(S_in * sf * max|factor|) must stay below log2(q_0 ... q_{nl-1}) - 1.  The library cannot check it.
 *
 * (aggregateEncryptedWeights.cpp:82-83) EvalMult(ct, pt) core, in place, no rescale:
 * d_ct[b][k][i][.] = d_ct[b][k][i][.] * d_pt[b % n_pt][i][.] mod q_i   (k = 0, 1; i < nl). */
int mkckks_mult_plain_batch(mkckks_ctx *c, uint64_t *d_ct, const uint64_t *d_pt, uint32_t n_ct, uint32_t n_pt, uint32_t nl);
/* (aggregateEncryptedWeights.cpp:82-83) Rescale of that product: d_in u64[n_ct][2][nl][N] -> d_out u64[n_ct][2][nl-1][N].
 * DEFINED bit for bit as the pointwise product of the canonical residues mod q_i on both components followed by
 * mkckks_rescale_batch (DropLastElementAndScale); where the rescale runs on the fused kernels the product is formed
 * inside its two row passes and never reaches memory (MKCKKS_PLAIN_FUSED=0 forces the composition, =1 the fused form
 * wherever it exists).  d_in is not modified.  As with mkckks_rescale_batch the output's polynomials are nl-1 limbs
 * apart and the input's nl, so the two cannot share memory: d_out overlapping d_in is MKCKKS_E_INVALID here. */
int mkckks_mult_plain_rescale_batch(mkckks_ctx *c, const uint64_t *d_in, const uint64_t *d_pt, uint64_t *d_out, uint32_t n_ct,
                                    uint32_t n_pt, uint32_t nl);

/* ---- cc->ReEncrypt(ct, reKey)  (changeCipherDomain.cpp:74,89,105) --------
 * INDCPA proxy re-encryption (the HRA-secure form: mkckks_rerandomize_batch first) = hybrid key switch of c1 with the
 * eval key:
 * out = (c0 + <d,b>/P, <d,a>/P).  d_evk is u64[beta][2][D][N] (full level);
 * ciphertexts have nl <= L limbs; in/out may alias. */
int mkckks_reencrypt_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_evk, uint64_t *d_out,
                           uint32_t n_ct, uint32_t nl);
/* the same, folded into a running aggregate: d_acc[b] = d_acc[b] + ReEncrypt(d_ct[b]) coefficient-wise mod q_i
 * (ReEncrypt at changeCipherDomain.cpp:74 followed by EvalAdd at aggregateEncryptedWeights.cpp:82, without the
 * round trip of the re-encrypted ciphertext through HBM).  d_acc must not alias d_ct. */
int mkckks_reencrypt_accumulate_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_evk, uint64_t *d_acc,
                                      uint32_t n_ct, uint32_t nl);
/* n-client form of the server loop (changeCipherDomain x n, then the EvalAdd chain of
 * aggregateEncryptedWeights.cpp:82): d_out[b] = sum_c ReEncrypt(d_cts[c][b], d_evks[c]) coefficient-wise mod q_i.
 * d_cts u64[n_clients][n_ct][2][nl][N], d_evks u64[n_clients][beta][2][D][N] (one re-encryption key per client,
 * all towards the common domain), d_out u64[n_ct][2][nl][N].  Bit-identical to re-encrypting every ciphertext and
 * adding them in any order; the last ModDown pass of all clients and the sum are one kernel. */
int mkckks_reencrypt_sum_batch(mkckks_ctx *c, const uint64_t *d_cts, const uint64_t *d_evks, uint64_t *d_out,
                               uint32_t n_clients, uint32_t n_ct, uint32_t nl);
/* The form the integer-class Q limbs (q_0) take inside mkckks_reencrypt_sum_batch / mkckks_reencrypt_wsum_batch for a
 * chunk of n_idx ciphertext indices on a ring with row_tiles row tiles and n_int_q such limbs: 1 = one kernel whose
 * workgroup walks the clients, 0 = two kernels through a compact workspace.  mode is the switch MKCKKS_Q0_WALK: 0 and 1
 * force a form, any other value chooses by grid size.  A pure function (no context, no device); both forms give the same
 * bits. */
int mkckks_q0_walk_choice(uint32_t row_tiles, uint32_t n_int_q, uint32_t n_idx, int mode);
/* How many fp64-class ModUp targets of a digit whose sources are all fp64-class are converted inside the inverse column
 * pass of those sources instead of by the conversion kernels: the digit has n_fp_targets of them, and the call's grid
 * for that pass is grid = polynomials x such digits x column tiles.  mode is the switch MKCKKS_ICOL_CONV: 0..3 force
 * that many (as far as the digit has them), any other value chooses.  A pure function (no context, no device); every
 * choice gives the same bits. */
uint32_t mkckks_icol_conv_targets(uint32_t n_fp_targets, uint64_t grid, int mode);
/* ---- weighted aggregation: sum_c w_c * x_c in place of the plain mean -----------------------------------------------
 * The weighted form of the server loop (ReEncrypt x n, then per client cc->EvalMult(ct, w_c) as at
 * aggregateEncryptedWeights.cpp:82-83, then the EvalAdd chain), with the weights folded into what the merged n-client
 * flow already reads.  M_c = trunc(h_weights[c] * sf(sf_level) + 0.5), the 128-bit integer of EvalMult(ct, w_c), reduced
 * modulo whichever limb it meets.  Hybrid key switching is linear in the key, so
 *   M_c * ReEncrypt(ct_c, evk_c) ~ ReEncrypt((M_c * c0_c, c1_c), M_c * evk_c)      (equal up to ApproxModDown's rounding)
 * and the weighted sum is DEFINED as the right-hand side, summed over the clients, followed by ONE mkckks_rescale_batch:
 * the rescale's rounding error is not multiplied by the 2^p-sized constant as it is in rescale-then-EvalMult.
 * sf_level: for noiseScaleDeg-2 inputs at level = L - nl pass level + 1 and rescale afterwards -- the result has the
 * limbs, level, scale (S_in / q_{nl-1} * sf(level + 1)) and noiseScaleDeg (2) of mkckks_rescale_mult_const_batch(sum, .);
 * for noiseScaleDeg-1 inputs pass level and do not rescale (the bookkeeping of mkckks_mult_const_batch).
 * Headroom: before the rescale the encrypted coefficients are about S_in * sf(sf_level) * |sum_c w_c v_c|, which must
 * stay below q_0 * ... * q_{nl-1} / 2, as in the compact-leg rule below: log2(S_in * sf(sf_level)) <
 * log2(q_0 ... q_{nl-1}) - 1 leaves room for |values| <= 1 and no more.  The library cannot check it.
 * All three: h_weights are HOST doubles, read before the call returns; a weight that is not finite or whose constant
 * does not fit 125 bits -> MKCKKS_E_INVALID; a zero count is a no-op; host-only context -> MKCKKS_E_NODEVICE.  The
 * constant tables are cached on the device per (weights, sf_level): a step that repeats them uploads nothing.
 *
 * (aggregateEncryptedWeights.cpp:82-83) d_evk_out[k] = M_k * d_evk_in[k] on all D limbs (Q and P) of n_keys eval keys
 * u64[n_keys][beta][2][D][N].  Once per (key, weight, level).  d_evk_out must not overlap d_evk_in (MKCKKS_E_INVALID). */
int mkckks_scale_evk_batch(mkckks_ctx *c, const uint64_t *d_evk_in, uint64_t *d_evk_out, uint32_t n_keys,
                           const double *h_weights, uint32_t sf_level);
/* (aggregateEncryptedWeights.cpp:82-83) d_out[b] = sum_c ReEncrypt((M_c * c0_c[b], c1_c[b]), d_evks_scaled[c]): layouts
 * of mkckks_reencrypt_sum_batch; d_evks_scaled = mkckks_scale_evk_batch of the clients' keys with the SAME weights and
 * level (a key scaled with other weights gives a wrong aggregate and no error).  d_out has nl limbs and is not yet
 * rescaled; it must not overlap d_cts.  Bit-identical to the per-client chain on the scaled inputs. */
int mkckks_reencrypt_wsum_batch(mkckks_ctx *c, const uint64_t *d_cts, const uint64_t *d_evks_scaled, uint64_t *d_out,
                                uint32_t n_clients, uint32_t n_ct, uint32_t nl, const double *h_weights, uint32_t sf_level);
/* (aggregateEncryptedWeights.cpp:82-83) d_out[b] = sum_k M_k * d_in[k][b], d_in u64[n_terms][n_ct][2][nl][N]: the
 * in-domain clients, EvalMult(ct, w_k) and the EvalAdd chain in one pass.  first_is_sum != 0: term 0 is added as it is
 * (the slot mkckks_reencrypt_wsum_batch wrote) and h_weights[0] is ignored.  d_out may be term 0 itself and must not
 * overlap d_in otherwise. */
int mkckks_eval_wsum_batch(mkckks_ctx *c, const uint64_t *d_in, uint64_t *d_out, uint32_t n_terms, uint32_t n_ct, uint32_t nl,
                           const double *h_weights, uint32_t sf_level, int first_is_sum);
/* fan-out form of the distribution leg (orchestration/server_fns.sh:76-80: changeCipherDomain.cpp:74 run n-1 times
 * on ONE input file, once per client key): d_out[k][b] = ReEncrypt(d_ct[b], d_evks[k]).
 * d_ct u64[n_ct][2][nl][N] (read-only), d_evks u64[n_keys][beta][2][D][N] (layout of mkckks_reencrypt_sum_batch),
 * d_out u64[n_keys][n_ct][2][nl][N].  The key-independent half of the key switch (INTT of c1, ModUp conversions,
 * forward transform of every converted digit) runs once per ciphertext instead of once per (ciphertext, key).
 * Bit-identical, for every k, to mkckks_reencrypt_batch(c, d_ct, d_evks + k * evk_words, d_out + k * n_ct * ct_words,
 * n_ct, nl).  d_out must not overlap d_ct (MKCKKS_E_INVALID); n_keys == 0 or n_ct == 0 is a no-op. */
int mkckks_reencrypt_fanout_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_evks, uint64_t *d_out,
                                  uint32_t n_keys, uint32_t n_ct, uint32_t nl);
/* ---- compact ciphertexts for the distribution leg ------------------------------
 * What goes back to a client is only ever decrypted, and a ciphertext that will only be decrypted needs enough modulus
 * for scale * |value| + noise and nothing more (OpenFHE: cc->Compress(ct, towersLeft), "before sending the encrypted
 * result for decryption").  prefix(ct, m) = the first m limbs of both components: a lower level of the same RNS
 * ciphertext, valid while the encrypted coefficients stay below q_0 * ... * q_{m-1} / 2.
 * Order: the prefix is cut while the ciphertext is at noiseScaleDeg 2 (after EvalMult(., 1/n)), the key switch runs at
 * the low level, the rescale comes last -- the key-switch noise is added at scale ~ 2^(2p) and divided away by the
 * closing rescale.  (Rescale first, then cut, then key switch -- OpenFHE's Compress + ReEncrypt -- costs 5-8 bits.)
 * Headroom: for slot values bounded by A every plaintext coefficient is bounded by S * A (S the input's scaling factor,
 * ~ 2^(2p)), so nl_out = k is enough when q_0 * ... * q_k / 2 > S * A + noise.  With a 60-bit q_0 and p-bit scaling
 * limbs: k = 1 holds |values| < 2^(58-p) (256 at p = 50, 2^18 at p = 40; one bit is kept for noise and for sums that
 * exceed A), every further limb adds p bits.  The bound is on coefficients, so constant vectors reach it; beyond it
 * decryption wraps and returns garbage, not a small error.  The library cannot check it (the values are encrypted): it
 * is the deployment's choice, like the scaling size.
 *
 * compress for decryption: d_out[b] = Rescale(prefix(d_in[b], nl_out + 1)) -- drops limb nl_out with rounding
 * (ModReduceInternalInPlace on the truncated ciphertext).  d_in u64[n_ct][2][nl_in][N] (read in place, strided),
 * d_out u64[n_ct][2][nl_out][N], 1 <= nl_out < nl_in <= L.  Bit-identical to mkckks_rescale_batch at nl_out + 1 on a
 * packed copy of the prefix.  New scaling factor: old / q_{nl_out}; noiseScaleDeg 2 -> 1.  d_out must not overlap d_in
 * (MKCKKS_E_INVALID); n_ct == 0 is a no-op. */
int mkckks_compress_batch(mkckks_ctx *c, const uint64_t *d_in, uint64_t *d_out, uint32_t n_ct, uint32_t nl_in,
                          uint32_t nl_out);
/* compact fan-out: d_out[k][b] = Rescale(ReEncrypt(prefix(d_ct[b], nl_out + 1), d_evks[k])).
 * d_ct u64[n_ct][2][nl_in][N] read-only (the prefix is read in place), d_evks as mkckks_reencrypt_fanout_batch, d_out
 * u64[n_keys][n_ct][2][nl_out][N].  Bit-identical, for every k, to: packed copy of the prefix ->
 * mkckks_reencrypt_fanout_batch at nl_out + 1 -> mkckks_rescale_batch at nl_out + 1.  The key switch has
 * ceil((nl_out + 1) / alpha) digits over nl_out + 1 + K limbs instead of the full level's; the closing rescale is one
 * pass over all (key, ciphertext, component) polynomials of a key group.  d_out must not overlap d_ct
 * (MKCKKS_E_INVALID); n_keys == 0 or n_ct == 0 is a no-op. */
int mkckks_reencrypt_fanout_compact_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_evks, uint64_t *d_out,
                                          uint32_t n_keys, uint32_t n_ct, uint32_t nl_in, uint32_t nl_out);
/* stages of the above, exposed for parity tests and profiling:
 * KeySwitchHYBRID::EvalKeySwitchPrecomputeCore: c1 u64[n][nl][N] ->
 * digits u64[n][nparts][nl+K][N]; ApproxModDown: u64[n][nl+K][N] -> u64[n][nl][N]. */
int mkckks_modup_batch(mkckks_ctx *c, const uint64_t *d_c1, uint64_t *d_digits, uint32_t n, uint32_t nl);
int mkckks_moddown_batch(mkckks_ctx *c, const uint64_t *d_in, uint64_t *d_out, uint32_t n, uint32_t nl);

/* ---- randomness for KeyGen / ReKeyGen / Encrypt, generated in HBM ------------
 * OpenFHE's TernaryUniformGenerator, DiscreteGaussianGenerator (sigma 3.19) and
 * DiscreteUniformGenerator.  Generator: the ChaCha20 block function (RFC 8439) under a
 * 256-bit key (h_key32: 32 HOST bytes, drawn from the OS by the callers -- getrandom(2) in
 * ppqsflhe_amd/host/sampler.hpp): a cryptographic PRF, like OpenFHE's Blake2-based PRNG and
 * unlike a 64-bit-seeded statistical generator.  Counter based: element i of `stream_id`
 * is a pure function of (key, stream_id, i).  Distributional parity only (OpenFHE's PRNG
 * stream cannot be reproduced).  d_out: int8[count] / int32[count] /
 * u64[n_polys][nl(+K)][N] (uniform in [0, q_limb), exact by rejection). */
#define MKCKKS_SAMPLER_KEY_BYTES 32
int mkckks_sample_ternary(mkckks_ctx *c, int8_t *d_out, size_t count, const uint8_t *h_key32, uint32_t stream_id);
int mkckks_sample_gauss(mkckks_ctx *c, int32_t *d_out, size_t count, double sigma, const uint8_t *h_key32,
                        uint32_t stream_id);
int mkckks_sample_uniform(mkckks_ctx *c, uint64_t *d_out, uint32_t n_polys, uint32_t nl, int with_p,
                          const uint8_t *h_key32, uint32_t stream_id);
/* wide ("flooding") Gaussian errors for mkckks_rerandomize_batch: d_out int64[count], element i =
 * (int64_t)rint(sigma * z) with z = component i % 2 of the Box-Muller pair i / 2 of stream `stream_id` (the mapping
 * csrc/sampler_kernels.hpp documents for decode flooding: chacha_normal_pair) -- a pure function of (key, stream_id, i),
 * independent of launch geometry and of `count`.  2^6 <= sigma <= 2^56, else MKCKKS_E_INVALID: below 2^6 a rounded
 * normal is no stand-in for a discrete Gaussian; |z| < 8.6, so up to 2^56 every |e| stays below the 2^62 of
 * mkckks_rerandomize_batch.  count == 0 is a no-op. */
int mkckks_sample_gauss_wide(mkckks_ctx *c, int64_t *d_out, size_t count, double sigma, const uint8_t *h_key32,
                             uint32_t stream_id);
/* known-answer hook: the 16 output words of one ChaCha20 block (RFC 8439 2.3.2) -> d_out16 (device) */
int mkckks_chacha20_block(mkckks_ctx *c, uint32_t *d_out16, const uint8_t *h_key32, uint32_t counter,
                          const uint32_t *h_nonce3);

/* ---- cc->KeyGen()  (client/src/keyGen.cpp:33) -----------------------------
 * randomness is supplied by the caller (mkckks_sample_* under OS-drawn keys in
 * ppqsflhe_amd/host, or a test's seeded vectors): s ternary int8[N], e int32[N] (COEFFICIENT),
 * a u64[D][N] uniform residues (taken as EVALUATION).
 * d_pk out u64[2][D][N], d_sk out u64[D][N] (EVALUATION). */
int mkckks_keygen(mkckks_ctx *c, const int8_t *d_s, const uint64_t *d_a, const int32_t *d_e,
                  uint64_t *d_pk, uint64_t *d_sk);
/* ---- cc->ReKeyGen(mySk, peerPk)  (client/src/REkeyGen.cpp:52) -------------
 * s_old int8[N]; u int8[beta][N]; e0,e1 int32[beta][N]; d_evk out u64[beta][2][D][N]. */
int mkckks_rekeygen(mkckks_ctx *c, const int8_t *d_s_old, const uint64_t *d_pk_new, const int8_t *d_u,
                    const int32_t *d_e0, const int32_t *d_e1, uint64_t *d_evk);

/* ==== slot rotations and slot sums: cc->EvalRotateKeyGen / cc->EvalRotate / cc->EvalSumKeyGen / cc->EvalSum ============
 * Upstream CryptoContext calls the reference never makes: every operation of its mains leaves a slot where the client
 * put it.  With them a ciphertext's slots can be moved, summed, and (mkckks_mult_plain_rescale_batch first) turned into
 * an encrypted inner product with a public vector.
 * Automorphism: for odd g < 2N, sigma_g(a)(X) = a(X^g).  In EVALUATION format (X[i] = a(psi^(2 brev(i) + 1))) it is a
 * gather that is the same for every limb: sigma_g(X)[i] = X[src(i)] with 2 brev(src(i)) + 1 = (2 brev(i) + 1) g mod 2N.
 * On a ternary secret in COEFFICIENT format coefficient k goes to position k g mod 2N; a position at or above N means
 * position - N with the sign flipped.  Slot j sits at zeta^(5^j), so g = 5^r mod 2N rotates LEFT by r:
 * out[j] = in[(j + r) mod N/2]; a negative r is the inverse element; g = MKCKKS_GALOIS_CONJ(N) = 2N - 1 conjugates.
 * Refusals of all compute calls below: MKCKKS_E_INVALID for an even g or g >= 2N, null pointers, nl outside [1, L],
 * an output that overlaps its input; a zero count is a no-op; a host-only context gives MKCKKS_E_NODEVICE.  The
 * polynomial arrays must be 16-byte aligned (every allocation is; an odd word offset into one is not): MKCKKS_E_INVALID.
 *
 * (cc->EvalRotate's index -> element map, upstream FindAutomorphismIndex2nComplex) host only, works on a device = -1
 * context: *g = 5^step mod 2N; step < 0 gives the inverse element, step 0 gives 1. */
#define MKCKKS_GALOIS_CONJ(ring_dim) (2u * (ring_dim) - 1u)
int mkckks_galois_element(const mkckks_ctx *c, int32_t step, uint32_t *g);
/* (cc->EvalRotate, the automorphism half: upstream DCRTPoly::AutomorphismTransform) d_out[p] = sigma_g(d_in[p]) on
 * u64[n_polys][nl][N], EVALUATION, out of place.  No arithmetic: canonical residues stay canonical. */
int mkckks_automorphism_batch(mkckks_ctx *c, const uint64_t *d_in, uint64_t *d_out, uint32_t n_polys, uint32_t nl, uint32_t g);
/* (cc->EvalRotateKeyGen, the secret's half) d_out int8[N] = sigma_g(d_s), COEFFICIENT, signed; out of place. */
int mkckks_automorphism_secret(mkckks_ctx *c, const int8_t *d_s, int8_t *d_out, uint32_t g);
/* (cc->EvalRotateKeyGen / cc->EvalSumKeyGen for one element) The Galois key for g is the re-encryption key from
 * sigma_g(s) to s: bit for bit mkckks_rekeygen(sigma_g(d_s), d_pk, d_u, d_e0, d_e1), same layouts and randomness
 * arguments; d_pk is the public key of s; d_evk out u64[beta][2][D][N].  Generated by the OWNER of s (for the server's
 * slot sums: the owner of the common-domain key).  A Galois key for a JOINT key (mkckks_keygen_join: nobody holds s) is
 * made collectively, in one round: every party calls this with its OWN s_p and the JOINT public key, and
 * mkckks_evk_sum adds the n shares ("collective evaluation keys" below, with the noise and the security rules). */
int mkckks_galois_keygen(mkckks_ctx *c, const int8_t *d_s, const uint64_t *d_pk, const int8_t *d_u, const int32_t *d_e0,
                         const int32_t *d_e1, uint32_t g, uint64_t *d_evk);
/* (cc->EvalRotate) d_out[b] = ReEncrypt((sigma_g(c0), sigma_g(c1)), d_evk): word for word what mkckks_reencrypt_batch
 * returns on the permuted ciphertext.  d_ct, d_out u64[n_ct][2][nl][N], nl <= L (a partial last digit included); d_evk
 * from mkckks_galois_keygen with the SAME g (another key gives noise and no error).  Both components are permuted
 * straight into d_out and the key switch runs there in place: one read and one write of the ciphertext more than
 * mkckks_reencrypt_batch.  Noise: that of one re-encryption. */
int mkckks_rotate_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_evk, uint64_t *d_out, uint32_t n_ct, uint32_t nl,
                        uint32_t g);
/* (cc->EvalSum) d_out = d_ct, then for k = 0 .. log2(span) - 1 in that order: d_out = d_out + Rotate(d_out, 5^(2^k))
 * with key k of d_evks u64[log2 span][beta][2][D][N] (key k for step 2^k; not read when span = 1, which copies the
 * input).  Slot j then holds in[j] + ... + in[j + span - 1] (indices mod N/2); with span = N/2 every slot holds the sum
 * of all slots.  span: a power of two in [1, N/2], else MKCKKS_E_INVALID.  Bit-identical to the loop of
 * mkckks_rotate_batch and mkckks_eval_add_batch.  Noise: log2(span) re-encryptions, each doubled by the steps after it. */
int mkckks_slot_sum_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_evks, uint64_t *d_out, uint32_t n_ct,
                          uint32_t nl, uint32_t span);

/* ==== linear transforms by diagonals, double hoisted: EvalLinearTransform over cc->EvalFastRotationPrecompute /
 * cc->EvalFastRotation (upstream ckksrns-advancedshe: EvalLinearTransform, EvalFastRotationExt) ==========================
 * Upstream calls the reference never makes.  They apply a PUBLIC linear map to an encrypted vector by the diagonal
 * method,
 *     out[j] = sum_r diag_r[j] * in[(j + r) mod N/2],
 * which is what projecting the aggregate on a public basis, undoing a sketch, mixing layers, applying a banded or block
 * matrix to every block of the update and several inner products with public vectors at once all come down to.
 * Double hoisting: the ModUp digits of c1 are made ONCE per ciphertext; every rotation is only an eval-key inner product
 * on permuted digits; the plaintext diagonals are multiplied in while the sum is still over the extended basis Q_l P; ONE
 * ModDown per component closes the transform.  Against the composition (mkckks_rotate_batch + mkckks_mult_plain_batch per
 * diagonal, mkckks_eval_sum_batch) that is 1 inverse transform of c1 instead of n_rot, 1 ModUp instead of n_rot and 2
 * ModDowns instead of 2 n_rot; ModDown's rounding error enters once, after the plaintext products, not n_rot times each
 * multiplied by a plaintext of the size of the scaling factor.
 *
 * (the plaintext side of EvalLinearTransformPrecompute: MakeCKKSPackedPlaintext over the extended basis, upstream
 * "MakeAuxPlaintext") What mkckks_encode_batch does, over Q_l P: d_pt out u64[n][nl+K][N], EVALUATION, canonical; slots
 * 0 .. nl-1 are the Q limbs, bit-identical to mkckks_encode_batch, slots nl .. nl+K-1 are the P limbs, the residues of
 * the same rounded integer polynomial. */
int mkckks_encode_ext_batch(mkckks_ctx *c, const double *d_vals, uint64_t *d_pt, uint32_t n, uint32_t nl, double scale);
/* (EvalLinearTransform with EvalFastRotationExt and one closing KeySwitchDown) d_ct, d_out u64[n_ct][2][nl][N], not
 * overlapping; d_evks u64[n_rot][beta][2][D][N], the Galois key of h_g[r] in slot r (the layout of mkckks_slot_sum_batch);
 * d_pts u64[n_rot][nl+K][N] from mkckks_encode_ext_batch, shared by all ciphertexts; h_g a HOST array of n_rot Galois
 * elements.  g = 1 means "no rotation": its key slot is never read (d_evks may be null when every element is 1).
 * Duplicate elements are allowed.  Definition, bit for bit: with m_i the modulus of extended slot i, d_j the digits
 * mkckks_modup_batch returns for c1, sigma_g the gather of mkckks_automorphism_batch and (kb, ka)_{r,j} key r,
 *     A_b[i] = sum_r pt_r[i] ( sum_j sigma_{g_r}(d_j[i]) kb_{r,j}[i] + [i < nl] [P]_{q_i} sigma_{g_r}(c0[i]) )  mod m_i
 *     A_a[i] = sum_r pt_r[i] ( sum_j sigma_{g_r}(d_j[i]) ka_{r,j}[i] )                                          mod m_i
 *     (for g_r = 1 the inner key sum is [i < nl] [P]_{q_i} c1[i] in A_a and absent from A_b)
 *     d_out = ( ModDown(A_b), ModDown(A_a) ), each word for word what mkckks_moddown_batch returns.
 * P x on the Q limbs passes through ModDown exactly as + x.  Residues are canonical and every sum is exact mod m_i.
 * Scale and level: for an input at level L - nl with scale S encode the diagonals at sf(level) (noiseScaleDeg 1) or
 * sf(level + 1) (noiseScaleDeg 2), the rule of mkckks_mult_plain_batch; the output has nl limbs at scale S sf and the
 * caller rescales with mkckks_rescale_batch.  Headroom is the caller's:
 *     log2(S sf max_j sum_r |diag_r[j]|) < log2(q_0 ... q_{nl-1}) - 1.
 * Refusals as in the rotation block: MKCKKS_E_INVALID for null pointers, nl outside [1, L], an even g or g >= 2N, an
 * output that overlaps an input, arrays that are not 16-byte aligned, more than 6 key-switch digits; n_rot == 0 or
 * n_ct == 0 is a no-op; a host-only context gives MKCKKS_E_NODEVICE. */
int mkckks_linear_transform_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_evks, const uint64_t *d_pts,
                                  const uint32_t *h_g, uint64_t *d_out, uint32_t n_rot, uint32_t n_ct, uint32_t nl);
/* (the baby-step giant-step form of the same transform) Every step is r = G + b with n1 baby steps b and n2 giant steps
 * G, and
 *     out = sum_G rot_G( sum_b rot_{-G}(diag_{G+b}) * rot_b(x) ),
 * which needs about n1 + n2 Galois keys where the call above needs n1 n2 (a 128 x 128 block: 30 keys of ~50 MB each at
 * N = 2^16 in place of 254).  d_ct, d_out u64[n_ct][2][nl][N], not overlapping; h_gb[n1], h_gg[n2] HOST arrays of Galois
 * elements; d_bkeys u64[n1][beta][2][D][N] and d_gkeys u64[n2][..]: slot k holds the key of element k, the slot of an
 * element 1 is never read and either array may be null when all its elements are 1; d_pts u64[n2][n1][nl+K][N] from
 * mkckks_encode_ext_batch, entry (t, b) the diagonal of step G_t + b rolled RIGHT by G_t slots; h_present HOST
 * uint8[n2][n1]: the plaintext slot of an absent entry is never read, a giant row without a present entry costs nothing
 * (its ModDown and ModUp included), a baby column without one is not computed.  Duplicate elements are allowed.
 * Definition, bit for bit (notation of the call above; all residues canonical, every sum exact mod m_i):
 *   babies, g = h_gb[b]:
 *     Bb_b[i] = sum_j sigma_g(d_j[i]) kb_{b,j}[i] + [i < nl] [P]_{q_i} sigma_g(c0[i])
 *     Ba_b[i] = sum_j sigma_g(d_j[i]) ka_{b,j}[i]
 *     (g = 1:  Bb_b[i] = [i < nl] [P]_{q_i} c0[i],  Ba_b[i] = [i < nl] [P]_{q_i} c1[i])
 *   inner sums, for each giant t:
 *     Ub_t[i] = sum_{b present} pt_{t,b}[i] Bb_b[i],   Ua_t[i] = sum_{b present} pt_{t,b}[i] Ba_b[i]
 *   giants, g = h_gg[t]:  g = 1 adds (Ub_t, Ua_t) to (A_b, A_a); otherwise v_t = ModDown(Ua_t) (u64[nl][N], word for word
 *   mkckks_moddown_batch), e_j the mkckks_modup_batch digits of v_t, and
 *     A_b[i] += sigma_g(Ub_t[i]) + sum_j sigma_g(e_j[i]) kgb_{t,j}[i]
 *     A_a[i] +=                    sum_j sigma_g(e_j[i]) kga_{t,j}[i]
 *   (Ub_t carries the factor P already: it is permuted on all nl + K slots and not multiplied again)
 *   d_out = ( ModDown(A_b), ModDown(A_a) ).
 * With n2 = 1 and h_gg[0] = 1 the call returns the words of mkckks_linear_transform_batch on the same keys, plaintexts
 * and elements.  Scale, level and headroom follow that call.  Noise: one key switch per level of the tree and one ModDown
 * rounding per giant, which enters before no plaintext product.  Workspace: babies, inner sums and giant digits are per
 * ciphertext; the ciphertexts are taken in chunks of min(MKCKKS_CHUNK, max(1, cap / per-ciphertext words)) with a cap of
 * 2 GiB (MKCKKS_BSGS_WS_MIB, in MiB, overrides it); the bits do not depend on the chunk.
 * Refusals: MKCKKS_E_INVALID for null pointers, an even g or g >= 2N, n1 or n2 equal to 0 or above MKCKKS_BSGS_MAX, nl
 * outside [1, L], an output that overlaps an input, arrays that are not 16-byte aligned, more than 6 key-switch digits;
 * n_ct == 0 or no present entry at all is a no-op; a host-only context gives MKCKKS_E_NODEVICE. */
#define MKCKKS_BSGS_MAX 64
int mkckks_linear_transform_bsgs_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_bkeys, const uint32_t *h_gb,
                                       uint32_t n1, const uint64_t *d_gkeys, const uint32_t *h_gg, uint32_t n2,
                                       const uint64_t *d_pts, const uint8_t *h_present, uint64_t *d_out, uint32_t n_ct,
                                       uint32_t nl);

/* ==== ciphertext products: cc->EvalMultKeyGen / cc->EvalMult(ct, ct) / cc->Relinearize / cc->EvalInnerProduct(ct, ct) ===
 * Upstream CryptoContext calls the reference never makes: everything its mains compute is linear in the encrypted
 * values.  With them the server can form products of two ENCRYPTED vectors: squared norms, the alignment with an
 * encrypted reference update, pairwise distances, per-coordinate variances; mkckks_slot_sum_batch then turns a product
 * into an encrypted inner product, and only that scalar is decrypted.
 * Tensor product, pointwise mod q_i in EVALUATION format: (a0, a1) x (b0, b1) = (a0 b0, a0 b1 + a1 b0, a1 b1) =: (d0, d1,
 * d2), a degree-2 ("three-component") ciphertext u64[n_ct][3][nl][N] that decrypts as d0 + d1 s + d2 s^2.
 * Relinearisation key: the re-encryption key from s^2 to s.  Relinearisation: (d0, d1) + KeySwitch(d2, rlk), the hybrid
 * key switch of mkckks_reencrypt_batch on the degree-2 component.
 * Scale rule: the result has scale S_a * S_b on the same limbs, noiseScaleDeg = the sum of the operands'; the caller
 * rescales with mkckks_rescale_batch.  Headroom: log2(S_a * S_b * |values|^2) must stay below
 * log2(q_0 ... q_{nl-1}) - 1; the library cannot check it.  Noise: that of one re-encryption plus the product terms
 * (m_a e_b + m_b e_a + e_a e_b).
 * Refusals of the compute calls: MKCKKS_E_INVALID for null pointers, nl outside [1, L], n_terms == 0, an output that
 * overlaps an input (mkckks_mult_relin_batch alone accepts an output that IS an input); a zero n_ct is a no-op; a
 * host-only context gives MKCKKS_E_NODEVICE.  The ciphertext arrays are read and written 16 bytes at a time and must
 * be 16-byte aligned (every allocation is; an odd word offset into one is not): MKCKKS_E_INVALID.
 *
 * (cc->EvalMultKeyGen) The relinearisation key of s: bit for bit mkckks_rekeygen with NTT(s_old) replaced by sk^2, the
 * pointwise square of the EVALUATION-form secret over all D limbs: evk[j][0] = pk0 u_j + e0_j + (P mod q_i) sk^2 on digit
 * j's own limbs (the gadget is 0 elsewhere, and 0 on the P limbs), evk[j][1] = pk1 u_j + e1_j.  Arguments, randomness
 * layouts and d_evk u64[beta][2][D][N] as mkckks_galois_keygen, without g.  Generated by the OWNER of s (for the server's
 * products: the owner of the common-domain key).  A relinearisation key for a JOINT key is made collectively, in two
 * rounds: mkckks_rekeygen(s_p, joint pk) summed by mkckks_evk_sum, then mkckks_relin_share summed by mkckks_evk_sum
 * ("collective evaluation keys" below, with the noise and the security rules).  The compute calls of this section take a
 * collectively made key unchanged. */
int mkckks_relin_keygen(mkckks_ctx *c, const int8_t *d_s, const uint64_t *d_pk, const int8_t *d_u, const int32_t *d_e0,
                        const int32_t *d_e1, uint64_t *d_evk);
/* (cc->EvalMultNoRelin, summed) d_out3[b] = sum over t < n_terms of the tensor product of d_a[t][b] and d_b[t][b];
 * d_a, d_b u64[n_terms][n_ct][2][nl][N], d_out3 u64[n_ct][3][nl][N], canonical.  n_terms = 1 is the plain tensor
 * product; d_a == d_b is the square (two polynomials are read instead of four).  The lazy-relinearisation form: many
 * products, ONE key switch.  d_out3 overlaps neither input. */
int mkckks_tensor_sum_batch(mkckks_ctx *c, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out3, uint32_t n_terms,
                            uint32_t n_ct, uint32_t nl);
/* (cc->Relinearize) d_out[b] = (d0, d1) + KeySwitch(d2, d_rlk) of d_in3 u64[n_ct][3][nl][N]; d_out u64[n_ct][2][nl][N],
 * nl <= L (a partial last digit included).  Bit for bit mkckks_eval_add_batch((d0, d1), mkckks_reencrypt_batch((0, d2),
 * d_rlk)).  d_out never overlaps d_in3: the key switch reads d2 after (d0, d1) were written. */
int mkckks_relinearize_batch(mkckks_ctx *c, const uint64_t *d_in3, const uint64_t *d_rlk, uint64_t *d_out, uint32_t n_ct,
                             uint32_t nl);
/* (cc->EvalMult(ct, ct)) d_out = Relinearize(tensor product of d_a and d_b): bit-identical to mkckks_tensor_sum_batch
 * with one term followed by mkckks_relinearize_batch, but d2 exists only in the engine's chunk buffer.  d_out may be
 * exactly d_a or d_b (any other overlap is refused); d_a == d_b squares. */
int mkckks_mult_relin_batch(mkckks_ctx *c, const uint64_t *d_a, const uint64_t *d_b, const uint64_t *d_rlk, uint64_t *d_out,
                            uint32_t n_ct, uint32_t nl);

/* ==== polynomial evaluation: cc->EvalPoly (ckksrns-advancedshe EvalPolyPS), fused Paterson-Stockmeyer products ==========
 * A non-linear function of an encrypted slot: p(x) = c_0 + c_1 x + ... + c_d x^d in the power basis, 2 <= d <= 63,
 * applied to every slot of every ciphertext: clipping by a polynomial approximation of min(1, C / sqrt(t)) at an
 * encrypted squared norm, smooth signs, activations after a linear transform.  Upstream call the reference never makes.
 *
 * Input: ciphertexts x at nl limbs, noiseScaleDeg 1, scale S_1 (a host double).
 * Plan.  B = the smallest power of two with B^2 >= d + 1 (2, 4 or 8), G = ceil((d + 1) / B), 2 <= G <= B; coefficients
 * beyond d are zero.  p(x) = sum_{j<G} sum_{i<B} c_{jB+i} x^i y^j with y = x^B.
 * Power ladder of a base z: z^1 = z; for k >= 2 with i = ceil(k / 2), j = k - i:
 *     z^k = mkckks_rescale_batch(mkckks_mult_relin_batch(z^i, prefix(z^j, nl_i))) at nl_k = nl_i - 1 limbs,
 *     S_k = S_i * S_j / q_{nl_i - 1}, computed in that order in doubles,
 * prefix(., m) = the first m limbs of both components (the level cut of mkckks_compress_batch, without its rescale).  The
 * depth of z^k is ceil(log2 k).  Babies x^1 .. x^{B-1}; y = x^{B/2} x^{B/2} by the same rule (it is power B of the ladder
 * on x); giants y^1 .. y^{G-1} by the ladder on y.  x^0 and y^0 are the virtual ciphertext "1" with scale 1.
 * nl_T = the smallest limb count among babies and giants = nl - log2 B - ceil(log2(G - 1)) (ceil(log2 1) = 0).
 * Constants.  nl_out = nl_T - 2 >= 1, else the call is refused.  S_out = the standard scale of the output's level,
 * mkckks_scaling_factor(L - nl_out): the result adds to and multiplies with any ordinary ciphertext there.  With
 * Sigma = S_out * q_{nl_T-1} * q_{nl_T-2}:  w_{j,i} = c_{jB+i} * (Sigma / (S_{x^i} * S_{y^j})),  M_{j,i} = rint(w_{j,i}) as an
 * integer (a double at or above 2^53 is one, so M is exact at any size), used as its residue mod each q_t, t < nl_T; a
 * negative M is q - (|M| mod q).  A non-finite w, or |w| >= q_0 ... q_{nl_T-1} / 2, is MKCKKS_E_INVALID.
 * Fused outer sum, on the first nl_T limbs, pointwise mod q_t, b_i = prefix(x^i), g_j = prefix(y^j):
 *     Q_j = sum_{i>=1} M_{j,i} b_i                                              (two components, never stored)
 *     (d0, d1, d2) = sum_{j>=1} [Q_j (x) g_j + M_{j,0} (g_j, 0)] + (Q_0, 0) + (M_{0,0}, 0, 0)
 * (x) the tensor product of mkckks_tensor_sum_batch; M_{0,0} is added to every word of d0 (a constant polynomial is a
 * constant vector in EVALUATION form).  All results canonical; every sum is exact mod q_t.
 * Close: mkckks_relinearize_batch at nl_T, mkckks_rescale_batch at nl_T and at nl_T - 1: u64[n_ct][2][nl_out][N] at scale
 * S_out, noiseScaleDeg 1.
 * Cost: depth log2 B + ceil(log2(G - 1)) + 2 (up to two levels more than the recursive form's ceil(log2(d + 1)), spent
 * for ONE fused pass); (B - 1) + (G - 2) + 1 relinearisations against d - 1 for Horner's rule (d = 15: 6 against 14).
 * Headroom, the caller's: Sigma * sum_k |c_k| A^k < q_0 ... q_{nl_T-1} / 2 for |x| <= A; the library cannot check it
 * (evalPoly --max-abs does).  Noise: that of the ladder's products, amplified by |p'(x)|.
 * Refusals of the compute calls follow the products block: MKCKKS_E_INVALID for null pointers, arrays that are not 16-byte
 * aligned, an output that overlaps an input, limb counts outside their ranges, more key-switch digits than
 * mkckks_relinearize_batch accepts; a zero n_ct is a no-op; a host-only context gives MKCKKS_E_NODEVICE.
 * MKCKKS_POLY_FUSED=0 runs the outer sum as the composition (mkckks_eval_wsum_batch's kernel per giant index on packed
 * prefix copies, mkckks_tensor_sum_batch's kernel, the constant column and term), =1 as the fused kernel; unset, the
 * engine chooses.  The bits are the same. */
#define MKCKKS_POLY_MAX_DEGREE 63
#define MKCKKS_POLY_MAX_B 8
struct mkckks_poly_plan {
    uint32_t B, G;        /* baby and giant counts: x^0 .. x^{B-1}, y^0 .. y^{G-1}                    */
    uint32_t nl_T;        /* limbs of the outer sum                                                    */
    uint32_t nl_out;      /* limbs of the result                                                       */
    uint32_t n_relin;     /* relinearisations: (B - 1) + (G - 2) + 1                                   */
    uint32_t depth;       /* levels consumed: nl - nl_out                                              */
    uint32_t baby_nl[MKCKKS_POLY_MAX_B - 1];  /* limbs of x^1 .. x^{B-1} (the first B - 1 entries)   */
    uint32_t giant_nl[MKCKKS_POLY_MAX_B - 1]; /* limbs of y^1 .. y^{G-1} (the first G - 1 entries)   */
};
/* Host-only and pure (works on a device = -1 context).  MKCKKS_E_INVALID for a degree outside [2, 63], nl outside [1, L]
 * or a plan with nl_out < 1 (the message names the limbs needed).  The function and the structure share their name: the
 * structure is always written `struct mkckks_poly_plan`. */
int mkckks_poly_plan(const mkckks_ctx *c, uint32_t degree, uint32_t nl, struct mkckks_poly_plan *out);
/* The ladder: d_out = z^1 .. z^n_pow of d_z u64[n_ct][2][nl][N] at scale scale_in.  Power k is packed
 * u64[n_ct][2][nl_k][N] (nl_k = nl - ceil(log2 k)) directly behind power k - 1: its word offset is
 * n_ct * 2 * N * (nl_1 + ... + nl_{k-1}), derivable from h_nl_out.  h_nl_out / h_scale_out (HOST, n_pow entries each,
 * either may be null) receive nl_k and S_k.  1 <= n_pow <= 64 with nl - ceil(log2 n_pow) >= 1.  Bit-identical to the loop
 * of packed prefix copy + mkckks_mult_relin_batch + mkckks_rescale_batch.  d_out overlaps neither d_z nor the key. */
int mkckks_powers_batch(mkckks_ctx *c, const uint64_t *d_z, const uint64_t *d_rlk, uint64_t *d_out, uint32_t n_ct,
                        uint32_t nl, uint32_t n_pow, double scale_in, uint32_t *h_nl_out, double *h_scale_out);
/* Host-only.  h_w (HOST, double[G][B]) receives w_{j,i}, *scale_out receives S_out: the ladder's scale arithmetic
 * reproduced on the host.  h_coef: degree + 1 coefficients; a zero coefficient gives an exact zero; a non-finite one is
 * MKCKKS_E_INVALID, as is everything mkckks_poly_plan refuses. */
int mkckks_poly_weights(const mkckks_ctx *c, const double *h_coef, uint32_t degree, uint32_t nl, double scale_in,
                        double *h_w, double *scale_out);
/* The fused outer sum for caller-supplied operands and weights: d_baby = x^1 .. x^{B-1} and d_giant = y^1 .. y^{G-1},
 * each packed like the output of mkckks_powers_batch with the limb counts h_baby_nl[B-1] / h_giant_nl[G-1] (HOST; every
 * one in [nl_T, L]), read in place at their first nl_T limbs; h_w HOST double[G][B].  B in {2, 4, 8}, 2 <= G <= B.
 * d_out3 u64[n_ct][3][nl_T][N] overlaps no input. */
int mkckks_poly_tensor_batch(mkckks_ctx *c, const uint64_t *d_baby, const uint32_t *h_baby_nl, const uint64_t *d_giant,
                             const uint32_t *h_giant_nl, const double *h_w, uint64_t *d_out3, uint32_t B, uint32_t G,
                             uint32_t n_ct, uint32_t nl_T);
/* The whole algorithm, workspace-chunked like mkckks_mult_relin_batch: d_out u64[n_ct][2][nl_out][N] = p(d_ct), scale
 * *scale_out (nullable) = S_out.  Bit-identical to mkckks_powers_batch (on x with n_pow = B, then on y = its power B with
 * n_pow = G - 1) + mkckks_poly_weights + mkckks_poly_tensor_batch + mkckks_relinearize_batch + mkckks_rescale_batch
 * twice.  d_ct is not modified; d_out overlaps neither d_ct nor the key. */
int mkckks_poly_eval_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_rlk, const double *h_coef,
                           uint32_t degree, uint64_t *d_out, uint32_t n_ct, uint32_t nl, double scale_in,
                           double *scale_out);

/* ==== Chebyshev series: cc->EvalChebyshevSeries / EvalChebyshevFunction (ckksrns-advancedshe), on the machinery above =====
 * p(u) = c_0 T_0(u) + c_1 T_1(u) + ... + c_d T_d(u), 2 <= d <= 63, T_k the Chebyshev polynomials of the first kind, for
 * a function fitted on an interval [a, b]: |T_k| <= 1 there and the coefficients of a fit decay, where the power-basis
 * coefficients of the same polynomial grow with the degree (the interpolant of 1 / sqrt(t) on [0.25, 4]: 5.0 at d = 15,
 * 9.3e2 at d = 31, 3.6e8 at d = 63) and every bit of that growth is a bit of the ciphertext's precision.  c_0 is the
 * plain coefficient of T_0 (numpy.polynomial.chebyshev's convention); upstream's EvalChebyshevSeries takes c_0 / 2 there.
 * Upstream calls the reference never makes.
 *
 * Interval.  (a, b) exactly (-1, 1): u = x at nl_u = nl limbs, S_u = S_in.  Otherwise one level is spent: alpha = 2 / (b - a),
 * beta = -(a + b) / (b - a), nl_u = nl - 1, Sigma_1 = mkckks_scaling_factor(L - nl_u) * q_{nl-1} and
 *     u = mkckks_rescale_batch(mkckks_affine_batch(x, alpha * (Sigma_1 / S_in), beta * Sigma_1)),
 * so u = alpha x + beta sits at the standard scale of its level, S_u = mkckks_scaling_factor(L - nl_u).  All in doubles, in
 * the order written.
 * Affine map: out = M_a * in + (M_c, 0) with M_a = rint(w_mul), M_c = rint(w_add) as exact integers (the rule of M_{j,i} in
 * the polynomial block, its refusals included), pointwise mod q_t on nl limbs; M_c is added to every word of component 0.
 * No rescale: the result has scale S_in * M_a.
 * Ladder of a base u (T_1 = u, T_0 = the constant 1 with scale 1): for k >= 2 with i = ceil(k / 2), j = k - i (i - j is 0 or 1)
 *     T_k = 2 T_i T_j - T_{i-j}
 *     T_k = mkckks_rescale_batch(mkckks_relinearize_batch(cheb_tensor(T_i, T_j, T_{i-j}; w))) at nl_k = nl_i - 1 limbs,
 *     S_k = S_i * S_j / q_{nl_i - 1},   w = S_i * S_j / S_{i-j}   (the product first, then the quotient; S_0 = 1),
 * the index split, limb counts and scales of the power ladder above (the factor 2 is an integer and leaves the scale
 * alone).  T_{jB} = T_j(T_B): the giants are the same ladder on y = T_B.
 * Ladder step before relinearisation, cheb_tensor(a, b, t; w), on the first nl limbs of a, b, t (each read in place at its
 * own limb count >= nl), pointwise mod q_l, M = rint(w) as an exact integer by the rule of M_{j,i}:
 *     d0 = 2 a0 b0 - M t0,   d1 = 2 (a0 b1 + a1 b0) - M t1,   d2 = 2 a1 b1      (t absent: t0 = 1, t1 = 0)
 * M makes the scale of t equal to S_a * S_b exactly, in an integer, so the difference is formed before the rescale.  All
 * results canonical.
 * Block rewrite.  With the plan (B, G, nl_T, nl_out, limb counts) = mkckks_poly_plan(d, nl_u) and T_{jB+i} = 2 T_i T_{jB} -
 * T_{(j-1)B+(B-i)} for j >= 1, 0 < i < B, the series becomes sum_j sum_i m_{j,i} T_i T_{jB}.  In doubles, in this order:
 *     c' = c padded with zeros to B * G
 *     for j = G - 1 down to 1:  for i = B - 1 down to 1:  m[j][i] = 2 c'[jB+i];  c'[(j-1)B + (B-i)] -= c'[jB+i]
 *                               m[j][0] = c'[jB]
 *     m[0][i] = c'[i] for 0 <= i < B
 * Weights: w_{j,i} = m_{j,i} * (Sigma / (S_{T_i} * S_{y_j})) exactly as mkckks_poly_weights forms them from c (an m of zero
 * gives an exact zero), S_out and Sigma as there.  Outer sum: mkckks_poly_tensor_batch with babies T_1 .. T_{B-1} and giants
 * T_B, T_{2B}, ..; then mkckks_relinearize_batch at nl_T and mkckks_rescale_batch at nl_T and nl_T - 1: u64[n_ct][2][nl_out][N]
 * at scale S_out.  Cost: that of mkckks_poly_eval_batch at the same degree, plus the level and the streaming pass of the map.
 * Headroom, the caller's: Sigma * sum |m_{j,i}| < q_0 ... q_{nl_T-1} / 2 suffices for |u| <= 1, because |T_k| <= 1 (evalPoly
 * --cheb checks it).  Outside [a, b] the T_k grow like the powers and nothing holds.
 * Refusals of the compute calls follow the polynomial block: MKCKKS_E_INVALID for null pointers (d_t alone may be null),
 * arrays that are not 16-byte aligned, an output that overlaps an input (mkckks_affine_batch alone accepts an output that
 * IS its input), limb counts outside their ranges, a >= b or a non-finite bound, a weight that is not finite or does not
 * fit half the modulus of its level (a ladder step's weight S_i * S_j included), a plan with nl_out < 1 (the message names
 * the limbs needed); a zero n_ct is a no-op; a host-only context gives MKCKKS_E_NODEVICE.
 * MKCKKS_CHEB_FUSED=0 runs the ladder step from the kernels of the blocks above (packed prefix copies, the tensor
 * product, doubling and - M t by the weighted sum's kernel and the constant column's), =1 as the fused kernel; unset, the
 * engine chooses.  The bits are the same. */
/* (cc->EvalMult(ct, const) + cc->EvalAdd(ct, const)) d_out = M_a * d_in + (M_c, 0); d_in, d_out u64[n_ct][2][nl][N].  d_out
 * may be exactly d_in. */
int mkckks_affine_batch(mkckks_ctx *c, const uint64_t *d_in, uint64_t *d_out, uint32_t n_ct, uint32_t nl, double w_mul,
                        double w_add);
/* One ladder step before relinearisation for caller-supplied operands: d_a u64[n_ct][2][nl_a][N], d_b ..[nl_b].., d_t
 * ..[nl_t].. or null (the constant; nl_t is then ignored), each limb count in [nl, L]; d_a == d_b squares (two polynomials
 * are read) and needs nl_a == nl_b.  d_out3 u64[n_ct][3][nl][N] overlaps no input. */
int mkckks_cheb_tensor_batch(mkckks_ctx *c, const uint64_t *d_a, uint32_t nl_a, const uint64_t *d_b, uint32_t nl_b,
                             const uint64_t *d_t, uint32_t nl_t, double w, uint64_t *d_out3, uint32_t n_ct, uint32_t nl);
/* The ladder: d_out = T_1 .. T_n of d_u u64[n_ct][2][nl][N] at scale scale_in, packed like the output of
 * mkckks_powers_batch (T_k u64[n_ct][2][nl_k][N] directly behind T_{k-1}); h_nl_out / h_scale_out (HOST, n entries each,
 * either may be null) receive nl_k and S_k.  1 <= n <= 64 with nl - ceil(log2 n) >= 1.  Bit-identical to the loop of
 * mkckks_cheb_tensor_batch + mkckks_relinearize_batch + mkckks_rescale_batch.  d_out overlaps neither d_u nor the key. */
int mkckks_cheb_ladder_batch(mkckks_ctx *c, const uint64_t *d_u, const uint64_t *d_rlk, uint64_t *d_out, uint32_t n_ct,
                             uint32_t nl, uint32_t n, double scale_in, uint32_t *h_nl_out, double *h_scale_out);
/* Host-only and pure (works on a device = -1 context).  h_coef: the degree + 1 series coefficients c_0 .. c_d; nl and
 * scale_in are those of u.  h_w (HOST, double[G][B]) receives w_{j,i}, *scale_out receives S_out.  Refusals as
 * mkckks_poly_weights. */
int mkckks_cheb_weights(const mkckks_ctx *c, const double *h_coef, uint32_t degree, uint32_t nl, double scale_in,
                        double *h_w, double *scale_out);
/* The whole algorithm, workspace-chunked like mkckks_poly_eval_batch: d_out u64[n_ct][2][nl_out][N] = p(alpha d_ct + beta),
 * scale *scale_out (nullable) = S_out.  Bit-identical to mkckks_affine_batch + mkckks_rescale_batch (unless (a, b) is
 * (-1, 1)) + mkckks_cheb_ladder_batch (on u with n = B, then on y = its T_B with n = G - 1) + mkckks_cheb_weights +
 * mkckks_poly_tensor_batch + mkckks_relinearize_batch + mkckks_rescale_batch twice.  d_ct is not modified; d_out overlaps
 * neither d_ct nor the key. */
int mkckks_cheb_eval_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_rlk, const double *h_coef,
                           uint32_t degree, double a, double b, uint64_t *d_out, uint32_t n_ct, uint32_t nl,
                           double scale_in, double *scale_out);

/* ---- cc->Encrypt(pk, pt)  (client/src/encryptModelWeights.cpp:83,91,110) --
 * d_pt u64[n_ct][nl][N] encoded plaintexts (EVALUATION); v int8[n_ct][N];
 * e0,e1 int32[n_ct][N]; out u64[n_ct][2][nl][N]. */
int mkckks_encrypt_batch(mkckks_ctx *c, const uint64_t *d_pk, const uint64_t *d_pt, const int8_t *d_v,
                         const int32_t *d_e0, const int32_t *d_e1, uint64_t *d_ct, uint32_t n_ct, uint32_t nl);

/* ---- cc->ReEncrypt(ct, reKey, publicKey), first half  (changeCipherDomain.cpp:74 with the third argument) ------
 * HRA-secure proxy re-encryption (Cohen 2019): upstream's PREBase::ReEncrypt(ct, evalKey, publicKey) re-randomises
 * the ciphertext with an encryption of zero under the SOURCE domain's public key (EncryptZeroCore, errors from a wide
 * "flooding" Gaussian) before the key switch.  This is that re-randomisation; for t < n_ct, i < nl:
 *     out[t][0][i] = ct[t][0][i] + pk[0][i] * NTT_i(v_t) + NTT_i(e0_t)   mod q_i
 *     out[t][1][i] = ct[t][1][i] + pk[1][i] * NTT_i(v_t) + NTT_i(e1_t)   mod q_i
 * d_ct u64[n_ct][2][nl_in][N], read at its first nl limbs (a lower level is a prefix, as in mkckks_compress_batch);
 * d_pk u64[2][D][N] addressed by limb id; d_v int8[n_ct][N] ternary; d_e0 / d_e1 int64[n_ct][N] with |e| < 2^62 (the
 * caller's contract; mkckks_sample_gauss_wide keeps it); d_out u64[n_ct][2][nl][N].  d_out == d_ct is allowed exactly
 * when nl_in == nl (in place); any other overlap is MKCKKS_E_INVALID.  1 <= nl <= nl_in <= L; n_ct == 0 is a no-op.
 * The randomness is the caller's, as in mkckks_encrypt_batch: hosts draw it with mkckks_sample_ternary /
 * mkckks_sample_gauss_wide under an OS-drawn key of their own.  Outputs are canonical residues: the result equals
 * exact integer arithmetic word for word.
 * Consequence: ReEncrypt(ct, evk, pk) = mkckks_rerandomize_batch followed by any of the re-encryption entry points
 * (mkckks_reencrypt_batch, _sum_batch, _fanout_batch, _fanout_compact_batch).
 * Noise rule: under the key of pk the mask decrypts to e0 + e1 * s (+ the key's own e * v, below 0.3 % at sigma >= 2^6):
 * standard deviation sigma * sqrt(1 + h) per coefficient, h the number of non-zero coefficients of the ternary secret,
 * ~ sigma * sqrt(2N/3).  Keep it well below the ciphertext's own noise at its scale (at noiseScaleDeg 2, scale ~ 2^(2p),
 * sigma up to 2^28 costs no measurable precision at p = 40 and 50). */
int mkckks_rerandomize_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_pk, const int8_t *d_v,
                             const int64_t *d_e0, const int64_t *d_e1, uint64_t *d_out, uint32_t n_ct, uint32_t nl_in,
                             uint32_t nl);

/* ---- seeded secret-key ciphertexts (new: half the bytes of a client ciphertext) ---------------------------------
 * A seeded ciphertext is (c0, seed): c1 = a is not sent but regenerated from a 32-byte ChaCha20 key K and a u32
 * stream id sid as
 *     a := mkckks_sample_uniform(d, n_polys = 1, nl, with_p = 0, K, sid)
 * i.e. limb i, coefficient j is word i*N + j of stream sid, taken as EVALUATION (rejection as k_sample_uniform: attempt
 * counter in nonce word 2, at most 64 attempts).  A lower level is a prefix of limbs.  Security rules: K reveals a
 * only (a is public in RLWE); K must key nothing else (sharing it with the stream of e would reveal e and, with it,
 * s); a client choosing its own K gains nothing, it could send any c1 anyway.
 * cc->Encrypt(privateKey, pt) with a seeded a (replaces cc->Encrypt(publicKey, pt), encryptModelWeights.cpp:83,91,110):
 * item t: a = stream (h_seed32, stream_base + t); d_c0 out u64[n_ct][nl][N] = pt + NTT(e) - a*s mod q_i;
 * d_sk u64[D][N] EVALUATION (first nl limbs); d_pt u64[n_ct][nl][N] EVALUATION; d_e int32[n_ct][N] COEFFICIENT.
 * stream_base + n_ct - 1 must fit in 32 bits.  n_ct == 0 is a no-op. */
int mkckks_encrypt_seeded_batch(mkckks_ctx *c, const uint64_t *d_sk, const uint64_t *d_pt, const int32_t *d_e,
                                uint64_t *d_c0, uint32_t n_ct, uint32_t nl, const uint8_t *h_seed32,
                                uint32_t stream_base);
/* new: rebuild c1 of seeded ciphertexts in place.  d_ct u64[n_ct][2][nl][N] (component 0 untouched);
 * h_seeds32 [n_ct][32] and h_stream_ids [n_ct] are HOST arrays, read before return.  Any n_ct (the keys travel in the
 * kernel arguments, 64 ciphertexts per launch); n_ct == 0 is a no-op.  What the server hosts call after the upload of
 * c0 and before mkckks_reencrypt_sum_batch / mkckks_eval_sum_batch. */
int mkckks_expand_seeded_batch(mkckks_ctx *c, uint64_t *d_ct, uint32_t n_ct, uint32_t nl,
                               const uint8_t *h_seeds32, const uint32_t *h_stream_ids);
/* scaled real coefficient vectors -> residues in EVALUATION format over nl limbs
 * (the integer half of CKKSPackedEncoding::Encode; the fp64 canonical embedding
 * runs on the GPU too: mkckks_encode_batch).  Each double (|x| < 2^120) is
 * rounded to the nearest integer (ties away from zero) and that integer is
 * reduced exactly per limb: coef double[n][N] -> u64[n][nl][N]. */
int mkckks_lift_ntt_batch(mkckks_ctx *c, const double *d_coef, uint64_t *d_out, uint32_t n, uint32_t nl);

/* ---- cc->MakeCKKSPackedPlaintext(values)  (encryptModelWeights.cpp:82,90,109) --
 * CKKSPackedEncoding::Encode, full packing: d_vals double[n][N/2] real slot values
 * (zero padded by the caller) -> inverse canonical embedding (fp64 special FFT), x scale,
 * round, residues, NTT -> d_pt u64[n][nl][N].  scale: the plaintext's scaling factor
 * (FLEXIBLEAUTOEXT level 0: mkckks_scaling_factor(ctx, 0, big=1)). */
int mkckks_encode_batch(mkckks_ctx *c, const double *d_vals, uint64_t *d_pt, uint32_t n, uint32_t nl, double scale);
/* ---- pt->GetRealPackedValue()  (decryptModelWeights.cpp:83,92,109) ------------
 * CRT interpolation of d_m u64[n][nl][N] (output of mkckks_decrypt_batch), / scale,
 * canonical embedding -> d_vals double[n][N/2]: the exact embedding, without upstream
 * Decode's noise estimate and flooding (those: mkckks_decode_flood_batch).
 * nl <= 32.  The centred lift is accumulated in fp64 (upstream and the oracle use long double), so the decrypted
 * integers must stay below the largest double: any |x| <= Q / 2 up to nl = 20 with 50-bit scaling limbs (Q ~ 2^980);
 * at deeper levels (Q ~ 2^1580 at nl = 32) only |x| < 2^1000 is supported -- a message at its scale, a long way below
 * Q / 2 -- and a coefficient near Q / 2 decodes to +-inf where the oracle still returns a finite value. */
int mkckks_decode_batch(mkckks_ctx *c, const uint64_t *d_m, double *d_vals, uint32_t n, uint32_t nl, double scale);
/* ---- pt->GetRealPackedValue() after cc->Decrypt with upstream's decode-time noise flooding
 * (CKKSPackedEncoding::Decode as reached from decryptModelWeights.cpp:81-83,90-92,108-110; the defence against
 * key recovery from shared CKKS decryptions, Li-Micciancio, ePrint 2022/816).  Layout and limits of
 * mkckks_decode_batch; full packing (N/2 slots).  Per item, with m the centred lift of d_m in integer units,
 * p = scaling_bits and u = scale / 2^p (upstream Decode brings the scaling factor to 2^p before it estimates; u = 1
 * when scale = 2^p; a noiseScaleDeg-2 aggregate decoded at scale ~ 2^(2p) has u ~ 2^p):
 *   m'_0 = m_0, m'_j = -m_{N-j}                      (coefficients of m(X^-1) mod X^N + 1)
 *   d_j = m_j + m_{N-j}, j = 1..N-1;  mu = sum d / (N-1);
 *   sigma = sqrt(sum (d - mu)^2 / (N-2)) / u         (fp64, fixed reduction order: the bits repeat)
 *   log2 sigma > p - 5  -> the item fails ("The decryption failed because the approximation error is too high.
 *                          Check the parameters.")
 *   sigma_flood = sqrt(2) * max(sigma, sqrt(N) / 8)  (upstream CKKS_M_FACTOR = 1)
 *   work position i < N/2: re = ((m_i + m'_i) / 2 + u sigma_flood z0) / scale,
 *                          im = ((m_{i+N/2} + m'_{i+N/2}) / 2 + u sigma_flood z1) / scale, then the embedding.
 * z0, z1: N(0,1) by Box-Muller from the ChaCha20 stream `stream_id` under h_key32 (32 HOST bytes; give flooding a
 * key of its own): a pure function of (key, stream_id, item, i); mapping in csrc/sampler_kernels.hpp.
 * Writes every output, then returns MKCKKS_E_PRECISION if any item failed (the first one is named in
 * mkckks_last_error()).  h_log2_sigma (nullable, HOST, [n]) gets log2 sigma of every item (before the floor).
 * Synchronous: downloads the per-item estimates once, which synchronises the context's stream. */
int mkckks_decode_flood_batch(mkckks_ctx *c, const uint64_t *d_m, double *d_vals, uint32_t n, uint32_t nl,
                              double scale, const uint8_t *h_key32, uint32_t stream_id,
                              double *h_log2_sigma /* nullable, [n] */);

/* ---- cc->Decrypt(sk, ct, &pt)  (client/src/decryptModelWeights.cpp:81,90,108)
 * DecryptCore: m = INTT(c0 + c1*s); d_m out u64[n_ct][nl][N] (COEFFICIENT).
 * CRT interpolation + Decode follow on the GPU: mkckks_decode_batch (exact) or mkckks_decode_flood_batch
 * (upstream's decode-time noise flooding). */
int mkckks_decrypt_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_sk, uint64_t *d_m,
                         uint32_t n_ct, uint32_t nl);

/* ==== threshold decryption: a joint public key whose secret nobody holds ======================================
 * The reference enables the capability (server/src/genCC.cpp:73, Enable(MULTIPARTY)) and never calls it; its clients'
 * uploads are re-encrypted into ONE client's domain, whose key then opens every individual upload.  With a joint key
 * pk = (sum b_i, a), secret sum s_i, the aggregate is opened by n partial decryptions that are summed.
 *
 * ---- cc->MultipartyKeyGen(prevPublicKey) -------------------------------------------------------------------------
 * The joining key generation: for all D limbs
 *     pk[0] = pk_prev[0] + NTT(e) - pk_prev[1] * NTT(s),   pk[1] = pk_prev[1];   sk = NTT(s) as in mkckks_keygen.
 * d_pk_prev u64[2][D][N] (EVALUATION); s ternary int8[N], e int32[N] (COEFFICIENT), the caller's randomness as in
 * mkckks_keygen; d_pk out u64[2][D][N], d_sk out u64[D][N].  d_pk may be d_pk_prev (in place); no other overlap.  The
 * first party calls mkckks_keygen, every further party this with its predecessor's public key; the last party's
 * public key is the joint key.  mkckks_rekeygen takes it like any public key (own domain -> joint domain), and so does
 * mkckks_encrypt_batch. */
int mkckks_keygen_join(mkckks_ctx *c, const uint64_t *d_pk_prev, const int8_t *d_s, const int32_t *d_e, uint64_t *d_pk,
                       uint64_t *d_sk);
/* ---- cc->MultipartyDecryptMain (lead = 0) / cc->MultipartyDecryptLead (lead != 0) --------------------------------
 * One party's share of a decryption under the joint key; for t < n_ct, i < nl:
 *     share[t][i] = INTT_i( ct[t][1][i] * sk[i] + (lead ? ct[t][0][i] : 0) ) + (e[t] mod q_i)     mod q_i
 * in COEFFICIENT format, canonical residues (the result equals exact integer arithmetic word for word).
 * d_ct u64[n_ct][2][nl_in][N] read at its first nl limbs (a lower level is a prefix, as in mkckks_rerandomize_batch);
 * d_sk u64[D][N] addressed by limb id (the party's own sk of mkckks_keygen / mkckks_keygen_join); d_e int64[n_ct][N]
 * smudging errors with |e| < 2^62 (the caller's contract; mkckks_sample_gauss_wide keeps it); d_share out
 * u64[n_ct][nl][N].  Every pointer is required, d_e included: a share without smudging gives c1 * s_i away, so there
 * is no noiseless mode (tests pass zeros).  1 <= nl <= nl_in <= L; d_share must not overlap d_ct (MKCKKS_E_INVALID);
 * n_ct == 0 is a no-op.  Upstream adds the noise in EVALUATION and transforms after the fusion; by linearity mod q_i
 * the two orders give the same bits.  Bit-identical to mkckks_rerandomize_batch(v = 0, e0 = e, e1 = 0) followed by
 * mkckks_decrypt_batch (lead), or the same on a copy whose component 0 is zero (lead = 0).
 * Noise rule: n shares add sum_i e_i to the plaintext polynomial; the real part of slot k receives
 * sum_j e_j cos(j theta_k), so the decoded values carry a Gaussian error of standard deviation
 * sigma * sqrt(n * N / 2) / scale.  At noise degree 2 (scale ~ 2^(2p)) that is nothing for any sigma of the sampler; at
 * scale 2^p it is the price of the statistical security sigma buys.
 * d_sk may also be a key share u64[L][N] (lambda * sigma_j of the t-of-n section below): both paths, the fused kernels and
 * the composition under the library switches, read limbs 0 .. nl - 1 of d_sk only.
 * Security rules: n-of-n -- the server plus any n - 1 parties learn the aggregate only, and a party that does not
 * answer blocks the round unless the key was shared t-of-n ("t-of-n threshold decryption" below: any t parties
 * decrypt).  ONE share per ciphertext per party, with fresh errors each time:
 * two shares of one ciphertext average the smudging away.  The key the smudging errors are drawn under keys nothing
 * else. */
int mkckks_partial_decrypt_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_sk, const int64_t *d_e,
                                 uint64_t *d_share, uint32_t n_ct, uint32_t nl_in, uint32_t nl, int lead);
/* ---- cc->MultipartyDecryptFusion ---------------------------------------------------------------------------------
 * m = sum_p shares[p] mod q_i: d_shares u64[n_parties][n_ct][nl][N] -> d_m u64[n_ct][nl][N], the layout
 * mkckks_decrypt_batch writes, so mkckks_decode_batch / mkckks_decode_flood_batch follow unchanged.  n_parties >= 1;
 * d_m may alias shares[0] (d_m == d_shares), any other overlap is MKCKKS_E_INVALID; n_ct == 0 is a no-op.  The
 * caller guarantees that exactly ONE share was made with lead != 0 (the hosts check it from the share headers). */
int mkckks_fuse_shares_batch(mkckks_ctx *c, const uint64_t *d_shares, uint64_t *d_m, uint32_t n_parties, uint32_t n_ct,
                             uint32_t nl);
/* ---- collective public-key switch: deliver the joint-key aggregate instead of opening it ----------------------------
 * (Mouchet et al., "Multiparty homomorphic encryption from ring-learning-with-errors", the PCKS protocol.)  Each party
 * adds to its c1 * s_p term an encryption of zero under the RECIPIENT's public key pk = (b, a); for t < n_ct, i < nl, in
 * EVALUATION form with canonical residues:
 *     share[t][0][i] = ct[t][1][i] * sk[i] + (lead ? ct[t][0][i] : 0) + pk[0][i] * NTT_i(v_t) + NTT_i(e0_t)   mod q_i
 *     share[t][1][i] =                                                  pk[1][i] * NTT_i(v_t) + NTT_i(e1_t)   mod q_i
 * Layouts and contracts of the two entry points it merges: d_ct u64[n_ct][2][nl_in][N] read at its first nl limbs (a
 * lower level is a prefix); d_sk u64[D][N] addressed by limb id, limbs < nl only, so a key share u64[L][N]
 * (lambda_j * sigma_j of the t-of-n section below) is a key; d_pk u64[2][D][N] the recipient's public key, addressed by
 * limb id; d_v int8[n_ct][N] ternary; d_e0 / d_e1 int64[n_ct][N] with |e| < 2^62 (mkckks_sample_gauss_wide keeps it);
 * d_share out u64[n_ct][2][nl][N].  Every pointer is required.  1 <= nl <= nl_in <= L; d_share must not overlap d_ct
 * (MKCKKS_E_INVALID); n_ct == 0 is a no-op; a host-only context returns MKCKKS_E_NODEVICE.
 * Fusion needs no entry point of its own: the component-wise sum of the parties' shares is mkckks_eval_sum_batch, and
 * the result is decrypted by mkckks_decrypt_batch under the recipient's secret key.
 * The algebra: with S = sum_p s_p the joint secret, U = sum_p v_p, E0 = sum_p e0_p, E1 = sum_p e1_p and exactly one lead,
 *     sum_p share_p = (c0 + c1 * S + b * U + E0,  a * U + E1),
 * a ciphertext under the recipient's key s_out (b = -a * s_out + e_pk): it decrypts to m + e_agg + U * e_pk + E0 + E1 * s_out.
 * Nobody on the way sees m: c1 * S exists only masked by b * U.
 * Noise rule: per-coefficient variance n * (sigma0^2 + h * sigma1^2 + (2N/3) * sigma_pk^2) for n parties, sigma0 / sigma1
 * the deviations of e0 / e1, sigma_pk that of the recipient key's error and h the number of non-zero coefficients of
 * s_out; the decoded values carry a Gaussian error of standard deviation sqrt(that * N / 2) / scale.  With a smudging
 * sigma0 >= 2^10 and the standard sigma1 this is mkckks_partial_decrypt_batch's rule sigma0 * sqrt(n * N / 2) / scale to
 * within 10^-3.
 * Composition equality: the share is bit-identical to, in this order, mkckks_partial_decrypt_batch(e = 0),
 * mkckks_ntt_forward_batch, and mkckks_rerandomize_batch on the ciphertext whose component 0 is that result and whose
 * component 1 is zero -- at three times the passes, and with the unsmudged INTT(c1 * s_p) in memory on the way.
 * Security rules: e0 is the SMUDGING error (wide: mkckks_sample_gauss_wide at the deployment's sigma, as in
 * mkckks_partial_decrypt_batch), e1 an ordinary encryption error (the scheme's standard sigma).  The recipient can compute
 * share0 + share1 * s_out = c1 * s_p (+ c0) + smudge (+ small) for every party: the view mkckks_partial_decrypt_batch
 * gives everybody.  So "ONE share per ciphertext per party" becomes a budget: r recipients of one aggregate receive r
 * independently smudged copies of c1 * s_p, which average the smudging down by sqrt(r) -- add log2(r) / 2 bits of
 * smudging for r recipients.  Fresh (v, e0, e1) per call, drawn under keys that key nothing else.  With key shares, all
 * shares that are summed must have been made with the SAME set T and for the SAME recipient, or they sum to noise. */
int mkckks_switch_share_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_sk, const uint64_t *d_pk,
                              const int8_t *d_v, const int64_t *d_e0, const int64_t *d_e1, uint64_t *d_share, uint32_t n_ct,
                              uint32_t nl_in, uint32_t nl, int lead);

/* ==== t-of-n threshold decryption: Shamir shares of the joint secret ============================================
 * (Mouchet et al., "An efficient threshold access-structure for RLWE-based multiparty homomorphic encryption".)
 * Once per key epoch party i shares its own sk_i among the n parties with threshold t, limb by limb and coefficient
 * by coefficient over Z_{q_l}, in EVALUATION form; party j sums what it received: sigma_j = sum_i f_i(j) = F(j), where
 * F = sum_i f_i has degree t - 1 and F(0) = sum_i sk_i, the joint secret.  In a round any set T of at least t parties
 * decrypts: party j in T passes lambda_j^T * sigma_j to mkckks_partial_decrypt_batch in the place of its secret key,
 * lambda_j^T = prod_{m in T, m != j} m (m - j)^-1 mod q_l the Lagrange coefficient at 0, so that
 * sum_{j in T} lambda_j sigma_j = sum_i sk_i (mod q_l); smudging and mkckks_fuse_shares_batch are unchanged.  The
 * Lagrange factor multiplies the key share, not the error: the noise rule above holds with n replaced by |T|.
 * Rules: key shares are SECRETS and travel over private, authenticated channels, which this library does not provide;
 * dealers are honest-but-curious (no verifiable sharing, no proactive refresh, no resharing to a new party); any t
 * parties together hold the joint secret; ONE decryption share per ciphertext per party still holds; all shares that
 * are fused must have been made with the SAME set T, or they fuse to noise -- the fusion cannot tell.
 *
 * ---- the dealer's step ---------------------------------------------------------------------------------------------
 * For p < n_parties, i < nl, every coefficient c:
 *     shares[p][i][c] = sk[i][c] + sum_{k=1}^{threshold-1} r_k[i][c] * (p + 1)^k     mod q_i
 * Party indices are 1-based evaluation points: shares[p] goes to party p + 1.  r_k is BY DEFINITION the polynomial
 *     mkckks_sample_uniform(d, n_polys = 1, nl, with_p = 0, h_key32, stream_id + k - 1)
 * (limb i, coefficient c = word i*N + c of the stream, rejection as there: the definition seeded ciphertexts use), but it
 * is never written to memory: r_k together with one share gives sk away.  Key rule: h_key32 keys nothing else -- one
 * fresh OS-drawn key per call.  d_sk u64[D][N], limbs 0 .. nl - 1 read; d_shares out u64[n_parties][nl][N], canonical
 * residues equal to exact integer arithmetic word for word.  1 <= threshold <= n_parties <= MKCKKS_MAX_PARTIES and
 * 1 <= nl <= L; threshold = 1 is the degenerate sharing (every share is sk).  MKCKKS_E_INVALID if
 * stream_id + threshold - 1 does not fit in 32 bits, or if d_shares overlaps the limbs of d_sk that are read. */
#define MKCKKS_MAX_PARTIES 64
int mkckks_share_key(mkckks_ctx *c, const uint64_t *d_sk, uint64_t *d_shares, uint32_t nl, uint32_t n_parties,
                     uint32_t threshold, const uint8_t *h_key32, uint32_t stream_id);
/* ---- weighted sum of key shares ------------------------------------------------------------------------------------
 *     out[i][c] = sum_{j<m} h_w[j][i] * in[j][i][c]     mod q_i,   canonical
 * d_in u64[m][nl][N]; h_w HOST u64[m][nl], read before return, every weight below its modulus (else MKCKKS_E_INVALID);
 * d_out u64[nl][N].  m >= 1, 1 <= nl <= L.  d_out may be d_in (in[0]); any other overlap is MKCKKS_E_INVALID.  Three
 * uses: party j's sum sigma_j of the shares it received (all weights 1), the per-round lambda * sigma_j (m = 1, weights
 * from mkckks_lagrange_at_zero), and the recovery of F at any point. */
int mkckks_combine_key_shares(mkckks_ctx *c, const uint64_t *d_in, const uint64_t *h_w, uint64_t *d_out, uint32_t m,
                              uint32_t nl);
/* ---- Lagrange coefficients at 0 (host only: works on a device = -1 context) ----------------------------------------
 * h_out[a][l] = lambda of h_parties[a] within the set h_parties[0 .. n_active), mod q_l, for the L limbs of Q.
 * h_parties are 1-based party indices.  An index of 0 or above MKCKKS_MAX_PARTIES, a duplicate and n_active == 0 are
 * each MKCKKS_E_INVALID. */
int mkckks_lagrange_at_zero(const mkckks_ctx *c, const uint32_t *h_parties, uint32_t n_active, uint64_t *h_out);

/* ==== collective evaluation keys of a JOINT key: cc->MultiEvalAtIndexKeyGen / cc->MultiEvalSumKeyGen +
 * cc->MultiAddEvalAutomorphismKeys, and cc->MultiKeySwitchGen + cc->MultiAddEvalKeys + cc->MultiMultEvalKey +
 * cc->MultiAddEvalMultKeys =========================================================================================
 * Upstream CryptoContext calls the reference (built with MULTIPARTY) never makes.  With a joint key pk = (sum b_p, a),
 * S = sum_p s_p, nobody can call mkckks_galois_keygen or mkckks_relin_keygen on S.  Every step below is linear in what
 * the parties already hold; g_j is the gadget of digit j ((P mod q_i) on digit j's own limbs, 0 elsewhere).
 *   Galois key for g, ONE round: party p computes mkckks_galois_keygen(s_p, pk_joint, u, e0, e1, g): a public-key
 *     encryption of P g_j sigma_g(s_p) under the joint key.  mkckks_evk_sum of the n shares encrypts
 *     P g_j sigma_g(S): a Galois key of the joint key.  Noise: n times one key's.
 *   Relinearisation key, TWO rounds.  Round 1: party p computes mkckks_rekeygen(s_p, pk_joint, ...) ("own domain ->
 *     joint domain"); the sum K1 satisfies K1[j][0] + K1[j][1] S = P g_j S + n1, n1 = e_pk U + E0 + E1 S.  Round 2:
 *     party p computes mkckks_relin_share(K1, sk_p, fresh e0, e1); the sum is (S K1[j][0] + E0', S K1[j][1] + E1'),
 *     which decrypts under S to P g_j S^2 + S n1 + E0' + E1' S: a relinearisation key of the joint key.
 *   Noise rule: the key error is dominated by S n1, a product of two polynomials: its standard deviation is about
 *     sqrt(N * 2n/3) times that of n1 (S has n ternary summands of variance 2/3 per coefficient).  The measured effect
 *     on decoded values is in DESIGN.md ("collective evaluation keys").
 * The result is an ordinary u64[beta][2][D][N] key: mkckks_rotate_batch, mkckks_slot_sum_batch,
 * mkckks_relinearize_batch and mkckks_mult_relin_batch take it unchanged.
 * Security rules.  A share holds no secret under RLWE (it is a public-key encryption, or K1 times a secret plus fresh
 * error) and may be sent in the clear.  A single share, or a sum of FEWER than all n, used as a key gives noise and no
 * error: the library cannot tell.  Every call takes FRESH errors (and u); a repeated error cancels in the difference of
 * two shares.  ALL n parties of the key epoch take part, once per epoch, while all are present: the t-of-n key shares
 * of mkckks_share_key play no role here.
 * Refusals, decided before a device is asked for: MKCKKS_E_INVALID for null pointers, a party count outside
 * [1, MKCKKS_MAX_PARTIES], an overlap other than the one each call names, and key arrays that are not 16-byte aligned;
 * a host-only context gives MKCKKS_E_NODEVICE.
 *
 * (cc->MultiAddEvalKeys / MultiAddEvalAutomorphismKeys / MultiAddEvalMultKeys) d_out[k] = sum over p of d_in[p][k] mod
 * q_i on ALL D limbs (mkckks_eval_sum_batch stops at L); d_in u64[n_parties][n_keys][beta][2][D][N], d_out
 * u64[n_keys][beta][2][D][N], canonical, equal to exact integer arithmetic word for word at any residues (64 terms of
 * q - 1 included).  d_out may be d_in (the first party's keys); any other overlap is refused.  n_keys = 0 is a no-op. */
int mkckks_evk_sum(mkckks_ctx *c, const uint64_t *d_in, uint64_t *d_out, uint32_t n_parties, uint32_t n_keys);
/* (cc->MultiMultEvalKey) round 2 of the relinearisation key: for every digit j, component c and ALL D limbs i (the Q
 * limbs and the K limbs of P)  d_share[j][c][i] = d_key1[j][c][i] * d_sk[i] + NTT_i(e_c[j]) mod q_i, canonical.
 * d_key1, d_share u64[beta][2][D][N]; d_sk u64[D][N] as mkckks_keygen / mkckks_keygen_join write it (all D limbs are
 * read); d_e0, d_e1 int32[beta][N] in COEFFICIENT form (the contract of mkckks_rekeygen).  d_share may be d_key1; any
 * other overlap is refused.  One fused column + row kernel pair where the ring size has them, else the composition of
 * lift, transform and multiply-add; all paths give the same bits. */
int mkckks_relin_share(mkckks_ctx *c, const uint64_t *d_key1, const uint64_t *d_sk, const int32_t *d_e0, const int32_t *d_e1,
                       uint64_t *d_share);

/* ---- multi-GPU aggregation step (new) -----------------------
 * after an RCCL ncclSum over uint64 of `n_terms` canonical residues per word,
 * reduce every word mod its limb modulus: d_ct u64[n_ct][2][nl][N] in place. */
int mkckks_reduce_mod_batch(mkckks_ctx *c, uint64_t *d_ct, uint32_t n_ct, uint32_t nl, uint32_t n_terms);

/* ---- RCCL exchange step behind the C-ABI (SURVEY.md 8b export list, 8e.2) ----
 * Replaces the serial per-client loop of the reference's server (orchestration/server_fns.sh:62-80,
 * orchestration/run.sh:37-43: one changeCipherDomain per client, then one aggregateEncryptedWeights):
 * every GPU re-encrypts and sums ITS clients (mkckks_reencrypt_sum_batch), then
 *   d_shard[b] = ( sum over ranks r of d_partial_r[rank * n_ct_shard + b] )  coefficient-wise mod q_i
 * as ONE ncclReduceScatter(ncclUint64, ncclSum) over xGMI + a word-wise reduction (n_ranks <= 8 canonical residues
 * below 2^61 cannot wrap 2^64).  d_partial: u64[n_ranks * n_ct_shard][2][nl][N] on every rank; d_shard:
 * u64[n_ct_shard][2][nl][N].  Enqueued on the context's stream.  `comm` is an ncclComm_t (as void*): from
 * mkckks_comm_create, or any communicator of the RCCL this process carries whose rank is bound to the context's
 * device.  librccl.so.1 is resolved at first use (dlopen by SONAME: a process that already loaded an RCCL, e.g.
 * PyTorch's, keeps that one); mkckks_comm_library() names the file.
 * Communicator bootstrap: rank 0 calls mkckks_comm_unique_id, ships the MKCKKS_COMM_ID_BYTES bytes to the other
 * ranks by any side channel, every rank calls mkckks_comm_create (collective: ncclCommInitRank). */
#define MKCKKS_COMM_ID_BYTES 128
int mkckks_comm_unique_id(void *h_id_out /* MKCKKS_COMM_ID_BYTES */);
int mkckks_comm_create(mkckks_ctx *c, const void *h_id, int n_ranks, int rank, void **comm_out);
int mkckks_comm_destroy(mkckks_ctx *c, void *comm);
int mkckks_reduce_scatter_sum_mod(mkckks_ctx *c, void *comm, const uint64_t *d_partial, uint64_t *d_shard,
                                  uint32_t n_ct_shard, uint32_t nl, uint32_t n_ranks);
const char *mkckks_comm_library(void);

/* ---- diagnostics: in-kernel phase stamps of a -DMK_STAMP=1 build created under MKCKKS_STAMPS=1 (tools/stamps.py);
 * h_out: 2^20 words; *n_out = words written, 0 in a product build */
int mkckks_debug_stamps(mkckks_ctx *c, unsigned long long *h_out, uint32_t region, size_t *n_out);

/* ---- diagnostics for tests: run ONE arithmetic primitive of the library per element ("known-answer hook" of the
 * modular arithmetic).  in: u64[n_in(op)][count] operand planes, out: u64[n_out(op)][count]; doubles travel as bit
 * patterns; element i of every output plane depends on element i of the input planes only.  On a device context the
 * pointers are device pointers and the op runs as one element-wise kernel on the context's stream, through the DEVICE
 * form of the primitive; on a device = -1 context they are host pointers and the HOST form runs (the fp64 class has a
 * device form only: MKCKKS_E_NODEVICE there).  q: any odd modulus with 2^17 < q < 2^60, need not belong to the context
 * nor be prime; the reduction constants are built from it as the context's are.  Twiddle planes (always the LAST
 * planes of `in`) hold the residue w < q only: the companion (Shoup: floor(w 2^64 / q); pseudo-Mersenne: the pair
 * w << t, (w 2^32 mod q) << t; fp64: (double) w, w / q) is made by the code that fills the NTT tables.
 * MKCKKS_E_INVALID: unknown op, an fp64 op with q >= 5 * 2^48, a pseudo-Mersenne op with a q that is not 2^k - c with
 * c <= 2^(k-34) and 40 <= k <= 60, a twiddle >= q, overlapping in / out.  count == 0 is a no-op.
 * Operands outside the domain a primitive documents give unspecified words (never a fault).
 *
 * op                    in planes                         out planes
 * CSUB                  x, m                              x - m if x >= m else x          (x, m < 2^63)
 * ADD_MOD / SUB_MOD     a, b                              canonical                       (a, b < q)
 * SHOUP_LAZY / _MUL     a, w                              [0,2q) / canonical              (any a)
 * MUL_MOD               a, b                              canonical                       (a, b < q)
 * BARRETT_REDUCE128     hi, lo                            canonical                       (hi:lo < 2^(k+62))
 * REDUCE_WIDE           hi, lo                            canonical                       (hi:lo < 2^124)
 * REDUCE_WORD           x                                 canonical
 * REDUCE_COLS_LAZY / _COLS   c0, c1, c2                   [0,4q) / canonical              (<= 4 products per column)
 * REDUCE_COLS4          c0, c1a, c1b, c2                  canonical                       (<= 8 products per column)
 * MAC128 / MAC128_SPLIT hi, lo, a, b                      hi', lo' = hi:lo + a b
 * CT_BUTTERFLY_C4 / _NC, GS_BUTTERFLY      x, y, w        x', y'
 * CANON8                v                                 canonical                       (v < 8q)
 * RADIX_FORWARD4 / RADIX_INVERSE4          x[16], w[15]   x'[16]  (one register round; w[(1 << s) - 1 + g])
 * PM_FOLD               x                                 < U + 2^30
 * PM_LAZY               a, w                              < 2.375U                        (a < 8U)
 * PM_REDUCE128          hi, lo                            canonical                       (hi:lo < 2^(2k+6))
 * PM_REDUCE_COLS        c0, c1, c2                        < 2.1U
 * CT_BUTTERFLY_PM_F / _PM_N, GS_BUTTERFLY_PM   x, y, w    x', y'
 * RADIX_FORWARD_PM4 / RADIX_INVERSE_PM4    x[16], w[15]   x'[16]
 * FP_MULMOD             y, w                              double
 * FP_REDUCE             x                                 double
 * FP_TO_CANONICAL       x                                 u64
 * FP_MULMOD_ANY         y, e  (both doubles)              double
 * U52_TO_DOUBLE         v (u64 < 2^52)                    double
 * SPLIT30_D             canonical double                  low 30 bits, bits 30.. (the conversion kernels' split)
 * CT_BUTTERFLY_FP / _FP_NR, GS_BUTTERFLY_FP    x, y, w    x', y'  (doubles)
 * RADIX_FORWARD_FP4 / RADIX_INVERSE_FP4    x[16], w[15]   x'[16]  (doubles) */
#define MKCKKS_OP_CSUB 0
#define MKCKKS_OP_ADD_MOD 1
#define MKCKKS_OP_SUB_MOD 2
#define MKCKKS_OP_SHOUP_LAZY 3
#define MKCKKS_OP_SHOUP_MUL 4
#define MKCKKS_OP_MUL_MOD 5
#define MKCKKS_OP_BARRETT_REDUCE128 6
#define MKCKKS_OP_REDUCE_WIDE 7
#define MKCKKS_OP_REDUCE_WORD 8
#define MKCKKS_OP_REDUCE_COLS_LAZY 9
#define MKCKKS_OP_REDUCE_COLS 10
#define MKCKKS_OP_REDUCE_COLS4 11
#define MKCKKS_OP_MAC128 12
#define MKCKKS_OP_MAC128_SPLIT 13
#define MKCKKS_OP_CT_BUTTERFLY_C4 14
#define MKCKKS_OP_CT_BUTTERFLY_NC 15
#define MKCKKS_OP_GS_BUTTERFLY 16
#define MKCKKS_OP_CANON8 17
#define MKCKKS_OP_RADIX_FORWARD4 18
#define MKCKKS_OP_RADIX_INVERSE4 19
#define MKCKKS_OP_PM_FOLD 20
#define MKCKKS_OP_PM_LAZY 21
#define MKCKKS_OP_PM_REDUCE128 22
#define MKCKKS_OP_PM_REDUCE_COLS 23
#define MKCKKS_OP_CT_BUTTERFLY_PM_F 24
#define MKCKKS_OP_CT_BUTTERFLY_PM_N 25
#define MKCKKS_OP_GS_BUTTERFLY_PM 26
#define MKCKKS_OP_RADIX_FORWARD_PM4 27
#define MKCKKS_OP_RADIX_INVERSE_PM4 28
#define MKCKKS_OP_FP_MULMOD 29
#define MKCKKS_OP_FP_REDUCE 30
#define MKCKKS_OP_FP_TO_CANONICAL 31
#define MKCKKS_OP_FP_MULMOD_ANY 32
#define MKCKKS_OP_U52_TO_DOUBLE 33
#define MKCKKS_OP_SPLIT30_D 34
#define MKCKKS_OP_CT_BUTTERFLY_FP 35
#define MKCKKS_OP_CT_BUTTERFLY_FP_NR 36
#define MKCKKS_OP_GS_BUTTERFLY_FP 37
#define MKCKKS_OP_RADIX_FORWARD_FP4 38
#define MKCKKS_OP_RADIX_INVERSE_FP4 39
#define MKCKKS_OP_COUNT 40
int mkckks_debug_arith(mkckks_ctx *c, uint32_t op, uint64_t q, const uint64_t *in, uint64_t *out, size_t count);

/* ---- introspection for tests: copy a CRT table to the host ---------------- */
int mkckks_ctx_twiddles(const mkckks_ctx *c, uint32_t limb, int inverse, uint64_t *h_out /*N*/);

#ifdef __cplusplus
}
#endif
#endif /* MKCKKS_H */
