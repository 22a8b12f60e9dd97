// capi.cpp -- extern "C" surface of libmkckks_hip.so (declared in include/mkckks.h).
// Thin: argument checks, exception -> status code translation, nothing else.
#include <cstring>
#include <new>
#include <string>

#include "../../include/mkckks.h"
#include "comm.hpp"
#include "engine.hpp"
#include "galois.hpp"

struct mkckks_ctx {
    mk::Engine *eng;
};

namespace {
thread_local std::string g_err;

template <typename F>
int guarded(F &&f) {
    try {
        f();
        return MKCKKS_OK;
    } catch (const mk::PrecisionError &e) {
        g_err = e.what();
        return MKCKKS_E_PRECISION;
    } catch (const mk::NoDevice &e) {
        g_err = e.what();
        return MKCKKS_E_NODEVICE;
    } catch (const mk::HipError &e) {
        g_err = e.what();
        return MKCKKS_E_HIP;
    } catch (const std::invalid_argument &e) {
        g_err = e.what();
        return MKCKKS_E_INVALID;
    } catch (const std::out_of_range &e) {
        g_err = e.what();
        return MKCKKS_E_INVALID;
    } catch (const std::bad_alloc &) {
        g_err = "out of host memory";
        return MKCKKS_E_NOMEM;
    } catch (const std::exception &e) {
        g_err = e.what();
        return MKCKKS_E_INTERNAL;
    } catch (...) {
        g_err = "unknown error";
        return MKCKKS_E_INTERNAL;
    }
}

// one bound on the number of parties, three names: the header's, the sharing kernel's and the Lagrange arithmetic's
static_assert(MKCKKS_MAX_PARTIES == mk::SHAMIR_MAX_PARTIES && MKCKKS_MAX_PARTIES == mk::ParamSet::LAGRANGE_MAX_PARTIES,
              "MKCKKS_MAX_PARTIES, SHAMIR_MAX_PARTIES and LAGRANGE_MAX_PARTIES must agree");

void need(bool ok, const char *what) {
    if (!ok) throw std::invalid_argument(what);
}
}  // namespace

extern "C" {

const char *mkckks_last_error(void) { return g_err.c_str(); }
const char *mkckks_version(void) { return "mkckks-hip 0.2 (gfx950)"; }

int mkckks_ctx_create(const mkckks_params *p, mkckks_ctx **out) {
    return guarded([&] {
        need(p && out, "null argument");
        mk::ParamSet ps;
        ps.generate(p->log_n, p->mult_depth, p->scaling_bits, p->first_bits, p->dnum, p->aux_bits, p->extra_bits);
        auto *eng = new mk::Engine(ps, p->device);
        *out = new mkckks_ctx{eng};
    });
}

int mkckks_ctx_destroy(mkckks_ctx *c) {
    return guarded([&] {
        if (!c) return;
        delete c->eng;
        delete c;
    });
}

int mkckks_ctx_info(const mkckks_ctx *c, mkckks_info *out) {
    return guarded([&] {
        need(c && out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        *out = mkckks_info{ps.n, ps.L, ps.K, ps.alpha, ps.beta, ps.n / 2};
    });
}

int mkckks_ctx_moduli(const mkckks_ctx *c, uint64_t *h_out) {
    return guarded([&] {
        need(c && h_out, "null argument");
        const auto &m = c->eng->params().moduli;
        std::memcpy(h_out, m.data(), m.size() * sizeof(uint64_t));
    });
}

int mkckks_ctx_arith(const mkckks_ctx *c, uint8_t *h_out) {
    return guarded([&] {
        need(c && h_out, "null argument");
        const auto &limb = c->eng->params().limb;
        for (size_t i = 0; i < limb.size(); ++i)
            h_out[i] = limb[i].fp ? MKCKKS_ARITH_FP64 : (limb[i].pm ? MKCKKS_ARITH_PM : MKCKKS_ARITH_INT);
    });
}

int mkckks_ctx_roots(const mkckks_ctx *c, uint64_t *h_out) {
    return guarded([&] {
        need(c && h_out, "null argument");
        const auto &r = c->eng->params().roots;
        std::memcpy(h_out, r.data(), r.size() * sizeof(uint64_t));
    });
}

int mkckks_scaling_factor(const mkckks_ctx *c, uint32_t level, int big, double *out) {
    return guarded([&] {
        need(c && out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        *out = big ? ps.sf_big.at(level) : ps.sf.at(level);
    });
}

int mkckks_ctx_twiddles(const mkckks_ctx *c, uint32_t limb, int inverse, uint64_t *h_out) {
    return guarded([&] {
        need(c && h_out, "null argument");
        need(limb < c->eng->params().D, "limb out of range");
        std::vector<uint64_t> w;
        c->eng->host_twiddles(limb, inverse != 0, w);
        std::memcpy(h_out, w.data(), w.size() * sizeof(uint64_t));
    });
}

int mkckks_debug_arith(mkckks_ctx *c, uint32_t op, uint64_t q, const uint64_t *in, uint64_t *out, size_t count) {
    return guarded([&] {
        need(c, "null context");
        need(op < MKCKKS_OP_COUNT, "unknown op");
        need(count == 0 || (in && out), "null argument");
        c->eng->debug_arith(op, q, in, out, count);
    });
}

int mkckks_set_stream(mkckks_ctx *c, void *s) {
    return guarded([&] {
        need(c, "null context");
        c->eng->set_stream(reinterpret_cast<hipStream_t>(s));
    });
}
int mkckks_sync(mkckks_ctx *c) {
    return guarded([&] {
        need(c, "null context");
        c->eng->sync();
    });
}

int mkckks_dev_alloc(mkckks_ctx *c, size_t bytes, void **d_out) {
    return guarded([&] {
        need(c && d_out, "null argument");
        *d_out = c->eng->dev_alloc(bytes);
    });
}
int mkckks_dev_free(mkckks_ctx *c, void *d) {
    return guarded([&] {
        need(c, "null context");
        if (d) c->eng->dev_free(d);
    });
}
int mkckks_upload(mkckks_ctx *c, void *d, const void *h, size_t bytes) {
    return guarded([&] {
        need(c && d && h, "null argument");
        c->eng->upload(d, h, bytes);
    });
}
int mkckks_download(mkckks_ctx *c, void *h, const void *d, size_t bytes) {
    return guarded([&] {
        need(c && d && h, "null argument");
        c->eng->download(h, d, bytes);
    });
}

int mkckks_host_alloc(mkckks_ctx *c, size_t bytes, void **h_out) {
    return guarded([&] {
        need(c && h_out, "null argument");
        *h_out = c->eng->host_alloc(bytes);
    });
}
int mkckks_host_free(mkckks_ctx *c, void *h) {
    return guarded([&] {
        need(c, "null context");
        c->eng->host_free(h);
    });
}
int mkckks_upload_async(mkckks_ctx *c, void *d, const void *h, size_t bytes, uint64_t *ticket_out) {
    return guarded([&] {
        need(c && (bytes == 0 || (d && h)), "null argument");
        const uint64_t t = c->eng->upload_async(d, h, bytes);
        if (ticket_out) *ticket_out = t;
    });
}
int mkckks_download_async(mkckks_ctx *c, void *h, const void *d, size_t bytes, uint64_t *ticket_out) {
    return guarded([&] {
        need(c && (bytes == 0 || (d && h)), "null argument");
        const uint64_t t = c->eng->download_async(h, d, bytes);
        if (ticket_out) *ticket_out = t;
    });
}
int mkckks_copy_done(mkckks_ctx *c, uint64_t ticket, int *done_out) {
    return guarded([&] {
        need(c && done_out, "null argument");
        *done_out = c->eng->copy_done(ticket) ? 1 : 0;
    });
}
int mkckks_copy_wait(mkckks_ctx *c, uint64_t ticket) {
    return guarded([&] {
        need(c, "null context");
        c->eng->copy_wait(ticket);
    });
}
int mkckks_fence_uploads(mkckks_ctx *c) {
    return guarded([&] {
        need(c, "null context");
        c->eng->fence_uploads();
    });
}
int mkckks_fence_compute(mkckks_ctx *c) {
    return guarded([&] {
        need(c, "null context");
        c->eng->fence_compute();
    });
}
int mkckks_debug_stamps(mkckks_ctx *c, unsigned long long *h_out, uint32_t region, size_t *n_out) {
    return guarded([&] {
        need(c && h_out && n_out, "null argument");
        *n_out = c->eng->debug_stamps(h_out, region);
    });
}
int mkckks_count_noncanonical(mkckks_ctx *c, const uint64_t *d_ct, uint32_t n_ct, uint32_t nl, uint64_t *h_count) {
    return guarded([&] {
        need(c && h_count && (n_ct == 0 || d_ct), "null argument");
        *h_count = c->eng->count_noncanonical(d_ct, n_ct, nl);
    });
}

int mkckks_ntt_forward_batch(mkckks_ctx *c, uint64_t *d, uint32_t n_polys, uint32_t nl, int with_p) {
    return guarded([&] {
        need(c && d, "null argument");
        c->eng->ntt_forward(d, n_polys, nl, with_p != 0);
    });
}
int mkckks_ntt_inverse_batch(mkckks_ctx *c, uint64_t *d, uint32_t n_polys, uint32_t nl, int with_p) {
    return guarded([&] {
        need(c && d, "null argument");
        c->eng->ntt_inverse(d, n_polys, nl, with_p != 0);
    });
}

int mkckks_eval_add_batch(mkckks_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *out, uint32_t n_ct,
                          uint32_t nl) {
    return guarded([&] {
        need(c && a && b && out, "null argument");
        c->eng->eval_add(a, b, out, n_ct, nl);
    });
}
int mkckks_eval_sum_batch(mkckks_ctx *c, const uint64_t *in, uint64_t *out, uint32_t n_clients, uint32_t n_ct,
                          uint32_t nl) {
    return guarded([&] {
        need(c && in && out, "null argument");
        c->eng->eval_sum(in, out, n_clients, n_ct, nl);
    });
}

int mkckks_rescale_mult_const_batch(mkckks_ctx *c, const uint64_t *in, uint64_t *out, uint32_t n_ct, uint32_t nl,
                                    double operand) {
    return guarded([&] {
        need(c && in && out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 2 && nl <= ps.L, "nl out of range");
        // after dropping limb nl-1 the ciphertext sits at level L-(nl-1)
        std::vector<uint64_t> f = ps.const_factors(nl - 1, ps.L - (nl - 1), operand);
        c->eng->rescale(in, out, n_ct, nl, &f);
    });
}
int mkckks_rescale_batch(mkckks_ctx *c, const uint64_t *in, uint64_t *out, uint32_t n_ct, uint32_t nl) {
    return guarded([&] {
        need(c && in && out, "null argument");
        c->eng->rescale(in, out, n_ct, nl, nullptr);
    });
}
int mkckks_mult_const_batch(mkckks_ctx *c, uint64_t *ct, uint32_t n_ct, uint32_t nl, double operand) {
    return guarded([&] {
        need(c && ct, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        c->eng->mult_const(ct, n_ct, nl, ps.const_factors(nl, ps.L - nl, operand));
    });
}
int mkckks_mult_plain_batch(mkckks_ctx *c, uint64_t *ct, const uint64_t *pt, uint32_t n_ct, uint32_t n_pt, uint32_t nl) {
    return guarded([&] {
        need(c && ct && pt, "null argument");
        need(nl >= 1 && nl <= c->eng->params().L, "nl out of range");
        need(n_pt == 1 || n_pt == n_ct, "n_pt must be 1 or n_ct");
        c->eng->mult_plain(ct, pt, n_ct, n_pt, nl);
    });
}
int mkckks_mult_plain_rescale_batch(mkckks_ctx *c, const uint64_t *in, const uint64_t *pt, uint64_t *out, uint32_t n_ct,
                                    uint32_t n_pt, uint32_t nl) {
    return guarded([&] {
        need(c && in && pt && out, "null argument");
        need(nl >= 2 && nl <= c->eng->params().L, "nl out of range");
        need(n_pt == 1 || n_pt == n_ct, "n_pt must be 1 or n_ct");
        c->eng->mult_plain_rescale(in, pt, out, n_ct, n_pt, nl);
    });
}

int mkckks_reencrypt_batch(mkckks_ctx *c, const uint64_t *ct, const uint64_t *evk, uint64_t *out, uint32_t n_ct,
                           uint32_t nl) {
    return guarded([&] {
        need(c && ct && evk && out, "null argument");
        c->eng->reencrypt(ct, evk, out, n_ct, nl);
    });
}
int mkckks_reencrypt_accumulate_batch(mkckks_ctx *c, const uint64_t *ct, const uint64_t *evk, uint64_t *acc,
                                      uint32_t n_ct, uint32_t nl) {
    return guarded([&] {
        need(c && ct && evk && acc, "null argument");
        c->eng->reencrypt(ct, evk, acc, n_ct, nl, true);
    });
}
int mkckks_reencrypt_sum_batch(mkckks_ctx *c, const uint64_t *cts, const uint64_t *evks, uint64_t *out, uint32_t n_clients,
                               uint32_t n_ct, uint32_t nl) {
    return guarded([&] {
        need(c && cts && evks && out, "null argument");
        c->eng->reencrypt_sum(cts, evks, out, n_clients, n_ct, nl);
    });
}
int mkckks_q0_walk_choice(uint32_t row_tiles, uint32_t n_int_q, uint32_t n_idx, int mode) {
    return mk::q0_walk_fused(row_tiles, n_int_q, n_idx, mode) ? 1 : 0;
}
uint32_t mkckks_icol_conv_targets(uint32_t n_fp_targets, uint64_t grid, int mode) {
    return mk::icol_conv_targets(n_fp_targets, grid, mode);
}
int mkckks_scale_evk_batch(mkckks_ctx *c, const uint64_t *d_evk_in, uint64_t *d_evk_out, uint32_t n_keys,
                           const double *h_weights, uint32_t sf_level) {
    return guarded([&] {
        need(c && (n_keys == 0 || (d_evk_in && d_evk_out && h_weights)), "null argument");
        c->eng->scale_evk(d_evk_in, d_evk_out, n_keys, h_weights, sf_level);
    });
}
int mkckks_reencrypt_wsum_batch(mkckks_ctx *c, const uint64_t *d_cts, const uint64_t *d_evks_scaled, uint64_t *d_out,
                                uint32_t n_clients, uint32_t n_ct, uint32_t nl, const double *h_weights, uint32_t sf_level) {
    return guarded([&] {
        need(c && ((n_clients == 0 || n_ct == 0) || (d_cts && d_evks_scaled && d_out && h_weights)), "null argument");
        c->eng->reencrypt_wsum(d_cts, d_evks_scaled, d_out, n_clients, n_ct, nl, h_weights, sf_level);
    });
}
int mkckks_eval_wsum_batch(mkckks_ctx *c, const uint64_t *d_in, uint64_t *d_out, uint32_t n_terms, uint32_t n_ct, uint32_t nl,
                           const double *h_weights, uint32_t sf_level, int first_is_sum) {
    return guarded([&] {
        need(c && ((n_terms == 0 || n_ct == 0) || (d_in && d_out && h_weights)), "null argument");
        c->eng->eval_wsum(d_in, d_out, n_terms, n_ct, nl, h_weights, sf_level, first_is_sum != 0);
    });
}
int mkckks_reencrypt_fanout_batch(mkckks_ctx *c, const uint64_t *ct, const uint64_t *evks, uint64_t *out, uint32_t n_keys,
                                  uint32_t n_ct, uint32_t nl) {
    return guarded([&] {
        need(c && ct && evks && out, "null argument");
        need(nl >= 1 && nl <= c->eng->params().L, "nl out of range");
        if (!n_keys || !n_ct) return;
        c->eng->reencrypt_fanout(ct, evks, out, n_keys, n_ct, nl);
    });
}
// argument rules shared by the two compact entry points; the overlap test works on addresses only
static void need_compact_args(const mk::ParamSet &ps, const uint64_t *in, const uint64_t *out, uint32_t n_keys, uint32_t n_ct,
                              uint32_t nl_in, uint32_t nl_out) {
    need(nl_out >= 1 && nl_out < nl_in && nl_in <= ps.L, "need 1 <= nl_out < nl_in <= L");
    const size_t poly_bytes = (size_t)n_ct * 2 * ps.n * sizeof(uint64_t);
    const uintptr_t i_lo = (uintptr_t)in, i_hi = i_lo + poly_bytes * nl_in;
    const uintptr_t o_lo = (uintptr_t)out, o_hi = o_lo + (size_t)n_keys * poly_bytes * nl_out;
    need(!(o_lo < i_hi && i_lo < o_hi), "output overlaps input");
}
int mkckks_compress_batch(mkckks_ctx *c, const uint64_t *in, uint64_t *out, uint32_t n_ct, uint32_t nl_in, uint32_t nl_out) {
    return guarded([&] {
        need(c && in && out, "null argument");
        need_compact_args(c->eng->params(), in, out, 1, n_ct, nl_in, nl_out);
        if (!n_ct) return;
        c->eng->compress(in, out, n_ct, nl_in, nl_out);
    });
}
int mkckks_reencrypt_fanout_compact_batch(mkckks_ctx *c, const uint64_t *ct, const uint64_t *evks, uint64_t *out,
                                          uint32_t n_keys, uint32_t n_ct, uint32_t nl_in, uint32_t nl_out) {
    return guarded([&] {
        need(c && ct && evks && out, "null argument");
        need_compact_args(c->eng->params(), ct, out, n_keys, n_ct, nl_in, nl_out);
        if (!n_keys || !n_ct) return;
        c->eng->reencrypt_fanout_compact(ct, evks, out, n_keys, n_ct, nl_in, nl_out);
    });
}
int mkckks_modup_batch(mkckks_ctx *c, const uint64_t *c1, uint64_t *digits, uint32_t n, uint32_t nl) {
    return guarded([&] {
        need(c && c1 && digits, "null argument");
        c->eng->modup(c1, digits, n, nl);
    });
}
int mkckks_moddown_batch(mkckks_ctx *c, const uint64_t *in, uint64_t *out, uint32_t n, uint32_t nl) {
    return guarded([&] {
        need(c && in && out, "null argument");
        c->eng->moddown(in, out, n, nl);
    });
}

int mkckks_keygen(mkckks_ctx *c, const int8_t *s, const uint64_t *a, const int32_t *e, uint64_t *pk, uint64_t *sk) {
    return guarded([&] {
        need(c && s && a && e && pk && sk, "null argument");
        c->eng->keygen(s, a, e, pk, sk);
    });
}
int mkckks_rekeygen(mkckks_ctx *c, const int8_t *s_old, const uint64_t *pk_new, const int8_t *u, const int32_t *e0,
                    const int32_t *e1, uint64_t *evk) {
    return guarded([&] {
        need(c && s_old && pk_new && u && e0 && e1 && evk, "null argument");
        c->eng->rekeygen(s_old, pk_new, u, e0, e1, evk);
    });
}
// ---- slot rotations: every refusal is decided here, before a device is asked for
static void need_galois(const mk::ParamSet &ps, uint32_t g) {
    need(mk::galois_valid(g, ps.log_n), "Galois element must be odd and below 2N");
}
static void need_apart(const void *in, const void *out, size_t bytes) {
    const uintptr_t i = (uintptr_t)in, o = (uintptr_t)out;
    need(!(o < i + bytes && i < o + bytes), "output overlaps input");
}
int mkckks_galois_element(const mkckks_ctx *c, int32_t step, uint32_t *g) {
    return guarded([&] {
        need(c && g, "null argument");
        *g = mk::galois_element(step, c->eng->params().log_n);
    });
}
int mkckks_automorphism_batch(mkckks_ctx *c, const uint64_t *in, uint64_t *out, uint32_t n_polys, uint32_t nl, uint32_t g) {
    return guarded([&] {
        need(c && in && out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        need_galois(ps, g);
        need_apart(in, out, (size_t)n_polys * nl * ps.n * sizeof(uint64_t));
        if (!n_polys) return;
        c->eng->automorphism(in, out, n_polys, nl, g);
    });
}
int mkckks_automorphism_secret(mkckks_ctx *c, const int8_t *s, int8_t *out, uint32_t g) {
    return guarded([&] {
        need(c && s && out, "null argument");
        need_galois(c->eng->params(), g);
        need_apart(s, out, c->eng->params().n);
        c->eng->automorphism_secret(s, out, g);
    });
}
int mkckks_galois_keygen(mkckks_ctx *c, const int8_t *s, const uint64_t *pk, const int8_t *u, const int32_t *e0,
                         const int32_t *e1, uint32_t g, uint64_t *evk) {
    return guarded([&] {
        need(c && s && pk && u && e0 && e1 && evk, "null argument");
        need_galois(c->eng->params(), g);
        c->eng->galois_keygen(s, pk, u, e0, e1, g, evk);
    });
}
int mkckks_rotate_batch(mkckks_ctx *c, const uint64_t *ct, const uint64_t *evk, uint64_t *out, uint32_t n_ct, uint32_t nl,
                        uint32_t g) {
    return guarded([&] {
        need(c && ct && evk && out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        need_galois(ps, g);
        need_apart(ct, out, (size_t)n_ct * 2 * nl * ps.n * sizeof(uint64_t));
        if (!n_ct) return;
        c->eng->rotate(ct, evk, out, n_ct, nl, g);
    });
}
int mkckks_slot_sum_batch(mkckks_ctx *c, const uint64_t *ct, const uint64_t *evks, uint64_t *out, uint32_t n_ct, uint32_t nl,
                          uint32_t span) {
    return guarded([&] {
        need(c && ct && out && (evks || span == 1), "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        need(span >= 1 && !(span & (span - 1)) && span <= ps.n / 2, "span must be a power of two in [1, N/2]");
        need_apart(ct, out, (size_t)n_ct * 2 * nl * ps.n * sizeof(uint64_t));
        if (!n_ct) return;
        c->eng->slot_sum(ct, evks, out, n_ct, nl, span);
    });
}
// ---- ciphertext products: every refusal is decided here, before a device is asked for
// bytes of `count` polynomials of nl limbs, saturated (a count that large overlaps everything)
static size_t poly_bytes(unsigned __int128 count, uint32_t nl, uint32_t n) {
    const unsigned __int128 b = count * nl * n * sizeof(uint64_t);
    return b > (unsigned __int128)(SIZE_MAX / 2) ? SIZE_MAX / 2 : (size_t)b;
}
static bool ranges_meet(const void *x, size_t x_bytes, const void *y, size_t y_bytes) {
    const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y;
    const uintptr_t a_end = a + x_bytes < a ? UINTPTR_MAX : a + x_bytes, b_end = b + y_bytes < b ? UINTPTR_MAX : b + y_bytes;
    return a < b_end && b < a_end;
}
static void need_aligned16(std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs) need(((uintptr_t)p & 15) == 0, "ciphertext arrays must be 16-byte aligned");
}
// ---- linear transforms: every refusal is decided here, before a device is asked for (h_g is a host array and is read)
int mkckks_encode_ext_batch(mkckks_ctx *c, const double *vals, uint64_t *pt, uint32_t n, uint32_t nl, double scale) {
    return guarded([&] {
        need(c && vals && pt, "null argument");
        need(scale > 0, "scale must be positive");
        need(nl >= 1 && nl <= c->eng->params().L, "nl out of range");
        c->eng->encode_ext(vals, pt, n, nl, scale);
    });
}
int mkckks_linear_transform_batch(mkckks_ctx *c, const uint64_t *ct, const uint64_t *evks, const uint64_t *pts,
                                  const uint32_t *h_g, uint64_t *out, uint32_t n_rot, uint32_t n_ct, uint32_t nl) {
    return guarded([&] {
        need(c && ct && pts && h_g && out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        if (!n_rot || !n_ct) return;
        bool keyed = false;
        for (uint32_t r = 0; r < n_rot; ++r) {
            need_galois(ps, h_g[r]);
            keyed = keyed || h_g[r] != 1u;
        }
        need(evks || !keyed, "null argument");  // a transform of unrotated terms alone reads no key
        need_aligned16({ct, evks, pts, out});
        const size_t ct_bytes = poly_bytes((unsigned __int128)n_ct * 2, nl, ps.n);
        need(!ranges_meet(ct, ct_bytes, out, ct_bytes), "output overlaps input");
        need(!ranges_meet(pts, poly_bytes(n_rot, nl + ps.K, ps.n), out, ct_bytes), "output overlaps the plaintexts");
        if (keyed)
            need(!ranges_meet(evks, poly_bytes((unsigned __int128)n_rot * ps.beta * 2, ps.D, ps.n), out, ct_bytes),
                 "output overlaps the keys");
        need(ps.num_parts(nl) <= 6, "more than 6 key-switch digits unsupported");
        c->eng->linear_transform(ct, evks, pts, h_g, out, n_rot, n_ct, nl);
    });
}
int mkckks_linear_transform_bsgs_batch(mkckks_ctx *c, const uint64_t *ct, const uint64_t *bkeys, const uint32_t *h_gb,
                                       uint32_t n1, const uint64_t *gkeys, const uint32_t *h_gg, uint32_t n2,
                                       const uint64_t *pts, const uint8_t *h_present, uint64_t *out, uint32_t n_ct,
                                       uint32_t nl) {
    return guarded([&] {
        need(c && ct && h_gb && h_gg && pts && h_present && out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(n1 >= 1 && n1 <= MKCKKS_BSGS_MAX && n2 >= 1 && n2 <= MKCKKS_BSGS_MAX, "n1 and n2 must be in [1, MKCKKS_BSGS_MAX]");
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        bool bkeyed = false, gkeyed = false, any = false;
        for (uint32_t b = 0; b < n1; ++b) {
            need_galois(ps, h_gb[b]);
            bkeyed = bkeyed || h_gb[b] != 1u;
        }
        for (uint32_t t = 0; t < n2; ++t) {
            need_galois(ps, h_gg[t]);
            gkeyed = gkeyed || h_gg[t] != 1u;
        }
        need((bkeys || !bkeyed) && (gkeys || !gkeyed), "null argument");
        need_aligned16({ct, bkeys, gkeys, pts, out});
        const size_t ct_bytes = poly_bytes((unsigned __int128)n_ct * 2, nl, ps.n);
        need(!ranges_meet(ct, ct_bytes, out, ct_bytes), "output overlaps input");
        need(!ranges_meet(pts, poly_bytes((unsigned __int128)n1 * n2, nl + ps.K, ps.n), out, ct_bytes),
             "output overlaps the plaintexts");
        if (bkeyed)
            need(!ranges_meet(bkeys, poly_bytes((unsigned __int128)n1 * ps.beta * 2, ps.D, ps.n), out, ct_bytes),
                 "output overlaps the keys");
        if (gkeyed)
            need(!ranges_meet(gkeys, poly_bytes((unsigned __int128)n2 * ps.beta * 2, ps.D, ps.n), out, ct_bytes),
                 "output overlaps the keys");
        need(ps.num_parts(nl) <= 6, "more than 6 key-switch digits unsupported");
        for (size_t k = 0; k < (size_t)n1 * n2; ++k) any = any || h_present[k];
        if (!n_ct || !any) return;
        c->eng->linear_transform_bsgs(ct, bkeys, h_gb, n1, gkeys, h_gg, n2, pts, h_present, out, n_ct, nl);
    });
}
int mkckks_relin_keygen(mkckks_ctx *c, const int8_t *s, const uint64_t *pk, const int8_t *u, const int32_t *e0,
                        const int32_t *e1, uint64_t *evk) {
    return guarded([&] {
        need(c && s && pk && u && e0 && e1 && evk, "null argument");
        c->eng->relin_keygen(s, pk, u, e0, e1, evk);
    });
}
int mkckks_tensor_sum_batch(mkckks_ctx *c, const uint64_t *a, const uint64_t *b, uint64_t *out3, uint32_t n_terms,
                            uint32_t n_ct, uint32_t nl) {
    return guarded([&] {
        need(c && a && b && out3, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        need(n_terms >= 1, "n_terms must be at least 1");
        need_aligned16({a, b, out3});
        const size_t in_bytes = poly_bytes((unsigned __int128)n_terms * n_ct * 2, nl, ps.n);
        const size_t out_bytes = poly_bytes((unsigned __int128)n_ct * 3, nl, ps.n);
        need(!ranges_meet(a, in_bytes, out3, out_bytes) && !ranges_meet(b, in_bytes, out3, out_bytes), "output overlaps input");
        if (!n_ct) return;
        c->eng->tensor_sum(a, b, out3, n_terms, n_ct, nl);
    });
}
int mkckks_relinearize_batch(mkckks_ctx *c, const uint64_t *in3, const uint64_t *rlk, uint64_t *out, uint32_t n_ct,
                             uint32_t nl) {
    return guarded([&] {
        need(c && in3 && rlk && out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        need_aligned16({in3, out});
        need(!ranges_meet(in3, poly_bytes((unsigned __int128)n_ct * 3, nl, ps.n), out, poly_bytes((unsigned __int128)n_ct * 2, nl, ps.n)),
             "output overlaps input");
        if (!n_ct) return;
        c->eng->relinearize(in3, rlk, out, n_ct, nl);
    });
}
int mkckks_mult_relin_batch(mkckks_ctx *c, const uint64_t *a, const uint64_t *b, const uint64_t *rlk, uint64_t *out,
                            uint32_t n_ct, uint32_t nl) {
    return guarded([&] {
        need(c && a && b && rlk && out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        need_aligned16({a, b, out});
        const size_t bytes = poly_bytes((unsigned __int128)n_ct * 2, nl, ps.n);
        need((out == a || !ranges_meet(a, bytes, out, bytes)) && (out == b || !ranges_meet(b, bytes, out, bytes)),
             "output partially overlaps an input");
        if (!n_ct) return;
        c->eng->mult_relin(a, b, rlk, out, n_ct, nl);
    });
}
// ---- polynomial evaluation: every refusal is decided here, before a device is asked for (the h_ arrays are host arrays)
static_assert(MKCKKS_POLY_MAX_DEGREE == mk::POLY_MAX_DEGREE && MKCKKS_POLY_MAX_B == mk::POLY_MAX_B, "polynomial limits");
static_assert(sizeof(struct mkckks_poly_plan) == sizeof(mk::PolyPlan), "mkckks_poly_plan mirrors mk::PolyPlan");
int mkckks_poly_plan(const mkckks_ctx *c, uint32_t degree, uint32_t nl, struct mkckks_poly_plan *out) {
    return guarded([&] {
        need(c && out, "null argument");
        const mk::PolyPlan p = c->eng->params().poly_plan(degree, nl);
        std::memcpy(out, &p, sizeof(p));
    });
}
// words of powers 1 .. n_pow of n_ct ciphertexts, from the ladder's limb counts
static size_t ladder_bytes(const uint32_t *nlk, uint32_t n_pow, uint32_t n_ct, uint32_t n) {
    unsigned __int128 limbs = 0;
    for (uint32_t k = 0; k < n_pow; ++k) limbs += nlk[k];
    const unsigned __int128 b = limbs * n_ct * 2 * n * sizeof(uint64_t);
    return b > (unsigned __int128)(SIZE_MAX / 2) ? SIZE_MAX / 2 : (size_t)b;
}
int mkckks_powers_batch(mkckks_ctx *c, const uint64_t *d_z, const uint64_t *d_rlk, uint64_t *d_out, uint32_t n_ct, uint32_t nl,
                        uint32_t n_pow, double scale_in, uint32_t *h_nl_out, double *h_scale_out) {
    return guarded([&] {
        need(c && d_z && d_rlk && d_out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        need(n_pow >= 1 && n_pow <= 64, "n_pow must be in [1, 64]");
        need(scale_in > 0, "scale must be positive");
        std::vector<uint32_t> nlk(n_pow);
        std::vector<double> sk(n_pow);
        ps.power_ladder(nl, n_pow, scale_in, nlk.data(), sk.data());
        need_aligned16({d_z, d_out});
        const size_t out_bytes = ladder_bytes(nlk.data(), n_pow, n_ct, ps.n);
        need(!ranges_meet(d_z, poly_bytes((unsigned __int128)n_ct * 2, nl, ps.n), d_out, out_bytes), "output overlaps input");
        need(!ranges_meet(d_rlk, poly_bytes((unsigned __int128)ps.beta * 2, ps.D, ps.n), d_out, out_bytes), "output overlaps the key");
        need(n_pow < 2 || ps.num_parts(nl) <= 6, "more than 6 key-switch digits unsupported");
        if (h_nl_out) std::memcpy(h_nl_out, nlk.data(), n_pow * sizeof(uint32_t));
        if (h_scale_out) std::memcpy(h_scale_out, sk.data(), n_pow * sizeof(double));
        if (!n_ct) return;
        c->eng->powers(d_z, d_rlk, d_out, n_ct, nl, n_pow);
    });
}
int mkckks_poly_weights(const mkckks_ctx *c, const double *h_coef, uint32_t degree, uint32_t nl, double scale_in, double *h_w,
                        double *scale_out) {
    return guarded([&] {
        need(c && h_coef && h_w && scale_out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        const mk::PolyPlan p = ps.poly_plan(degree, nl);
        std::vector<double> w((size_t)p.B * p.G);
        *scale_out = ps.poly_weights(h_coef, degree, nl, scale_in, w.data());
        std::memcpy(h_w, w.data(), w.size() * sizeof(double));
    });
}
int mkckks_poly_tensor_batch(mkckks_ctx *c, const uint64_t *d_baby, const uint32_t *h_baby_nl, const uint64_t *d_giant,
                             const uint32_t *h_giant_nl, const double *h_w, uint64_t *d_out3, uint32_t B, uint32_t G,
                             uint32_t n_ct, uint32_t nl_T) {
    return guarded([&] {
        need(c && d_baby && h_baby_nl && d_giant && h_giant_nl && h_w && d_out3, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(B == 2 || B == 4 || B == 8, "B must be 2, 4 or 8");
        need(G >= 2 && G <= B, "G must be in [2, B]");
        need(nl_T >= 1 && nl_T <= ps.L, "nl_T out of range");
        for (uint32_t i = 0; i + 1 < B; ++i) need(h_baby_nl[i] >= nl_T && h_baby_nl[i] <= ps.L, "a baby's limb count is outside [nl_T, L]");
        for (uint32_t j = 0; j + 1 < G; ++j) need(h_giant_nl[j] >= nl_T && h_giant_nl[j] <= ps.L, "a giant's limb count is outside [nl_T, L]");
        need_aligned16({d_baby, d_giant, d_out3});
        const size_t out_bytes = poly_bytes((unsigned __int128)n_ct * 3, nl_T, ps.n);
        need(!ranges_meet(d_baby, ladder_bytes(h_baby_nl, B - 1, n_ct, ps.n), d_out3, out_bytes) &&
                 !ranges_meet(d_giant, ladder_bytes(h_giant_nl, G - 1, n_ct, ps.n), d_out3, out_bytes),
             "output overlaps input");
        (void)ps.poly_constants(h_w, B * G, nl_T);  // the weights' refusals, before a device is asked for
        if (!n_ct) return;
        c->eng->poly_tensor(d_baby, h_baby_nl, d_giant, h_giant_nl, h_w, d_out3, B, G, n_ct, nl_T);
    });
}
int mkckks_poly_eval_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_rlk, const double *h_coef, uint32_t degree,
                           uint64_t *d_out, uint32_t n_ct, uint32_t nl, double scale_in, double *scale_out) {
    return guarded([&] {
        need(c && d_ct && d_rlk && h_coef && d_out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        const mk::PolyPlan p = ps.poly_plan(degree, nl);
        std::vector<double> w((size_t)p.B * p.G);
        const double s_out = ps.poly_weights(h_coef, degree, nl, scale_in, w.data());
        (void)ps.poly_constants(w.data(), p.B * p.G, p.nl_T);
        need_aligned16({d_ct, d_out});
        const size_t out_bytes = poly_bytes((unsigned __int128)n_ct * 2, p.nl_out, ps.n);
        need(!ranges_meet(d_ct, poly_bytes((unsigned __int128)n_ct * 2, nl, ps.n), d_out, out_bytes), "output overlaps input");
        need(!ranges_meet(d_rlk, poly_bytes((unsigned __int128)ps.beta * 2, ps.D, ps.n), d_out, out_bytes), "output overlaps the key");
        need(ps.num_parts(nl) <= 6, "more than 6 key-switch digits unsupported");
        if (scale_out) *scale_out = s_out;
        if (!n_ct) return;
        c->eng->poly_eval(d_ct, d_rlk, h_coef, degree, d_out, n_ct, nl, scale_in);
    });
}
// ---- Chebyshev series: every refusal is decided here, before a device is asked for (the h_ arrays are host arrays)
int mkckks_affine_batch(mkckks_ctx *c, const uint64_t *d_in, uint64_t *d_out, uint32_t n_ct, uint32_t nl, double w_mul,
                        double w_add) {
    return guarded([&] {
        need(c && d_in && d_out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        need_aligned16({d_in, d_out});
        const size_t bytes = poly_bytes((unsigned __int128)n_ct * 2, nl, ps.n);
        need(d_out == d_in || !ranges_meet(d_in, bytes, d_out, bytes), "output partially overlaps the input");
        const double w[2] = {w_mul, w_add};
        (void)ps.poly_constants(w, 2, nl);  // the weights' refusals
        if (!n_ct) return;
        c->eng->affine(d_in, d_out, n_ct, nl, w_mul, w_add);
    });
}
int mkckks_cheb_tensor_batch(mkckks_ctx *c, const uint64_t *d_a, uint32_t nl_a, const uint64_t *d_b, uint32_t nl_b,
                             const uint64_t *d_t, uint32_t nl_t, double w, uint64_t *d_out3, uint32_t n_ct, uint32_t nl) {
    return guarded([&] {
        need(c && d_a && d_b && d_out3, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        need(nl_a >= nl && nl_a <= ps.L && nl_b >= nl && nl_b <= ps.L && (!d_t || (nl_t >= nl && nl_t <= ps.L)),
             "an operand's limb count is outside [nl, L]");
        need(d_a != d_b || nl_a == nl_b, "the square needs one limb count");
        need_aligned16({d_a, d_b, d_t, d_out3});
        const size_t out_bytes = poly_bytes((unsigned __int128)n_ct * 3, nl, ps.n);
        need(!ranges_meet(d_a, poly_bytes((unsigned __int128)n_ct * 2, nl_a, ps.n), d_out3, out_bytes) &&
                 !ranges_meet(d_b, poly_bytes((unsigned __int128)n_ct * 2, nl_b, ps.n), d_out3, out_bytes) &&
                 !(d_t && ranges_meet(d_t, poly_bytes((unsigned __int128)n_ct * 2, nl_t, ps.n), d_out3, out_bytes)),
             "output overlaps input");
        (void)ps.poly_constants(&w, 1, nl);  // the weight's refusals
        if (!n_ct) return;
        c->eng->cheb_tensor(d_a, nl_a, d_b, nl_b, d_t, nl_t, w, d_out3, n_ct, nl);
    });
}
// every step's weight S_i * S_j / S_{i-j} must fit its level: decided here, so that a ladder never stops half way
static void need_ladder_weights(const mk::ParamSet &ps, const uint32_t *nlk, const double *sk, uint32_t n_cheb) {
    for (uint32_t k = 2; k <= n_cheb; ++k) {  // nlk / sk are 0-based: entry k - 1 belongs to T_k
        const uint32_t i = (k + 1) / 2, j = k - i;
        const double prod = sk[i - 1] * sk[j - 1];
        const double w = i != j ? prod / sk[0] : prod;
        (void)ps.poly_constants(&w, 1, nlk[i - 1]);
    }
}
int mkckks_cheb_ladder_batch(mkckks_ctx *c, const uint64_t *d_u, const uint64_t *d_rlk, uint64_t *d_out, uint32_t n_ct,
                             uint32_t nl, uint32_t n_cheb, double scale_in, uint32_t *h_nl_out, double *h_scale_out) {
    return guarded([&] {
        need(c && d_u && d_rlk && d_out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        need(n_cheb >= 1 && n_cheb <= 64, "n must be in [1, 64]");
        need(scale_in > 0 && std::isfinite(scale_in), "scale must be positive and finite");
        std::vector<uint32_t> nlk(n_cheb);
        std::vector<double> sk(n_cheb);
        ps.power_ladder(nl, n_cheb, scale_in, nlk.data(), sk.data());
        need_ladder_weights(ps, nlk.data(), sk.data(), n_cheb);
        need_aligned16({d_u, d_out});
        const size_t out_bytes = ladder_bytes(nlk.data(), n_cheb, n_ct, ps.n);
        need(!ranges_meet(d_u, poly_bytes((unsigned __int128)n_ct * 2, nl, ps.n), d_out, out_bytes), "output overlaps input");
        need(!ranges_meet(d_rlk, poly_bytes((unsigned __int128)ps.beta * 2, ps.D, ps.n), d_out, out_bytes), "output overlaps the key");
        need(n_cheb < 2 || ps.num_parts(nl) <= 6, "more than 6 key-switch digits unsupported");
        if (h_nl_out) std::memcpy(h_nl_out, nlk.data(), n_cheb * sizeof(uint32_t));
        if (h_scale_out) std::memcpy(h_scale_out, sk.data(), n_cheb * sizeof(double));
        if (!n_ct) return;
        c->eng->cheb_ladder(d_u, d_rlk, d_out, n_ct, nl, n_cheb, scale_in);
    });
}
int mkckks_cheb_weights(const mkckks_ctx *c, const double *h_coef, uint32_t degree, uint32_t nl, double scale_in, double *h_w,
                        double *scale_out) {
    return guarded([&] {
        need(c && h_coef && h_w && scale_out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        const mk::PolyPlan p = ps.poly_plan(degree, nl);
        std::vector<double> w((size_t)p.B * p.G);
        *scale_out = ps.cheb_weights(h_coef, degree, nl, scale_in, w.data());
        std::memcpy(h_w, w.data(), w.size() * sizeof(double));
    });
}
int mkckks_cheb_eval_batch(mkckks_ctx *c, const uint64_t *d_ct, const uint64_t *d_rlk, const double *h_coef, uint32_t degree,
                           double a, double b, uint64_t *d_out, uint32_t n_ct, uint32_t nl, double scale_in, double *scale_out) {
    return guarded([&] {
        need(c && d_ct && d_rlk && h_coef && d_out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(std::isfinite(a) && std::isfinite(b) && a < b, "the interval needs finite a < b");
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        need(scale_in > 0 && std::isfinite(scale_in), "scale must be positive and finite");
        const bool mapped = !(a == -1.0 && b == 1.0);
        const uint32_t nl_u = mapped ? nl - 1 : nl;
        mk::PolyPlan p{};
        try {
            if (mapped && nl_u < 1) throw std::invalid_argument("degree " + std::to_string(degree) + " needs at least 3 limbs");
            p = ps.poly_plan(degree, nl_u);
        } catch (const std::invalid_argument &e) {
            if (!mapped) throw;
            throw std::invalid_argument(std::string(e.what()) + " (the map of [a, b] onto [-1, 1] spends one of the input's " +
                                        std::to_string(nl) + ")");
        }
        const double scale_u = mapped ? ps.sf.at(ps.L - nl_u) : scale_in;
        if (mapped) {
            const double sigma1 = scale_u * (double)ps.moduli[nl - 1];
            const double w[2] = {2.0 / (b - a) * (sigma1 / scale_in), -(a + b) / (b - a) * sigma1};
            (void)ps.poly_constants(w, 2, nl);
        }
        std::vector<double> w((size_t)p.B * p.G);
        const double s_out = ps.cheb_weights(h_coef, degree, nl_u, scale_u, w.data());
        (void)ps.poly_constants(w.data(), p.B * p.G, p.nl_T);
        uint32_t nlx[mk::POLY_MAX_B], nly[mk::POLY_MAX_B];
        double sx[mk::POLY_MAX_B], sy[mk::POLY_MAX_B];
        ps.power_ladder(nl_u, p.B, scale_u, nlx, sx);
        need_ladder_weights(ps, nlx, sx, p.B);
        ps.power_ladder(nlx[p.B - 1], p.G - 1, sx[p.B - 1], nly, sy);
        need_ladder_weights(ps, nly, sy, p.G - 1);
        need_aligned16({d_ct, d_out});
        const size_t out_bytes = poly_bytes((unsigned __int128)n_ct * 2, p.nl_out, ps.n);
        need(!ranges_meet(d_ct, poly_bytes((unsigned __int128)n_ct * 2, nl, ps.n), d_out, out_bytes), "output overlaps input");
        need(!ranges_meet(d_rlk, poly_bytes((unsigned __int128)ps.beta * 2, ps.D, ps.n), d_out, out_bytes), "output overlaps the key");
        need(ps.num_parts(nl) <= 6, "more than 6 key-switch digits unsupported");
        if (scale_out) *scale_out = s_out;
        if (!n_ct) return;
        c->eng->cheb_eval(d_ct, d_rlk, h_coef, degree, a, b, d_out, n_ct, nl, scale_in);
    });
}
// ---- collective evaluation keys of a joint key: every refusal is decided here, before a device is asked for
int mkckks_evk_sum(mkckks_ctx *c, const uint64_t *in, uint64_t *out, uint32_t n_parties, uint32_t n_keys) {
    return guarded([&] {
        need(c && in && out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(n_parties >= 1 && n_parties <= MKCKKS_MAX_PARTIES, "need 1 <= n_parties <= MKCKKS_MAX_PARTIES");
        need_aligned16({in, out});
        const size_t set_bytes = poly_bytes((unsigned __int128)n_keys * ps.beta * 2, ps.D, ps.n);
        const size_t in_bytes = poly_bytes((unsigned __int128)n_parties * n_keys * ps.beta * 2, ps.D, ps.n);
        need(out == in || !ranges_meet(in, in_bytes, out, set_bytes), "output overlaps the shares (only the first share may be the output)");
        if (!n_keys) return;
        c->eng->evk_sum(in, out, n_parties, n_keys);
    });
}
int mkckks_relin_share(mkckks_ctx *c, const uint64_t *key1, const uint64_t *sk, const int32_t *e0, const int32_t *e1,
                       uint64_t *share) {
    return guarded([&] {
        need(c && key1 && sk && e0 && e1 && share, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need_aligned16({key1, sk, share});
        const size_t key_bytes = poly_bytes((unsigned __int128)ps.beta * 2, ps.D, ps.n), sk_bytes = poly_bytes(1, ps.D, ps.n);
        const size_t e_bytes = (size_t)ps.beta * ps.n * sizeof(int32_t);
        need(share == key1 || !ranges_meet(key1, key_bytes, share, key_bytes), "share partially overlaps the round-1 key");
        need(!ranges_meet(sk, sk_bytes, share, key_bytes) && !ranges_meet(e0, e_bytes, share, key_bytes) &&
                 !ranges_meet(e1, e_bytes, share, key_bytes),
             "share overlaps an input");
        c->eng->relin_share(key1, sk, e0, e1, share);
    });
}
int mkckks_encrypt_batch(mkckks_ctx *c, const uint64_t *pk, const uint64_t *pt, const int8_t *v, const int32_t *e0,
                         const int32_t *e1, uint64_t *ct, uint32_t n_ct, uint32_t nl) {
    return guarded([&] {
        need(c && pk && pt && v && e0 && e1 && ct, "null argument");
        c->eng->encrypt(pk, pt, v, e0, e1, ct, n_ct, nl);
    });
}
int mkckks_rerandomize_batch(mkckks_ctx *c, const uint64_t *ct, const uint64_t *pk, const int8_t *v, const int64_t *e0,
                             const int64_t *e1, uint64_t *out, uint32_t n_ct, uint32_t nl_in, uint32_t nl) {
    return guarded([&] {
        need(c && ct && pk && v && e0 && e1 && out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= nl_in && nl_in <= ps.L, "need 1 <= nl <= nl_in <= L");
        if (!(out == ct && nl_in == nl)) {  // in place is the one allowed overlap; addresses only
            const size_t poly_bytes = (size_t)n_ct * 2 * ps.n * sizeof(uint64_t);
            const uintptr_t i_lo = (uintptr_t)ct, i_hi = i_lo + poly_bytes * nl_in;
            const uintptr_t o_lo = (uintptr_t)out, o_hi = o_lo + poly_bytes * nl;
            need(!(o_lo < i_hi && i_lo < o_hi), "output overlaps input");
        }
        if (!n_ct) return;
        c->eng->rerandomize(ct, pk, v, e0, e1, out, n_ct, nl_in, nl);
    });
}
int mkckks_encrypt_seeded_batch(mkckks_ctx *c, const uint64_t *sk, const uint64_t *pt, const int32_t *e, uint64_t *c0,
                                uint32_t n_ct, uint32_t nl, const uint8_t *h_seed32, uint32_t stream_base) {
    return guarded([&] {
        need(c && sk && pt && e && c0 && h_seed32, "null argument");
        c->eng->encrypt_seeded(sk, pt, e, c0, n_ct, nl, h_seed32, stream_base);
    });
}
int mkckks_expand_seeded_batch(mkckks_ctx *c, uint64_t *ct, uint32_t n_ct, uint32_t nl, const uint8_t *h_seeds32,
                               const uint32_t *h_stream_ids) {
    return guarded([&] {
        need(c && ct && h_seeds32 && h_stream_ids, "null argument");
        c->eng->expand_seeded(ct, n_ct, nl, h_seeds32, h_stream_ids);
    });
}
int mkckks_lift_ntt_batch(mkckks_ctx *c, const double *coef, uint64_t *out, uint32_t n, uint32_t nl) {
    return guarded([&] {
        need(c && coef && out, "null argument");
        c->eng->lift_ntt(coef, out, n, nl);
    });
}
int mkckks_sample_ternary(mkckks_ctx *c, int8_t *out, size_t count, const uint8_t *h_key32, uint32_t stream_id) {
    return guarded([&] {
        need(c && out && h_key32, "null argument");
        c->eng->sample_ternary(out, count, h_key32, stream_id);
    });
}
int mkckks_sample_gauss(mkckks_ctx *c, int32_t *out, size_t count, double sigma, const uint8_t *h_key32,
                        uint32_t stream_id) {
    return guarded([&] {
        need(c && out && h_key32, "null argument");
        c->eng->sample_gauss(out, count, sigma, h_key32, stream_id);
    });
}
int mkckks_sample_gauss_wide(mkckks_ctx *c, int64_t *out, size_t count, double sigma, const uint8_t *h_key32,
                             uint32_t stream_id) {
    return guarded([&] {
        need(c && out && h_key32, "null argument");
        need(sigma >= 0x1p6 && sigma <= 0x1p56, "sigma outside [2^6, 2^56]");
        if (!count) return;
        c->eng->sample_gauss_wide(out, count, sigma, h_key32, stream_id);
    });
}
int mkckks_sample_uniform(mkckks_ctx *c, uint64_t *out, uint32_t n_polys, uint32_t nl, int with_p, const uint8_t *h_key32,
                          uint32_t stream_id) {
    return guarded([&] {
        need(c && out && h_key32, "null argument");
        c->eng->sample_uniform(out, n_polys, nl, with_p != 0, h_key32, stream_id);
    });
}
int mkckks_chacha20_block(mkckks_ctx *c, uint32_t *d_out16, const uint8_t *h_key32, uint32_t counter,
                          const uint32_t *h_nonce3) {
    return guarded([&] {
        need(c && d_out16 && h_key32 && h_nonce3, "null argument");
        c->eng->chacha_block(d_out16, h_key32, counter, h_nonce3);
    });
}
int mkckks_encode_batch(mkckks_ctx *c, const double *vals, uint64_t *pt, uint32_t n, uint32_t nl, double scale) {
    return guarded([&] {
        need(c && vals && pt, "null argument");
        need(scale > 0, "scale must be positive");
        c->eng->encode(vals, pt, n, nl, scale);
    });
}
int mkckks_decode_batch(mkckks_ctx *c, const uint64_t *m, double *vals, uint32_t n, uint32_t nl, double scale) {
    return guarded([&] {
        need(c && m && vals, "null argument");
        need(scale > 0, "scale must be positive");
        c->eng->decode(m, vals, n, nl, scale);
    });
}
int mkckks_decode_flood_batch(mkckks_ctx *c, const uint64_t *m, double *vals, uint32_t n, uint32_t nl, double scale,
                              const uint8_t *h_key32, uint32_t stream_id, double *h_log2_sigma) {
    return guarded([&] {
        need(c && m && vals && h_key32, "null argument");
        need(scale > 0, "scale must be positive");
        c->eng->decode_flood(m, vals, n, nl, scale, h_key32, stream_id, h_log2_sigma);
    });
}
int mkckks_decrypt_batch(mkckks_ctx *c, const uint64_t *ct, const uint64_t *sk, uint64_t *m, uint32_t n_ct,
                         uint32_t nl) {
    return guarded([&] {
        need(c && ct && sk && m, "null argument");
        c->eng->decrypt(ct, sk, m, n_ct, nl);
    });
}
int mkckks_keygen_join(mkckks_ctx *c, const uint64_t *pk_prev, const int8_t *s, const int32_t *e, uint64_t *pk,
                       uint64_t *sk) {
    return guarded([&] {
        need(c && pk_prev && s && e && pk && sk, "null argument");
        c->eng->keygen_join(pk_prev, s, e, pk, sk);
    });
}
int mkckks_partial_decrypt_batch(mkckks_ctx *c, const uint64_t *ct, const uint64_t *sk, const int64_t *e, uint64_t *share,
                                 uint32_t n_ct, uint32_t nl_in, uint32_t nl, int lead) {
    return guarded([&] {
        need(c && ct && sk && e && share, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= nl_in && nl_in <= ps.L, "need 1 <= nl <= nl_in <= L");
        const size_t item_bytes = (size_t)n_ct * ps.n * sizeof(uint64_t);  // addresses only
        const uintptr_t i_lo = (uintptr_t)ct, i_hi = i_lo + item_bytes * 2 * nl_in;
        const uintptr_t o_lo = (uintptr_t)share, o_hi = o_lo + item_bytes * nl;
        need(!(o_lo < i_hi && i_lo < o_hi), "share overlaps the ciphertexts");
        if (!n_ct) return;
        c->eng->partial_decrypt(ct, sk, e, share, n_ct, nl_in, nl, lead != 0);
    });
}
int mkckks_switch_share_batch(mkckks_ctx *c, const uint64_t *ct, const uint64_t *sk, const uint64_t *pk, const int8_t *v,
                              const int64_t *e0, const int64_t *e1, uint64_t *share, uint32_t n_ct, uint32_t nl_in, uint32_t nl,
                              int lead) {
    return guarded([&] {
        need(c && ct && sk && pk && v && e0 && e1 && share, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= nl_in && nl_in <= ps.L, "need 1 <= nl <= nl_in <= L");
        const size_t item_bytes = (size_t)n_ct * 2 * ps.n * sizeof(uint64_t);  // addresses only
        const uintptr_t i_lo = (uintptr_t)ct, i_hi = i_lo + item_bytes * nl_in;
        const uintptr_t o_lo = (uintptr_t)share, o_hi = o_lo + item_bytes * nl;
        need(!(o_lo < i_hi && i_lo < o_hi), "share overlaps the ciphertexts");
        if (!n_ct) return;
        c->eng->switch_share(ct, sk, pk, v, e0, e1, share, n_ct, nl_in, nl, lead != 0);
    });
}
int mkckks_fuse_shares_batch(mkckks_ctx *c, const uint64_t *shares, uint64_t *m, uint32_t n_parties, uint32_t n_ct,
                             uint32_t nl) {
    return guarded([&] {
        need(c && shares && m, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(n_parties >= 1, "need n_parties >= 1");
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        if (m != shares) {  // shares[0] is the one allowed alias; addresses only
            const size_t share_bytes = (size_t)n_ct * nl * ps.n * sizeof(uint64_t);
            const uintptr_t i_lo = (uintptr_t)shares, i_hi = i_lo + share_bytes * n_parties;
            const uintptr_t o_lo = (uintptr_t)m, o_hi = o_lo + share_bytes;
            need(!(o_lo < i_hi && i_lo < o_hi), "output overlaps the shares");
        }
        if (!n_ct) return;
        c->eng->fuse_shares(shares, m, n_parties, n_ct, nl);
    });
}
int mkckks_share_key(mkckks_ctx *c, const uint64_t *sk, uint64_t *shares, uint32_t nl, uint32_t n_parties, uint32_t threshold,
                     const uint8_t *h_key32, uint32_t stream_id) {
    return guarded([&] {
        need(c && sk && shares && h_key32, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        need(threshold >= 1 && threshold <= n_parties && n_parties <= MKCKKS_MAX_PARTIES,
             "need 1 <= threshold <= n_parties <= MKCKKS_MAX_PARTIES");
        need((uint64_t)stream_id + threshold - 1 <= 0xFFFFFFFFull, "stream ids overflow 32 bits");
        const size_t limb_bytes = (size_t)ps.n * sizeof(uint64_t);  // addresses only; the first nl limbs of sk are read
        const uintptr_t i_lo = (uintptr_t)sk, i_hi = i_lo + limb_bytes * nl;
        const uintptr_t o_lo = (uintptr_t)shares, o_hi = o_lo + limb_bytes * nl * n_parties;
        need(!(o_lo < i_hi && i_lo < o_hi), "shares overlap the key");
        c->eng->share_key(sk, shares, nl, n_parties, threshold, h_key32, stream_id);
    });
}
int mkckks_combine_key_shares(mkckks_ctx *c, const uint64_t *in, const uint64_t *h_w, uint64_t *out, uint32_t m, uint32_t nl) {
    return guarded([&] {
        need(c && in && h_w && out, "null argument");
        const mk::ParamSet &ps = c->eng->params();
        need(m >= 1, "need m >= 1");
        need(nl >= 1 && nl <= ps.L, "nl out of range");
        for (uint32_t j = 0; j < m; ++j)
            for (uint32_t i = 0; i < nl; ++i) need(h_w[(size_t)j * nl + i] < ps.moduli[i], "weight not below its modulus");
        if (out != in) {  // in[0] is the one allowed alias; addresses only
            const size_t poly_bytes = (size_t)nl * ps.n * sizeof(uint64_t);
            const uintptr_t i_lo = (uintptr_t)in, i_hi = i_lo + poly_bytes * m;
            const uintptr_t o_lo = (uintptr_t)out, o_hi = o_lo + poly_bytes;
            need(!(o_lo < i_hi && i_lo < o_hi), "output overlaps the inputs");
        }
        c->eng->combine_key_shares(in, h_w, out, m, nl);
    });
}
int mkckks_lagrange_at_zero(const mkckks_ctx *c, const uint32_t *h_parties, uint32_t n_active, uint64_t *h_out) {
    return guarded([&] {
        need(c && h_parties && h_out, "null argument");
        c->eng->params().lagrange_at_zero(h_parties, n_active, h_out);
    });
}
int mkckks_reduce_mod_batch(mkckks_ctx *c, uint64_t *ct, uint32_t n_ct, uint32_t nl, uint32_t n_terms) {
    return guarded([&] {
        need(c && ct, "null argument");
        c->eng->reduce_mod(ct, n_ct, nl, n_terms);
    });
}

int mkckks_comm_unique_id(void *h_id) {
    return guarded([&] {
        need(h_id, "null argument");
        mk::comm_unique_id(h_id);
    });
}
int mkckks_comm_create(mkckks_ctx *c, const void *h_id, int n_ranks, int rank, void **comm_out) {
    return guarded([&] {
        need(c && h_id && comm_out, "null argument");
        if (!c->eng->has_device()) throw mk::NoDevice("host-only context: no communicator");
        *comm_out = mk::comm_create(c->eng->device(), h_id, n_ranks, rank);
    });
}
int mkckks_comm_destroy(mkckks_ctx *c, void *comm) {
    return guarded([&] {
        need(c != nullptr, "null argument");
        mk::comm_destroy(comm);
    });
}
int mkckks_reduce_scatter_sum_mod(mkckks_ctx *c, void *comm, const uint64_t *d_partial, uint64_t *d_shard,
                                  uint32_t n_ct_shard, uint32_t nl, uint32_t n_ranks) {
    return guarded([&] {
        need(c && comm && d_partial && d_shard, "null argument");
        c->eng->reduce_scatter_sum_mod(comm, d_partial, d_shard, n_ct_shard, nl, n_ranks);
    });
}
const char *mkckks_comm_library(void) {
    try {
        return mk::comm_library_path();
    } catch (const std::exception &e) {
        g_err = e.what();
        return "";
    }
}

}  // extern "C"
