// codec_kernels.hpp -- the floating-point half of CKKS Encode / Decode on the GPU (fp64).
//
// Stands in for CKKSPackedEncoding::Encode / Decode and DiscreteFourierTransform::FFTSpecialInv / FFTSpecial
// ([upstream] pke/lib/encoding/ckkspackedencoding.cpp, core/lib/math/dftransform.cpp), reached from
// client/src/encryptModelWeights.cpp:82,90,109 and client/src/decryptModelWeights.cpp:83,92,109.
// Full packing: N/2 complex slots, slot j at zeta^(5^j).  One launch per butterfly stage (15 at N = 2^16): these are
// client-side, per-round operations on a few dozen ciphertexts, far off the server's hot loop.
#pragma once
#include "modarith.hpp"
#include "sampler_kernels.hpp"

namespace mk {

struct CodecTables {
    const uint32_t *rot;   // 5^j mod 2N, j < N/2
    const double2 *ksi;    // exp(2 pi i k / 2N), k <= 2N
    uint32_t slots, log_slots, m;  // N/2, log2, 2N
};

MK_D double2 cmul(double2 a, double2 b) { return double2{a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
MK_D uint32_t brev(uint32_t x, uint32_t bits) { return __brev(x) >> (32 - bits); }

// decode direction (FFTSpecial): one stage of length `len` on v[items][slots]
__global__ void k_fft_special_stage(double2 *v, CodecTables t, uint32_t len) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= t.slots / 2) return;
    double2 *p = v + (size_t)blockIdx.y * t.slots;
    const uint32_t half = len >> 1, quad = len << 2, gap = t.m / quad;
    const uint32_t i = (b / half) * len, j = b % half;
    const double2 w = t.ksi[(t.rot[j] % quad) * gap];
    const double2 u = p[i + j], x = cmul(p[i + j + half], w);
    p[i + j] = double2{u.x + x.x, u.y + x.y};
    p[i + j + half] = double2{u.x - x.x, u.y - x.y};
}
// encode direction (FFTSpecialInv), before the bit reversal and the 1/size scaling
__global__ void k_fft_special_inv_stage(double2 *v, CodecTables t, uint32_t len) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= t.slots / 2) return;
    double2 *p = v + (size_t)blockIdx.y * t.slots;
    const uint32_t half = len >> 1, quad = len << 2, gap = t.m / quad;
    const uint32_t i = (b / half) * len, j = b % half;
    const double2 w = t.ksi[(quad - (t.rot[j] % quad)) * gap];
    const double2 a = p[i + j], c = p[i + j + half];
    p[i + j] = double2{a.x + c.x, a.y + c.y};
    p[i + j + half] = cmul(double2{a.x - c.x, a.y - c.y}, w);
}
// real slot values -> complex work array
__global__ void k_codec_load(const double *vals, double2 *v, uint32_t slots) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= slots) return;
    v[(size_t)blockIdx.y * slots + i] = double2{vals[(size_t)blockIdx.y * slots + i], 0.0};
}
// bit reversal + 1/size + scale; real parts -> coef[0..slots), imaginary parts -> coef[slots..N)
__global__ void k_codec_to_coef(const double2 *v, double *coef, CodecTables t, double scale) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.slots) return;
    const double2 x = v[(size_t)blockIdx.y * t.slots + brev(i, t.log_slots)];
    const double f = scale / (double)t.slots;
    double *c = coef + (size_t)blockIdx.y * 2 * t.slots;
    c[i] = x.x * f;
    c[i + t.slots] = x.y * f;
}
__global__ void k_codec_store_real(const double2 *v, double *vals, uint32_t slots) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= slots) return;
    vals[(size_t)blockIdx.y * slots + i] = v[(size_t)blockIdx.y * slots + i].x;
}

// Garner mixed radix + centred lift of one coefficient whose residue in limb a is res(a) (canonical): the signed
// integer (above (Q-1)/2 -> negative) as fp64.  garner: inv[nl] then G[nl][nl] with G[i][k] = q_k mod q_i.
// dig(a) -> u64&: storage of the nl mixed-radix digits (a private array, or an LDS column per thread).
constexpr int CRT_MAX_LIMBS = 32;
template <class Res, class Dig>
MK_D double crt_centred(Res res, Dig dig, const LimbConst *limb, const u64 *garner, uint32_t nl) {
    dig(0) = res(0);
    for (uint32_t a = 1; a < nl; ++a) {
        const LimbConst la = limb[a];
        const u64 *G = garner + nl + (size_t)a * nl;
        u64 acc = reduce_word(dig(a - 1), la);
        for (int k = (int)a - 2; k >= 0; --k)
            acc = add_mod(mul_mod(acc, G[k], la), reduce_word(dig(k), la), la.q);
        dig(a) = mul_mod(sub_mod(res(a), acc, la.q), garner[a], la);
    }
    bool neg = false;  // above (Q-1)/2 ?  digits compared with (q_a - 1)/2 from the top
    for (int a = (int)nl - 1; a >= 0; --a) {
        const u64 half = (limb[a].q - 1) >> 1;
        const u64 da = dig(a);
        if (da != half) { neg = da > half; break; }
    }
    double acc = 0.0;
    for (int a = (int)nl - 1; a >= 0; --a) {
        const u64 q = limb[a].q;
        const u64 da = dig(a);
        acc = acc * (double)q + (double)(neg ? q - 1 - da : da);
    }
    return neg ? -(acc + 1.0) : acc;
}

// CRT interpolation of a decrypted polynomial (centred lift) -> value / scale as fp64, written bit-reversed into the
// complex work array (folds FFTSpecial's leading bit reversal).  m: [items][nl][N] COEFFICIENT-format residues.
__global__ void k_crt_to_complex(const u64 *m, double2 *v, CodecTables t, const LimbConst *limb, const u64 *garner,
                                 uint32_t nl, double scale) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= t.slots) return;
    const uint32_t n = 2 * t.slots;
    const u64 *mp = m + (size_t)blockIdx.y * nl * n;
    double part[2];
    for (int h = 0; h < 2; ++h) {
        const uint32_t j = i + h * t.slots;
        u64 dig[CRT_MAX_LIMBS];
        part[h] = crt_centred([&](uint32_t a) { return mp[(size_t)a * n + j]; },
                              [&](uint32_t a) -> u64 & { return dig[a]; }, limb, garner, nl) /
                  scale;
    }
    v[(size_t)blockIdx.y * t.slots + brev(i, t.log_slots)] = double2{part[0], part[1]};
}

// ---- Decode with noise flooding (CKKSPackedEncoding::Decode; contract in include/mkckks.h,
// mkckks_decode_flood_batch).  m' = coefficients of m(X^-1) mod X^N + 1 (m'_0 = m_0, m'_j = -m_{N-j});
// d_j = m_j + m_{N-j} (j >= 1) is the part a real message cannot have; the work array gets (m + m') / 2, flooded.
//
// k_crt_symmetrise: thread t < N/4 owns the coefficient quad {t, N/2-t, N/2+t, N-t}, i.e. the work-array positions
// t and N/2-t (thread 0: {0, N/4, N/2, 3N/4} -> positions 0 and N/4).  Sums and differences of a pair are formed in
// the residues and then lifted, so d is exact whenever |d| < 2^53 (every decryption that can pass the check; equal to
// the integer sum of the two lifts whenever that is below Q/2).  Work array: (m + m') / 2 in integer units,
// bit-reversed.  Per block: (e, s1, s2) with e = exponent of max|d| in the block, s1 = sum d 2^-e, s2 = sum (d 2^-e)^2
// over j = 1..N-1 (the power-of-two scaling is exact and keeps s2 finite up to the largest Q).  Fixed reduction order.
// The Garner digits live in dynamic LDS, u64[nl][FLOOD_THREADS] (a column per thread: no scratch).
constexpr int FLOOD_THREADS = 256;
__global__ void __launch_bounds__(FLOOD_THREADS)
    k_crt_symmetrise(const u64 *m, double2 *v, double *part, CodecTables t, const LimbConst *limb, const u64 *garner,
                     uint32_t nl) {
    const uint32_t n = 2 * t.slots, quarter = n / 4, tid = blockIdx.x * FLOOD_THREADS + threadIdx.x;
    const u64 *mp = m + (size_t)blockIdx.y * nl * n;
    double2 *vp = v + (size_t)blockIdx.y * t.slots;
    extern __shared__ u64 dig_lds[];
    // op 0: m_x alone, 1: m_x + m_y, 2: m_x - m_y (mod Q), lifted
    auto lift = [&](uint32_t x, uint32_t y, int op) {
        return crt_centred(
            [&](uint32_t a) {
                const u64 rx = mp[(size_t)a * n + x], ry = mp[(size_t)a * n + y], q = limb[a].q;
                return op == 0 ? rx : op == 1 ? add_mod(rx, ry, q) : sub_mod(rx, ry, q);
            },
            [&](uint32_t a) -> u64 & { return dig_lds[a * FLOOD_THREADS + threadIdx.x]; }, limb, garner, nl);
    };
    double da = 0.0, db = 0.0, wa = 0.0, wb = 0.0;  // the quad's two d values and their multiplicities among j = 1..N-1
    if (tid < quarter) {
        if (tid) {
            const uint32_t a = tid, b = t.slots - tid;  // pairs (a, N-a) and (b, N-b) = (N/2-t, N/2+t)
            const double xa = lift(a, n - a, 2), xb = lift(b, n - b, 2);
            da = lift(a, n - a, 1);
            db = lift(b, n - b, 1);
            wa = wb = 2.0;
            vp[brev(a, t.log_slots)] = double2{0.5 * xa, -0.5 * xb};
            vp[brev(b, t.log_slots)] = double2{0.5 * xb, -0.5 * xa};
        } else {
            const uint32_t c = quarter;  // pair (N/4, 3N/4); position 0: re = m_0, im = (m_{N/2} - m_{N/2}) / 2 = 0
            const double xc = lift(c, n - c, 2);
            vp[0] = double2{lift(0, 0, 0), 0.0};
            vp[brev(c, t.log_slots)] = double2{0.5 * xc, -0.5 * xc};
            da = lift(t.slots, t.slots, 1);  // d_{N/2} = 2 m_{N/2}, once
            db = lift(c, n - c, 1);
            wa = 1.0;
            wb = 2.0;
        }
    }
    __shared__ double red[3][FLOOD_THREADS / 64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double mx = fmax(fabs(da), fabs(db));
    for (int o = 32; o; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    if (!lane) red[0][wave] = mx;
    __syncthreads();
    mx = red[0][0];
    for (int w = 1; w < FLOOD_THREADS / 64; ++w) mx = fmax(mx, red[0][w]);
    int e = 0;
    if (mx > 0.0 && isfinite(mx)) frexp(mx, &e);  // an overflowed lift (inf) stays unscaled and fails the check
    const double xa = ldexp(da, -e), xb = ldexp(db, -e);
    double s1 = wa * xa + wb * xb, s2 = wa * xa * xa + wb * xb * xb;
    for (int o = 32; o; o >>= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if (!lane) {
        red[1][wave] = s1;
        red[2][wave] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        s1 = red[1][0];
        s2 = red[2][0];
        for (int w = 1; w < FLOOD_THREADS / 64; ++w) {
            s1 += red[1][w];
            s2 += red[2][w];
        }
        double *p = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 3;
        p[0] = (double)e;
        p[1] = s1;
        p[2] = s2;
    }
}

// per item, blocks combined in order: stats[item] = {sigma_hat, log2 sigma_hat, sigma_flood * unit, fail}
// mu = sum d / (N-1), sigma_hat^2 = sum (d - mu)^2 / (N-2) = (s2 - s1^2 / (N-1)) / (N-2), in units of
// unit = scale / 2^p (upstream Decode first brings the scaling factor to 2^p; unit = 1 when scale = 2^p);
// fail = !(log2 sigma_hat <= max_log2) (non-finite estimates fail); sigma_flood = sqrt(2) * max(sigma_hat, floor),
// stored in integer units for k_flood
__global__ void k_flood_stats(const double *part, double *stats, uint32_t items, uint32_t nb, uint32_t n,
                              double floor_sigma, double max_log2, double unit) {
    const uint32_t y = blockIdx.x * blockDim.x + threadIdx.x;
    if (y >= items) return;
    const double *p = part + (size_t)y * nb * 3;
    int E = (int)p[0];
    for (uint32_t b = 1; b < nb; ++b) E = max(E, (int)p[3 * b]);
    double s1 = 0.0, s2 = 0.0;
    for (uint32_t b = 0; b < nb; ++b) {
        const int de = (int)p[3 * b] - E;
        s1 += ldexp(p[3 * b + 1], de);
        s2 += ldexp(p[3 * b + 2], 2 * de);
    }
    double sigma = INFINITY, log2s = INFINITY;
    if (isfinite(s1) && isfinite(s2)) {
        const double var = fmax(0.0, (s2 - s1 * s1 / (double)(n - 1)) / (double)(n - 2));  // units of 2^(2E)
        sigma = ldexp(sqrt(var), E) / unit;
        log2s = (double)E + 0.5 * log2(var) - log2(unit);  // -inf when every d is 0
    }
    double *st = stats + (size_t)y * 4;
    st[0] = sigma;
    st[1] = log2s;
    st[2] = M_SQRT2 * fmax(sigma, floor_sigma) * unit;
    st[3] = log2s <= max_log2 ? 0.0 : 1.0;
}

// work array (bit-reversed, integer units) -> (x + stats[2] z) / scale; one thread per storage position, the
// normals of natural position i from chacha_normal_pair(key, sid, item * N/2 + i) (sampler_kernels.hpp)
__global__ void k_flood(double2 *v, const double *stats, CodecTables t, ChaChaKey key, uint32_t sid, double scale) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= t.slots) return;
    const uint32_t i = brev(s, t.log_slots);
    const double2 z = chacha_normal_pair(key, sid, (uint64_t)blockIdx.y * t.slots + i);
    const double sg = stats[(size_t)blockIdx.y * 4 + 2];
    double2 *p = v + (size_t)blockIdx.y * t.slots + s;
    const double2 x = *p;
    *p = double2{(x.x + sg * z.x) / scale, (x.y + sg * z.y) / scale};
}

}  // namespace mk
