// ubench_fpmod.hip -- exactness + throughput probe: FMA-based modular multiplication for q < 2^51 vs integer Shoup.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cmath>
#include "../ppqsflhe_amd/csrc/ntt_kernels.hpp"  // pm_lazy / pm_fold and the butterflies: the library's own pseudo-Mersenne arithmetic
typedef uint64_t u64;
typedef unsigned __int128 u128;

// the word-splitting form of pm_lazy and the butterfly tail written as u - v + 3q, which the library used before the
// carry-out form: kept here to time the two side by side and to compare their words on the device
namespace split {
__device__ __forceinline__ u64 pm_lazy(u64 a, u64 wt, u64 wxt, const mk::PmK &P) {
    const uint32_t a0 = (uint32_t)a, a1 = (uint32_t)(a >> 32);
    const u64 y0 = (u64)a0 * (uint32_t)wt;
    u64 z = (u64)a0 * (uint32_t)(wt >> 32) + mk::hi32_pair(y0);
    const u64 y1 = (u64)a1 * (uint32_t)wxt + (u64)(uint32_t)y0;
    z = (u64)a1 * (uint32_t)(wxt >> 32) + z;
    z += mk::hi32_pair(y1);
    const u64 lo = (((u64)(uint32_t)z << 32) | (uint32_t)y1) >> P.t;
    return (u64)(uint32_t)(z >> 32) * P.c2 + lo;
}
__device__ __forceinline__ void ct_f(u64 &x, u64 &y, u64 w, u64 wx, const mk::PmK &P) {
    const u64 u = mk::pm_fold(x, P), v = pm_lazy(y, w, wx, P);
    x = u + v;
    y = u - v + P.q3;
}
__device__ __forceinline__ void ct_n(u64 &x, u64 &y, u64 w, u64 wx, const mk::PmK &P) {
    const u64 v = pm_lazy(y, w, wx, P), u = x;
    x = u + v;
    y = u - v + P.q3;
}
__device__ __forceinline__ void gs(u64 &x, u64 &y, u64 w, u64 wx, const mk::PmK &P) {
    const u64 s = x + y, d = x - y + P.q3;
    x = mk::pm_fold(s, P);
    y = pm_lazy(d, w, wx, P);
}
}  // namespace split

// exactness of the pseudo-Mersenne product and butterflies on the device: the library's forms against the splitting forms
// (word for word) and against 128-bit integer arithmetic (residues), random operands with every 3rd / 5th one forced to
// the ends of the ranges (full low word with the largest high word; w = q - 1), and a count of the products whose low sum
// a_lo wt_lo + a_hi wxt_lo carries out of 64 bits -- the case the carry-out form exists for
__global__ void k_check_pm(const u64 *seeds, u64 q, uint32_t k, unsigned long long *bad, unsigned long long *carries, int iters) {
    u64 s = seeds[blockIdx.x * blockDim.x + threadIdx.x];
    mk::LimbConst lc{};
    lc.q = q; lc.k = k; lc.pm_c = (uint32_t)(((u64)1 << k) - q);
    const mk::PmK P = mk::pm_consts(lc);
    const u64 amax = ((u64)8 << k) - 1;
    unsigned long long nbad = 0, ncarry = 0;
    for (int i = 0; i < iters; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        u64 a = (s >> 1) & amax; s = s * 6364136223846793005ull + 1442695040888963407ull;
        u64 w = (u64)(((u128)(s >> 1) * q) >> 63);  // < q
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        u64 x = (s >> 2) & (amax >> 1);  // < 4U: the "n" butterfly's x
        if (i % 3 == 0) a |= 0xffffffffull;
        if (i % 5 == 0) a = amax - (i % 4);
        if (i % 7 == 0) w = q - 1 - (i % 3);
        const u64 wt = w << (63 - k), wxt = (u64)(((u128)w << 32) % q) << (63 - k);
        const u64 r = mk::pm_lazy(a, wt, wxt, P);
        const u64 prod = (u64)((u128)a * w % q);
        if (r != split::pm_lazy(a, wt, wxt, P) || r % q != prod) ++nbad;
        const u128 low = (u128)(uint32_t)a * (uint32_t)wt + (u128)(uint32_t)(a >> 32) * (uint32_t)wxt;
        ncarry += (unsigned)(low >> 64);
        const u64 xm = x % q, sum = (xm + prod) % q, dif = (xm + q - prod) % q;
        u64 x1 = x, y1 = a, x2 = x, y2 = a;
        mk::ct_butterfly_pm_n(x1, y1, wt, wxt, P);
        split::ct_n(x2, y2, wt, wxt, P);
        if (x1 != x2 || y1 != y2 || x1 % q != sum || y1 % q != dif) ++nbad;
        x1 = x2 = s;  // "f" folds any 64-bit x first
        y1 = y2 = a;
        mk::ct_butterfly_pm_f(x1, y1, wt, wxt, P);
        split::ct_f(x2, y2, wt, wxt, P);
        if (x1 != x2 || y1 != y2 || x1 % q != (s % q + prod) % q || y1 % q != (s % q + q - prod) % q) ++nbad;
        // inverse: x, y < 2.375U
        const u64 gx = x >> 1, gy = a >> 2;
        x1 = x2 = gx;
        y1 = y2 = gy;
        mk::gs_butterfly_pm(x1, y1, wt, wxt, P);
        split::gs(x2, y2, wt, wxt, P);
        const u64 gd = (gx % q + q - gy % q) % q;
        if (x1 != x2 || y1 != y2 || x1 % q != (gx % q + gy % q) % q || y1 % q != (u64)((u128)gd * w % q)) ++nbad;
    }
    atomicAdd(bad, nbad);
    atomicAdd(carries, ncarry);
}

// the library's own fp64 primitives (modarith.hpp: __dmul_rn / __fma_rn, no contraction left to the compiler): what is
// timed and checked here is the code that ships.  v = y*w - b*q exactly, |v| <= 1.5 q for |y| <= 2^52 (y, w integers held in
// doubles; wq = w/q rounded); fp_reduce: |result| <= q/2 (+1)
using mk::fp_mulmod;
using mk::fp_reduce;

// exactness: random |y| <= 4q, w < q; compare (fp result mod q) with integer y*w mod q
__global__ void k_check(const u64 *seeds, u64 q, unsigned long long *bad, double *maxabs, int iters) {
    u64 s = seeds[blockIdx.x * blockDim.x + threadIdx.x];
    const double qd = (double)q;
    unsigned long long nbad = 0;
    double mx = 0;
    for (int i = 0; i < iters; ++i) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        u64 a = s; s = s * 6364136223846793005ull + 1442695040888963407ull;
        u64 b = s;
        u64 w = (u64)(((u128)(a >> 1) * q) >> 63);          // < q
        u64 ymag = (u64)(((u128)(b >> 1) * (4 * q)) >> 63);  // < 4q
        if (i % 7 == 0) ymag = 4 * q - 1 - (i % 5);         // edges
        if (i % 11 == 0) w = q - 1 - (i % 3);
        const bool neg = (b & 1);
        double y = neg ? -(double)ymag : (double)ymag;
        double wd = (double)w, wq = wd / qd;
        double v = fp_mulmod(y, wd, wq, qd);
        mx = fmax(mx, fabs(v));
        // integer check
        u64 ref = (u64)((u128)(ymag % q) * w % q);
        if (neg && ref) ref = q - ref;
        double vr = fp_reduce(v, qd, 1.0 / qd);
        long long vi = (long long)vr;
        if (vi < 0) vi += (long long)q;
        if ((u64)vi != ref || v != rint(v)) ++nbad;
    }
    atomicAdd(bad, nbad);
    if (mx > 0) { unsigned long long *p = (unsigned long long *)maxabs; atomicMax(p, (unsigned long long)__double_as_longlong(mx)); }
}

template <int OP>
__global__ void k_rate(double *out, double seed) {
    const double q = 1125899908022273.0, qinv = 1.0 / q;
    double x0 = seed + threadIdx.x, x1 = x0 * 3 + 1, x2 = x0 * 5 + 7, x3 = x0 * 7 + 11;
    double y0 = x0 + 17, y1 = x1 + 19, y2 = x2 + 23, y3 = x3 + 29;
    const double w = 998877665544331.0, wq = w / q;
    u64 a0 = (u64)x0, a1 = (u64)x1, a2 = (u64)x2, a3 = (u64)x3, b0 = (u64)y0, b1 = (u64)y1, b2 = (u64)y2, b3 = (u64)y3;
    const u64 qi = 1125899908022273ull, q2 = 2 * qi, q4 = 4 * qi, wi = 998877665544331ull;
    const u64 wp = (u64)(((u128)wi << 64) / qi);
    for (int i = 0; i < 2048; ++i) {
        if (OP == 0) {  // fp butterfly incl. reducing both outputs every 2nd iteration
#define FPB(x, y) { double v = fp_mulmod(y, w, wq, q); double u = x; x = u + v; y = u - v; if (i & 1) { x = fp_reduce(x, q, qinv); y = fp_reduce(y, q, qinv); } }
            FPB(x0, y0) FPB(x1, y1) FPB(x2, y2) FPB(x3, y3)
        } else if (OP == 1) {  // integer butterfly (c4 correction)
#define INB(x, y) { u64 t = x + (0 - q4); u64 u = (long long)t < 0 ? x : t; u64 h = __umul64hi(y, wp); u64 v = y * wi - h * qi; x = u + v; y = u - v + q2; }
            INB(a0, b0) INB(a1, b1) INB(a2, b2) INB(a3, b3)
        } else if (OP == 3) {  // pseudo-Mersenne butterfly on a 60-bit prime, x folded every 2nd iteration (radix_forward_pm)
            mk::LimbConst lc{};
            lc.q = 1152921504606584833ull; lc.k = 60; lc.pm_c = (uint32_t)((1ull << 60) - lc.q);
            const mk::PmK P = mk::pm_consts(lc);
            const u64 wt = wi << 3, wxt = (u64)(((u128)wi << 32) % lc.q) << 3;
#define PMB(x, y) { if (i & 1) mk::ct_butterfly_pm_n(x, y, wt, wxt, P); else mk::ct_butterfly_pm_f(x, y, wt, wxt, P); }
            PMB(a0, b0) PMB(a1, b1) PMB(a2, b2) PMB(a3, b3)
        } else if (OP == 4) {  // the same with the word-splitting product and the u - v + 3q tail
            mk::LimbConst lc{};
            lc.q = 1152921504606584833ull; lc.k = 60; lc.pm_c = (uint32_t)((1ull << 60) - lc.q);
            const mk::PmK P = mk::pm_consts(lc);
            const u64 wt = wi << 3, wxt = (u64)(((u128)wi << 32) % lc.q) << 3;
#define PMS(x, y) { u64 u = (i & 1) ? x : mk::pm_fold(x, P); u64 v = split::pm_lazy(y, wt, wxt, P); x = u + v; y = u - v + P.q3; }
            PMS(a0, b0) PMS(a1, b1) PMS(a2, b2) PMS(a3, b3)
        } else if (OP == 2) {  // rint rate
            x0 = rint(x0 * 1.0000001) + 0.25; x1 = rint(x1 * 1.0000001) + 0.25; x2 = rint(x2 * 1.0000001) + 0.25; x3 = rint(x3 * 1.0000001) + 0.25;
        }
    }
    out[blockIdx.x * blockDim.x + threadIdx.x] = x0 + x1 + x2 + x3 + y0 + y1 + y2 + y3 + (double)(a0 + a1 + a2 + a3 + b0 + b1 + b2 + b3);
}

template <int OP>
void rate(const char *name, int per_iter) {
    const int blocks = 2048, threads = 256;
    double *out; (void)hipMalloc(&out, (size_t)blocks * threads * 8);
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    k_rate<OP><<<blocks, threads>>>(out, 3.0); (void)hipDeviceSynchronize();
    (void)hipEventRecord(e0);
    for (int r = 0; r < 5; ++r) k_rate<OP><<<blocks, threads>>>(out, 3.0 + r);
    (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
    float ms; (void)hipEventElapsedTime(&ms, e0, e1);
    double waves = (double)blocks * threads / 64, ops = waves * 2048 * per_iter * 5;
    double rate = ops / (ms * 1e-3) / 1024.0;
    printf("%-28s %8.3f ms  => %.1f cycles per wave-%s @2.4GHz\n", name, ms / 5, 2.4e9 / rate, "op");
    (void)hipFree(out);
}

int main() {
    const u64 qs[] = {1125899908022273ull, 1125899904679937ull, 1099511922689ull, 557057ull, (1ull << 51) - 129};
    for (u64 q : qs) {
        const int blocks = 256, threads = 256, iters = 20000;
        u64 *seeds; unsigned long long *bad; double *mx;
        (void)hipMalloc(&seeds, blocks * threads * 8); (void)hipMalloc(&bad, 8); (void)hipMalloc(&mx, 8);
        u64 *h = new u64[blocks * threads];
        for (int i = 0; i < blocks * threads; ++i) h[i] = 0x9E3779B97F4A7C15ull * (i + 1) + q;
        (void)hipMemcpy(seeds, h, blocks * threads * 8, hipMemcpyHostToDevice);
        (void)hipMemset(bad, 0, 8); (void)hipMemset(mx, 0, 8);
        k_check<<<blocks, threads>>>(seeds, q, bad, mx, iters);
        unsigned long long nb; double m;
        (void)hipMemcpy(&nb, bad, 8, hipMemcpyDeviceToHost); (void)hipMemcpy(&m, mx, 8, hipMemcpyDeviceToHost);
        printf("q=%llu (%d bits): %llu mismatches in %.1e trials, max|v|/q = %.3f\n", (unsigned long long)q,
               64 - __builtin_clzll(q), nb, (double)blocks * threads * iters, m / (double)q);
        delete[] h;
    }
    {   // pseudo-Mersenne product and butterflies: the reference context's 60-bit primes, a 55- and a 58-bit prime
        const struct { u64 q; uint32_t k; } pms[] = {{1152921504606748673ull, 60}, {1152921504606683137ull, 60},
                                                     {1152921504606584833ull, 60}, {36028797017456641ull, 55},
                                                     {288230376150630401ull, 58}};
        for (const auto &pm : pms) {
            const int blocks = 256, threads = 256, iters = 2000;
            u64 *seeds; unsigned long long *cnt;
            (void)hipMalloc(&seeds, blocks * threads * 8); (void)hipMalloc(&cnt, 16);
            u64 *h = new u64[blocks * threads];
            for (int i = 0; i < blocks * threads; ++i) h[i] = 0x9E3779B97F4A7C15ull * (i + 1) + pm.q;
            (void)hipMemcpy(seeds, h, blocks * threads * 8, hipMemcpyHostToDevice);
            (void)hipMemset(cnt, 0, 16);
            k_check_pm<<<blocks, threads>>>(seeds, pm.q, pm.k, cnt, cnt + 1, iters);
            unsigned long long c[2] = {~0ull, 0};
            (void)hipMemcpy(c, cnt, 16, hipMemcpyDeviceToHost);
            printf("pm q=%llu (%u bits): %llu mismatches in %.1e products and 3 butterflies each (carry 1 in %llu)\n",
                   (unsigned long long)pm.q, pm.k, c[0], (double)blocks * threads * iters, c[1]);
            delete[] h;
            (void)hipFree(seeds); (void)hipFree(cnt);
        }
    }
    rate<0>("fp64 butterfly (+reduce/2)", 4);
    rate<1>("int Shoup butterfly", 4);
    rate<2>("rint+mul+add", 4);
    rate<3>("int pseudo-Mersenne butterfly", 4);
    rate<4>("  the same, word-splitting form", 4);
    return 0;
}
