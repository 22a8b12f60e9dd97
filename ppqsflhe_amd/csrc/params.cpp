// params.cpp -- see params.hpp.  Host only; no HIP calls.
#include "params.hpp"

#include <cmath>
#include <cstring>
#include <stdexcept>
#include <string>

namespace mk {

u64 h_mulmod(u64 a, u64 b, u64 m) { return (u64)((u128)a * b % m); }

u64 h_powmod(u64 a, u64 e, u64 m) {
    u64 acc = 1 % m, base = a % m;
    for (; e; e >>= 1) {
        if (e & 1) acc = h_mulmod(acc, base, m);
        base = h_mulmod(base, base, m);
    }
    return acc;
}

u64 h_invmod(u64 a, u64 m) {
    // extended Euclid on signed 128-bit cofactors (m need not be prime)
    __int128 t = 0, nt = 1, r = m, nr = a % m;
    while (nr != 0) {
        __int128 qq = r / nr;
        __int128 tmp = t - qq * nt; t = nt; nt = tmp;
        tmp = r - qq * nr; r = nr; nr = tmp;
    }
    if (r != 1) throw std::invalid_argument("h_invmod: not invertible");
    if (t < 0) t += m;
    return (u64)t;
}

u64 h_shoup(u64 w, u64 q) { return (u64)(((u128)w << 64) / q); }

bool h_is_prime(u64 n) {
    if (n < 4) return n == 2 || n == 3;
    if (!(n & 1)) return false;
    for (u64 p : {3ull, 5ull, 7ull, 11ull, 13ull, 17ull, 19ull, 23ull, 29ull, 31ull, 37ull})
        if (n % p == 0) return n == p;
    u64 odd = n - 1;
    unsigned twos = 0;
    while (!(odd & 1)) { odd >>= 1; ++twos; }
    // witnesses sufficient for all n < 2^64
    for (u64 a : {2ull, 325ull, 9375ull, 28178ull, 450775ull, 9780504ull, 1795265022ull}) {
        u64 x = h_powmod(a % n, odd, n);
        if (a % n == 0 || x == 1 || x == n - 1) continue;
        bool witness = true;
        for (unsigned s = 1; s < twos && witness; ++s) {
            x = h_mulmod(x, x, n);
            if (x == n - 1) witness = false;
        }
        if (witness) return false;
    }
    return true;
}

// OpenFHE's RootOfUnity returns the smallest primitive root of the requested order.
// `order` is a power of two here: x^((q-1)/order) is primitive iff its (order/2)-th
// power is -1; all primitive roots are its odd powers.
u64 h_min_primitive_root(u64 order, u64 q) {
    if ((q - 1) % order) throw std::invalid_argument("modulus is not 1 mod 2N");
    u64 cof = (q - 1) / order, g = 0;
    for (u64 x = 2; !g; ++x) {
        u64 cand = h_powmod(x, cof, q);
        if (h_powmod(cand, order >> 1, q) == q - 1) g = cand;
    }
    u64 step = h_mulmod(g, g, q), walk = g, smallest = g;
    for (u64 i = 1; i < (order >> 1); ++i) {
        walk = h_mulmod(walk, step, q);
        if (walk < smallest) smallest = walk;
    }
    return smallest;
}

namespace {

// walks primes congruent to 1 modulo `step` (the cyclotomic order 2N)
struct PrimeWalk {
    u64 step;
    u64 down(u64 from) const {  // PreviousPrime
        u64 c = from - step;
        while (!h_is_prime(c)) c -= step;
        return c;
    }
    u64 up(u64 from) const {  // NextPrime
        u64 c = from + step;
        while (!h_is_prime(c)) c += step;
        return c;
    }
    u64 first_at(uint32_t bits) const {  // FirstPrime: starts at 2^bits + step + 1 when step | 2^bits
        u64 base = 1ull << bits;
        u64 c = base + (step - base % step) + 1;
        while (!h_is_prime(c)) c += step;
        return c;
    }
    u64 last_below(uint32_t bits) const {  // LastPrime
        u64 c = 1ull << bits;
        u64 r = c % step;
        if (r == 0) c -= step;
        c = c - r + 1;
        while (!h_is_prime(c)) c -= step;
        return c;
    }
};

uint32_t bit_length_of_product(const u64 *m, uint32_t cnt) {
    std::vector<u64> acc{1};
    for (uint32_t i = 0; i < cnt; ++i) {
        u64 carry = 0;
        for (auto &word : acc) {
            u128 t = (u128)word * m[i] + carry;
            word = (u64)t;
            carry = (u64)(t >> 64);
        }
        if (carry) acc.push_back(carry);
    }
    return (uint32_t)(acc.size() - 1) * 64 + (64 - (uint32_t)__builtin_clzll(acc.back()));
}

bool contains(const std::vector<u64> &v, size_t from, size_t to, u64 x) {
    for (size_t i = from; i < to; ++i)
        if (v[i] == x) return true;
    return false;
}

uint32_t reverse_bits(uint32_t x, uint32_t bits) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < bits; ++i, x >>= 1) r = (r << 1) | (x & 1);
    return r;
}

u64 product_mod(const std::vector<u64> &mods, const std::vector<uint32_t> &ids, int skip, u64 m) {
    u64 acc = 1 % m;
    for (size_t k = 0; k < ids.size(); ++k)
        if ((int)k != skip) acc = h_mulmod(acc, mods[ids[k]] % m, m);
    return acc;
}

}  // namespace

LimbConst make_limb_const(u64 q, u64 n) {
    LimbConst c{};
    c.q = q; c.q2 = 2 * q;
    c.k = 64 - (uint32_t)__builtin_clzll(q);
    c.sh = c.k - 2;
    c.mu = (u64)(((u128)1 << (62 + c.k)) / q);
    c.c64 = (u64)(((u128)1 << 64) % q);
    c.ninv = h_invmod(n % q, q);
    c.ninv_sh = h_shoup(c.ninv, q);
    c.qd = (double)q;
    c.qinv = (double)(1.0L / (long double)q);
    c.ninv_d = (double)c.ninv;
    c.ninv_qd = (double)((long double)c.ninv / (long double)q);
    c.fp = 0;  // the engine decides (needs both passes on the radix kernels)
    c.pm = 0;  // the engine decides (integer limbs of the form 2^k - c)
    c.pm_c = 0;
    c.pad_ = 0;
    return c;
}

void fp_table_entry(u64 w, u64 q, u64 &wd_bits, u64 &wq_bits) {
    const double wd = (double)w, wq = (double)((long double)w / (long double)q);
    std::memcpy(&wd_bits, &wd, 8);
    std::memcpy(&wq_bits, &wq, 8);
}

void pm_table_entry(u64 w, const LimbConst &L, u64 &wt, u64 &wxt) {
    wxt = pm_tw_companion(w, L);
    wt = pm_tw(w, L);
}

void ParamSet::generate(uint32_t log_n_, uint32_t depth, uint32_t sbits, uint32_t fbits, uint32_t dn,
                        uint32_t abits, uint32_t ebits) {
    if (log_n_ < 8 || log_n_ > 17) throw std::invalid_argument("log_n must be in [8,17]");
    if (depth < 1 || depth > 30) throw std::invalid_argument("mult_depth must be in [1,30]");
    if (sbits < 20 || sbits > 59 || fbits <= sbits || fbits > 60)
        throw std::invalid_argument("need 20 <= scaling_bits < first_bits <= 60");
    if (abits < 30 || abits > 60 || ebits < 18 || ebits > 30) throw std::invalid_argument("bad aux/extra bits");
    if (dn < 1) throw std::invalid_argument("dnum must be >= 1");
    log_n = log_n_; n = 1u << log_n_;
    mult_depth = depth; scaling_bits = sbits; first_bits = fbits; dnum = dn; aux_bits = abits; extra_bits = ebits;

    const PrimeWalk walk{2ull * n};
    L = depth + 2;  // depth+1 scaling levels + the FLEXIBLEAUTOEXT extra limb
    moduli.assign(L, 0);
    const uint32_t body = L - 1;  // limbs 0..body-1 are the classic FLEXIBLEAUTO chain

    // the chain is filled from the top: q_{body-1} first, then alternately just
    // below / just above the running scaling factor so that sf stays near 2^sbits
    moduli[body - 1] = walk.first_at(sbits);
    double running = (double)moduli[body - 1];
    for (int i = (int)body - 2, turn = 0; i >= 1; --i, ++turn) {
        running = running * running / (double)moduli[i + 1];
        u64 centre = (u64)std::llround(running);
        u64 aligned = centre - centre % walk.step + 1;  // = 1 mod 2N, <= centre
        u64 pick;
        if (turn % 2 == 0) {
            pick = aligned - walk.step;
            do pick = walk.down(pick); while (contains(moduli, i + 1, body, pick));
        } else {
            pick = aligned + walk.step;
            do pick = walk.up(pick); while (contains(moduli, i + 1, body, pick));
        }
        moduli[i] = pick;
    }
    moduli[0] = walk.last_below(fbits);
    moduli[L - 1] = walk.first_at(ebits - 1);

    // HYBRID key switching: digits of alpha limbs, K special primes of abits bits
    alpha = (L + dn - 1) / dn;
    beta = (L + alpha - 1) / alpha;
    if ((int)L - (int)(alpha * (beta - 1)) <= 0) throw std::invalid_argument("dnum does not partition Q");
    uint32_t widest = 0;
    for (uint32_t j = 0; j < beta; ++j) {
        uint32_t lo = j * alpha, hi = std::min(L, lo + alpha);
        widest = std::max(widest, bit_length_of_product(&moduli[lo], hi - lo));
    }
    K = (widest + abits - 1) / abits;
    D = L + K;
    u64 cursor = walk.first_at(abits);
    for (uint32_t i = 0; i < K; ++i) {
        do cursor = walk.down(cursor); while (contains(moduli, 0, L, cursor));
        moduli.push_back(cursor);
    }
    if (alpha > 8 || K > 8) throw std::invalid_argument("digit size / #special primes above 8 unsupported");
    // The chain avoids repeats within itself and P avoids Q, but the extra limb (first prime above 2^(ebits-1)) and q_0
    // are placed on their own: with ebits = sbits + 1, or where primes = 1 mod 2N are sparse (N = 2^16, 20-bit scaling),
    // the extra limb lands on a scaling limb.  Such a basis has no CRT (q_l^-1 mod q_i does not exist: no rescale), so it is refused here.
    for (uint32_t i = 0; i < D; ++i)
        if (contains(moduli, 0, i, moduli[i]))
            throw std::invalid_argument("moduli are not pairwise distinct: too few primes = 1 mod 2N of these widths (raise "
                                        "scaling_bits or extra_bits, or lower log_n)");

    roots.resize(D);
    limb.resize(D);
    for (uint32_t i = 0; i < D; ++i) {
        u64 q = moduli[i];
        roots[i] = h_min_primitive_root(walk.step, q);
        limb[i] = make_limb_const(q, n);
    }

    // scaling factors (FLEXIBLEAUTOEXT): sf[0] = extra limb, sf[1] = q_{L-2}, then sf^2/q going down
    sf.assign(L, 0.0);
    sf_big.assign(L, 0.0);
    sf[0] = (double)moduli[L - 1];
    sf[1] = (double)moduli[L - 2];
    for (uint32_t k = 2; k < L; ++k) sf[k] = sf[k - 1] * sf[k - 1] / (double)moduli[L - k];
    sf_big[0] = sf[0] * sf[1];
    for (uint32_t k = 1; k + 1 < L; ++k) sf_big[k] = sf[k] * sf[k];
}

void ParamSet::twiddles(uint32_t id, bool inverse, std::vector<u64> &w, std::vector<u64> &w_sh) const {
    u64 q = moduli[id];
    u64 base = inverse ? h_invmod(roots[id], q) : roots[id];
    w.assign(n, 0);
    w_sh.assign(n, 0);
    u64 pw = 1;
    for (uint32_t e = 0; e < n; ++e) {
        w[reverse_bits(e, log_n)] = pw;
        pw = h_mulmod(pw, base, q);
    }
    for (uint32_t e = 0; e < n; ++e) w_sh[e] = h_shoup(w[e], q);
}

static BaseConvTable make_table(const std::vector<u64> &mods, std::vector<uint32_t> src, std::vector<uint32_t> dst) {
    BaseConvTable t;
    t.src = std::move(src);
    t.dst = std::move(dst);
    const size_t ni = t.src.size(), no = t.dst.size();
    t.hatinv.resize(ni);
    t.hatinv_sh.resize(ni);
    t.hat.resize(ni * no);
    for (size_t i = 0; i < ni; ++i) {
        u64 si = mods[t.src[i]];
        t.hatinv[i] = h_invmod(product_mod(mods, t.src, (int)i, si), si);
        t.hatinv_sh[i] = h_shoup(t.hatinv[i], si);
        for (size_t j = 0; j < no; ++j) t.hat[i * no + j] = product_mod(mods, t.src, (int)i, mods[t.dst[j]]);
    }
    return t;
}

BaseConvTable ParamSet::modup_table(uint32_t nl, uint32_t part) const {
    uint32_t lo = part * alpha, hi = std::min(nl, lo + alpha);
    std::vector<uint32_t> src, dst;
    for (uint32_t i = lo; i < hi; ++i) src.push_back(i);
    for (uint32_t i = 0; i < nl + K; ++i)
        if (i < lo || i >= hi) dst.push_back(limb_of(i, nl));
    return make_table(moduli, src, dst);
}

BaseConvTable ParamSet::moddown_table(uint32_t nl) const {
    std::vector<uint32_t> src, dst;
    for (uint32_t k = 0; k < K; ++k) src.push_back(L + k);
    for (uint32_t i = 0; i < nl; ++i) dst.push_back(i);
    return make_table(moduli, src, dst);
}

std::vector<u64> hat_as_doubles(const BaseConvTable &t, const std::vector<u64> &moduli) {
    const size_t cnt = t.hat.size(), n_out = t.dst.size();
    std::vector<u64> v(2 * cnt + 2 * n_out);
    auto put = [&](size_t at, u64 h, u64 q) {
        const double hd = (double)h, hq = (double)((long double)h / (long double)q);
        std::memcpy(&v[at], &hd, 8);
        return hq;
    };
    for (size_t e = 0; e < cnt; ++e) {
        const double hq = put(e, t.hat[e], moduli[t.dst[e % n_out]]);
        std::memcpy(&v[cnt + e], &hq, 8);
    }
    for (size_t j = 0; j < n_out; ++j) {
        const u64 q = moduli[t.dst[j]];
        const double hq = put(2 * cnt + j, h_mulmod(t.hat[j], ((u64)1 << 30) % q, q), q);
        std::memcpy(&v[2 * cnt + n_out + j], &hq, 8);
    }
    return v;
}

u64 ParamSet::moddown_scale(uint32_t k) const {
    std::vector<uint32_t> src;
    for (uint32_t i = 0; i < K; ++i) src.push_back(L + i);
    const u64 p = moduli[L + k];
    return h_mulmod(limb[L + k].ninv, h_invmod(product_mod(moduli, src, (int)k, p), p), p);
}

BaseConvTable ParamSet::modup_table_pscaled(uint32_t nl, uint32_t part) const {
    BaseConvTable t = modup_table(nl, part);
    const size_t ni = t.src.size(), no = t.dst.size();
    for (size_t j = 0; j < no; ++j) {
        if (t.dst[j] < L) continue;
        const u64 p = moduli[t.dst[j]], sc = moddown_scale(t.dst[j] - L);
        for (size_t i = 0; i < ni; ++i) t.hat[i * no + j] = h_mulmod(t.hat[i * no + j], sc, p);
    }
    return t;
}

u64 ParamSet::p_mod(uint32_t id) const {
    u64 q = moduli[id], acc = 1;
    for (uint32_t k = 0; k < K; ++k) acc = h_mulmod(acc, moduli[L + k] % q, q);
    return acc;
}
u64 ParamSet::p_inv_mod(uint32_t id) const { return h_invmod(p_mod(id), moduli[id]); }
u64 ParamSet::q_inv_mod(uint32_t l, uint32_t i) const { return h_invmod(moduli[l] % moduli[i], moduli[i]); }

// EvalMult(ct, double): integer constant = trunc(operand * scale + 0.5) as a 128-bit integer, reduced modulo the `count`
// limbs from `first` on (indices into moduli)
static std::vector<u64> const_residues(const std::vector<u64> &moduli, double scale, double operand, uint32_t first,
                                       uint32_t count) {
    int log_sf = (int)std::ceil(std::log2(std::fabs(scale)));
    int log_approx = log_sf > 125 ? log_sf - 125 : 0;
    __int128 big = (__int128)(operand / std::pow(2.0, log_approx) * scale + 0.5);
    std::vector<u64> out(count);
    for (uint32_t i = 0; i < count; ++i) {
        const u64 q = moduli[first + i];
        __int128 m = (__int128)q;
        __int128 r = big % m;
        if (r < 0) r += m;
        u64 f = (u64)r;
        if (log_approx > 0) f = h_mulmod(f, h_powmod(2, (u64)log_approx, q), q);
        out[i] = f;
    }
    return out;
}

std::vector<u64> ParamSet::const_factors(uint32_t nl, uint32_t level, double operand) const {
    return const_residues(moduli, sf.at(level), operand, 0, nl);
}

bool ParamSet::const_fits(uint32_t level, double operand) const {
    if (level >= sf.size() || !std::isfinite(operand)) return false;
    const double scale = sf[level];
    const int log_sf = (int)std::ceil(std::log2(std::fabs(scale)));
    const double v = operand / std::pow(2.0, log_sf > 125 ? log_sf - 125 : 0) * scale;
    return std::isfinite(v) && std::fabs(v) < std::ldexp(1.0, 125);
}

std::vector<u64> ParamSet::const_factors_qp(uint32_t level, double operand) const {
    if (!const_fits(level, operand)) throw std::invalid_argument("weight is not finite or its constant does not fit 125 bits");
    return const_residues(moduli, sf[level], operand, 0, D);
}

void ParamSet::lagrange_at_zero(const uint32_t *parties, uint32_t n_active, u64 *out) const {
    if (!n_active || n_active > LAGRANGE_MAX_PARTIES) throw std::invalid_argument("lagrange: need 1 <= n_active <= 64");
    unsigned long long seen = 0;
    for (uint32_t a = 0; a < n_active; ++a) {
        const uint32_t j = parties[a];
        if (j < 1 || j > LAGRANGE_MAX_PARTIES) throw std::invalid_argument("lagrange: party index outside [1, 64]");
        if (seen >> (j - 1) & 1) throw std::invalid_argument("lagrange: duplicate party index");
        seen |= 1ull << (j - 1);
    }
    for (uint32_t a = 0; a < n_active; ++a)
        for (uint32_t l = 0; l < L; ++l) {
            const u64 q = moduli[l], j = parties[a];
            u64 num = 1, den = 1;  // prod m, prod (m - j) over the other members; indices <= 64 < q
            for (uint32_t b = 0; b < n_active; ++b) {
                if (b == a) continue;
                const u64 m = parties[b];
                num = h_mulmod(num, m, q);
                den = h_mulmod(den, m > j ? m - j : q - (j - m), q);
            }
            out[(size_t)a * L + l] = h_mulmod(num, h_invmod(den, q), q);
        }
}

// ---- polynomial evaluation: plan, ladder scales, weights and constants (include/mkckks.h: "polynomial evaluation") ------

static uint32_t ceil_log2(uint32_t v) {
    uint32_t r = 0;
    while ((1u << r) < v) ++r;
    return r;
}

void ParamSet::power_ladder(uint32_t nl, uint32_t n_pow, double scale_in, uint32_t *nl_out, double *scale_out) const {
    if (nl < 1 || nl > L) throw std::invalid_argument("nl out of range");
    if (n_pow < 1 || n_pow > 64) throw std::invalid_argument("n_pow must be in [1, 64]");
    if (ceil_log2(n_pow) >= nl) throw std::invalid_argument("the power ladder needs nl - ceil(log2 n_pow) >= 1 limbs");
    std::vector<uint32_t> nlk(n_pow + 1);
    std::vector<double> sk(n_pow + 1);
    nlk[1] = nl;
    sk[1] = scale_in;
    for (uint32_t k = 2; k <= n_pow; ++k) {
        const uint32_t i = (k + 1) / 2, j = k - i;
        nlk[k] = nlk[i] - 1;
        const double prod = sk[i] * sk[j];
        sk[k] = prod / (double)moduli[nlk[i] - 1];
    }
    for (uint32_t k = 1; k <= n_pow; ++k) {
        if (nl_out) nl_out[k - 1] = nlk[k];
        if (scale_out) scale_out[k - 1] = sk[k];
    }
}

PolyPlan ParamSet::poly_plan(uint32_t degree, uint32_t nl) const {
    if (degree < 2 || degree > POLY_MAX_DEGREE) throw std::invalid_argument("degree must be in [2, 63]");
    if (nl < 1 || nl > L) throw std::invalid_argument("nl out of range");
    PolyPlan p{};
    p.B = 2;
    while (p.B * p.B < degree + 1) p.B *= 2;
    p.G = (degree + p.B) / p.B;  // ceil((degree + 1) / B)
    const uint32_t log_b = ceil_log2(p.B), log_g = ceil_log2(p.G - 1);
    p.depth = log_b + log_g + 2;
    if (nl < p.depth + 1)
        throw std::invalid_argument("degree " + std::to_string(degree) + " needs " + std::to_string(p.depth + 1) +
                                    " limbs, the input has " + std::to_string(nl));
    p.nl_T = nl - log_b - log_g;
    p.nl_out = p.nl_T - 2;
    p.n_relin = (p.B - 1) + (p.G - 2) + 1;
    for (uint32_t i = 1; i < p.B; ++i) p.baby_nl[i - 1] = nl - ceil_log2(i);
    for (uint32_t j = 1; j < p.G; ++j) p.giant_nl[j - 1] = nl - log_b - ceil_log2(j);
    return p;
}

double ParamSet::poly_weights(const double *coef, uint32_t degree, uint32_t nl, double scale_in, double *w) const {
    const PolyPlan p = poly_plan(degree, nl);
    if (!(scale_in > 0) || !std::isfinite(scale_in)) throw std::invalid_argument("scale must be positive and finite");
    for (uint32_t k = 0; k <= degree; ++k)
        if (!std::isfinite(coef[k])) throw std::invalid_argument("coefficient " + std::to_string(k) + " is not finite");
    double sx[POLY_MAX_B + 1], sy[POLY_MAX_B];  // sx[i]: scale of x^i, sx[B] that of y; sy[j]: scale of y^j
    uint32_t nlx[POLY_MAX_B];
    power_ladder(nl, p.B, scale_in, nlx, sx + 1);
    sx[0] = sy[0] = 1.0;
    power_ladder(nlx[p.B - 1], p.G - 1, sx[p.B], nullptr, sy + 1);
    const double s_out = sf.at(L - p.nl_out);
    const double sigma = s_out * (double)moduli[p.nl_T - 1] * (double)moduli[p.nl_T - 2];
    for (uint32_t j = 0; j < p.G; ++j)
        for (uint32_t i = 0; i < p.B; ++i) {
            const uint32_t k = j * p.B + i;
            const double c = k <= degree ? coef[k] : 0.0;
            const double den = sx[i] * sy[j];
            w[k] = c == 0.0 ? 0.0 : c * (sigma / den);
        }
    return s_out;
}

std::vector<u64> ParamSet::poly_constants(const double *w, uint32_t count, uint32_t nl_T) const {
    if (nl_T < 1 || nl_T > L) throw std::invalid_argument("nl_T out of range");
    long double half = 0.5L;
    for (uint32_t t = 0; t < nl_T; ++t) half *= (long double)moduli[t];
    std::vector<u64> out((size_t)count * nl_T);
    for (uint32_t k = 0; k < count; ++k) {
        if (!std::isfinite(w[k])) throw std::invalid_argument("weight " + std::to_string(k) + " is not finite");
        const double a = std::fabs(w[k]);
        if ((long double)a >= half)
            throw std::invalid_argument("weight " + std::to_string(k) + " does not fit half the modulus of its level");
        // M = rint(|w|) as m * 2^sh: below 2^63 the rounded double converts exactly; above, a double is m * 2^sh with m < 2^53
        u64 m;
        int sh = 0;
        if (a < 9223372036854775808.0) {
            m = (u64)std::nearbyint(a);
        } else {
            const double f = std::frexp(a, &sh);  // a = f * 2^sh, 0.5 <= f < 1
            m = (u64)std::ldexp(f, 53);
            sh -= 53;
        }
        for (uint32_t t = 0; t < nl_T; ++t) {
            const u64 q = moduli[t];
            u64 r = m % q;
            if (sh) r = h_mulmod(r, h_powmod(2, (u64)sh, q), q);
            out[(size_t)k * nl_T + t] = (w[k] < 0 && r) ? q - r : r;
        }
    }
    return out;
}

// ---- Chebyshev series: T_{jB+i} = 2 T_i T_{jB} - T_{(j-1)B+(B-i)} for j >= 1, 0 < i < B, applied from the top block down

double ParamSet::cheb_weights(const double *coef, uint32_t degree, uint32_t nl, double scale_in, double *w) const {
    const PolyPlan p = poly_plan(degree, nl);
    for (uint32_t k = 0; k <= degree; ++k)
        if (!std::isfinite(coef[k])) throw std::invalid_argument("coefficient " + std::to_string(k) + " is not finite");
    const uint32_t B = p.B, G = p.G;
    std::vector<double> c((size_t)B * G, 0.0), m((size_t)B * G, 0.0);
    std::copy(coef, coef + degree + 1, c.begin());
    for (uint32_t j = G - 1; j >= 1; --j) {
        for (uint32_t i = B - 1; i >= 1; --i) {
            m[j * B + i] = 2.0 * c[j * B + i];
            c[(j - 1) * B + (B - i)] -= c[j * B + i];
        }
        m[j * B] = c[j * B];
    }
    for (uint32_t i = 0; i < B; ++i) m[i] = c[i];
    // B * G - 1 has the plan of `degree`: B is the smallest power of two with B^2 >= degree + 1, so (B / 2)^2 < B * G
    return poly_weights(m.data(), B * G - 1, nl, scale_in, w);
}

}  // namespace mk
