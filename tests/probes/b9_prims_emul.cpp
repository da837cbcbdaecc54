// b9_prims_emul.cpp -- CPU emulation of the device primitives, with the entry points of b9_prims_probe.hip, for
// tests/test_prims_host.py: the checkers of tests/prims_check.py must PASS on it and must REJECT each of its mutants
// (b9p_set_mutant), which shows that every check can see the error it is there for -- and lets the suite be developed
// without a GPU.  Built by the test with g++ -ffp-contract=off (every fma below is an explicit std::fma, as on the device).
// The one deliberate difference from the device: the reciprocal seed is the exact 1 / y, not v_rcp_f64's approximation.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

namespace {
int g_mutant = 0;
enum { MUT_LOG_COEF = 1, MUT_LOG_LN2LO = 2, MUT_EXP_COEF = 3, MUT_EXP_LN2LO = 4, MUT_BRACKET_LEN8 = 5, MUT_TREE_ORDER = 6,
       MUT_BOX_NO_INV = 7, MUT_SLACK_SMALL = 8, MUT_F32_BELOW_NEAREST = 9 };
const double INF = std::numeric_limits<double>::infinity();

double log_ge1(double x)
{
    const double Lg1 = 6.666666666666735130e-01 + (g_mutant == MUT_LOG_COEF ? 1e-12 : 0.0), Lg2 = 3.999999999940941908e-01,
                 Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01, Lg5 = 1.818357216161805012e-01,
                 Lg6 = 1.531383769920937332e-01, Lg7 = 1.479819860511658591e-01;
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = g_mutant == MUT_LOG_LN2LO ? 0.0 : 1.90821492927058770002e-10;
    if (!(x < INF)) return std::nan("");           // (+inf / NaN in, NaN out: v_frexp_mant of +inf is +inf, and inf - inf follows)
    int k;
    double m = std::frexp(x, &k);
    const bool lt = m < 0.70710678118654752440;
    m = lt ? m + m : m;
    k = lt ? k - 1 : k;
    const double f = m - 1.0, y = 2.0 + f;
    double r = 1.0 / y;
    r = std::fma(std::fma(-y, r, 1.0), r, r);
    r = std::fma(std::fma(-y, r, 1.0), r, r);
    double sq = f * r;
    sq = std::fma(std::fma(-y, sq, f), r, sq);
    const double z = sq * sq, w = z * z;
    const double t1 = w * std::fma(w, std::fma(w, Lg6, Lg4), Lg2);
    const double t2 = z * std::fma(w, std::fma(w, std::fma(w, Lg7, Lg5), Lg3), Lg1);
    const double R = t1 + t2, hfsq = 0.5 * f * f, dk = (double)k;
    return std::fma(dk, ln2_hi, -((hfsq - std::fma(sq, hfsq + R, dk * ln2_lo)) - f));
}

double exp_fast(double x)
{
    x = x < -750.0 ? -750.0 : (x > 750.0 ? 750.0 : x);
    const double k = std::nearbyint(x * 1.4426950408889634074);
    double r = std::fma(-k, 6.93147180369123816490e-01, x);
    if (g_mutant != MUT_EXP_LN2LO) r = std::fma(-k, 1.90821492927058770002e-10, r);
    double p = 1.0 / 6227020800.0;
    p = std::fma(p, r, 1.0 / 479001600.0); p = std::fma(p, r, 1.0 / 39916800.0); p = std::fma(p, r, 1.0 / 3628800.0);
    p = std::fma(p, r, 1.0 / 362880.0);    p = std::fma(p, r, 1.0 / 40320.0);    p = std::fma(p, r, 1.0 / 5040.0);
    p = std::fma(p, r, 1.0 / 720.0);       p = std::fma(p, r, 1.0 / 120.0);      p = std::fma(p, r, 1.0 / 24.0);
    p = std::fma(p, r, 1.0 / 6.0 + (g_mutant == MUT_EXP_COEF ? 1e-12 : 0.0)); p = std::fma(p, r, 0.5); p = std::fma(p, r, 1.0);
    p = std::fma(p, r, 1.0);
    return std::isnan(k) ? p : std::ldexp(p, (int)k);
}

double log1pexp(double x) { return log_ge1(1.0 + exp_fast(x)); }
double logaddexp(double a, double b)
{
    if (a == -INF) return b;
    if (b == -INF) return a;
    const double hi = a > b ? a : b, lo = a > b ? b : a;
    return hi + log1pexp(lo - hi);
}
double fdiv_(double num, double den)
{
    double r = 1.0 / den;
    r = std::fma(std::fma(-den, r, 1.0), r, r);
    r = std::fma(std::fma(-den, r, 1.0), r, r);
    const double q = num * r;
    return std::fma(std::fma(-den, q, num), r, q);
}
double mix_value(double ea, double l) { return (ea == 0.0 || l > 600.0) ? l : std::log(ea + exp_fast(l)); }

int bracket(const double *ax, int n, double x)
{
    int lo = 0, hi = n - 1;
    if (n < 2) return 0;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (ax[mid] <= x) lo = mid; else hi = mid; }
    return lo;
}
template <bool DESC>
int bracket8(const double *ax, int n, double x)
{
    int lo = 0, len = n - 1;
    if (n < 2) return 0;
    while (len >= 8) {
        const int step = len >> 3;
        int c = 0;
        for (int j = 1; j <= 7; ++j) c += (DESC ? ax[lo + j * step] >= x : ax[lo + j * step] <= x) ? 1 : 0;
        if (g_mutant == MUT_BRACKET_LEN8 && len == 8 && c == 7) c = 6;
        lo += c * step;
        len = (c == 7) ? len - 7 * step : step;
    }
    int c = 0;
    for (int j = 1; j < len; ++j) c += (DESC ? ax[lo + j] >= x : ax[lo + j] <= x) ? 1 : 0;
    return lo + c;
}
void find_bracket(const double *mass, int n, double m, int &lo, double &t)
{
    lo = bracket8<false>(mass, n, m);
    const double a = mass[lo], d = mass[lo + 1] - a;
    const double tq = fdiv_(m - a, d);
    t = d > 0.0 ? tq : 0.0;
}

// lane 0's tree, all lanes updated together
void tree(const double *in, double *v)
{
    std::memcpy(v, in, 64 * sizeof(double));
    static const int order[6] = {32, 16, 8, 4, 2, 1}, swapped[6] = {16, 32, 8, 4, 2, 1};
    for (int s = 0; s < 6; ++s) {
        const int O = g_mutant == MUT_TREE_ORDER ? swapped[s] : order[s];
        double nv[64];
        for (int l = 0; l < 64; ++l) nv[l] = l + O < 64 ? v[l] + v[l + O] : v[l];
        std::memcpy(v, nv, sizeof nv);
    }
}

float f32_below(double x) { return g_mutant == MUT_F32_BELOW_NEAREST ? (float)x : (float)(std::fma(-std::fabs(x), 0x1p-22, x) - 1e-30); }
float f32_above(double x) { return (float)(std::fma(std::fabs(x), 0x1p-22, x) + 1e-30); }

struct Lse { double mx, sm; };
void lse_add(Lse &a, double x)
{
    if (x == -INF) return;
    if (x > a.mx) { a.sm = a.sm * exp_fast(a.mx - x) + 1.0; a.mx = x; }
    else a.sm += exp_fast(x - a.mx);
}
Lse lse_merge(Lse a, Lse b)
{
    if (b.mx == -INF) return a;
    if (a.mx == -INF) return b;
    Lse r;
    if (a.mx >= b.mx) { r.mx = a.mx; r.sm = a.sm + b.sm * exp_fast(b.mx - a.mx); }
    else { r.mx = b.mx; r.sm = b.sm + a.sm * exp_fast(a.mx - b.mx); }
    return r;
}
}  // namespace

extern "C" {

void b9p_set_mutant(int m) { g_mutant = m; }

int b9p_map1(int op, const double *x, double *y, long long n)
{
    for (long long i = 0; i < n; ++i) y[i] = op == 0 || op == 1 ? log_ge1(x[i]) : op == 2 ? exp_fast(x[i]) : op == 3 ? log1pexp(x[i]) : op == 4 ? pow(10.0, x[i]) : log10(x[i]);
    return 0;
}
int b9p_map2(int op, const double *a, const double *b, double *y, long long n)
{
    for (long long i = 0; i < n; ++i) y[i] = op == 0 ? logaddexp(a[i], b[i]) : op == 1 ? fdiv_(a[i], b[i]) : mix_value(a[i], b[i]);
    return 0;
}
int b9p_u01(const unsigned *hi, const unsigned *lo, double *u, double *lg, long long n)
{
    for (long long i = 0; i < n; ++i) {
        const unsigned long long x = ((unsigned long long)(hi[i] >> 5) << 26) + (unsigned long long)(lo[i] >> 6);
        u[i] = ((double)x + 0.5) * (1.0 / 9007199254740992.0);
        u[i] = u[i] < 1.0 ? u[i] : 0x1.fffffffffffffp-1;
        lg[i] = std::log(u[i]);
    }
    return 0;
}
int b9p_philox(const unsigned *ctr, const unsigned *key, unsigned *out, long long n)
{
    for (long long i = 0; i < n; ++i) {
        unsigned c0 = ctr[4 * i], c1 = ctr[4 * i + 1], c2 = ctr[4 * i + 2], c3 = ctr[4 * i + 3], k0 = key[2 * i], k1 = key[2 * i + 1];
        for (int r = 0; r < 10; ++r) {
            const unsigned long long p0 = (unsigned long long)c0 * 0xD2511F53ull, p1 = (unsigned long long)c2 * 0xCD9E8D57ull;
            const unsigned hi0 = (unsigned)(p0 >> 32), lo0 = (unsigned)p0, hi1 = (unsigned)(p1 >> 32), lo1 = (unsigned)p1;
            c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
        out[4 * i] = c0; out[4 * i + 1] = c1; out[4 * i + 2] = c2; out[4 * i + 3] = c3;
    }
    return 0;
}
int b9p_search(int op, int, const double *ax, int n, int cap, const double *x, int *lo, double *t, long long nq)
{
    if (n < 2 || cap < n || (op == 3 && cap < n + 6)) return 1;
    for (long long i = 0; i < nq; ++i) {
        t[i] = 0.0;
        if (op == 0) lo[i] = bracket(ax, n, x[i]);
        else if (op == 1) lo[i] = bracket8<false>(ax, n, x[i]);
        else if (op == 2) lo[i] = bracket8<true>(ax, n, x[i]);
        else find_bracket(ax, n, x[i], lo[i], t[i]);
    }
    return 0;
}
int b9p_lockstep2(const double *a0, int n0, const double *a1, int n1, const double *x, int *lo0, int *lo1, long long nq)
{
    for (long long i = 0; i < nq; ++i) { lo0[i] = bracket8<false>(a0, n0, x[i]); lo1[i] = bracket8<false>(a1, n1, x[i]); }
    return 0;
}
// lanes the comment leaves unspecified keep their own value
int b9p_lane_down_f64(int O, const double *in, double *out, int nw)
{
    for (int w = 0; w < nw; ++w)
        for (int l = 0; l < 64; ++l) {
            const bool spec = O < 16 ? (l % 16) + O < 16 : O == 16 ? ((l / 16) % 2 == 0) : l < 32;
            out[w * 64 + l] = in[w * 64 + (spec ? l + O : l)];
        }
    return 0;
}
int b9p_lane_down_i32(int O, const int *in, int *out, int nw)
{
    for (int w = 0; w < nw; ++w)
        for (int l = 0; l < 64; ++l) {
            const bool spec = O < 16 ? (l % 16) + O < 16 : O == 16 ? ((l / 16) % 2 == 0) : l < 32;
            out[w * 64 + l] = in[w * 64 + (spec ? l + O : l)];
        }
    return 0;
}
int b9p_wave1(int op, const double *in, double *out, int nw)
{
    for (int w = 0; w < nw; ++w) {
        const double *v = in + (size_t)w * 64;
        double *o = out + (size_t)w * 64;
        if (op == 0) tree(v, o);
        else if (op == 1) {
            double m = v[0];
            for (int l = 1; l < 64; ++l) m = v[l] > m ? v[l] : m;
            for (int l = 0; l < 64; ++l) o[l] = m;
        } else for (int l = 0; l < 64; ++l) o[l] = v[0];
    }
    return 0;
}
int b9p_wave_sum7(const double *in, double *out, int nw)
{
    for (int w = 0; w < nw * 7; ++w) {
        double v[64];
        tree(in + (size_t)w * 64, v);
        for (int l = 0; l < 64; ++l) out[(size_t)w * 64 + l] = v[0];
    }
    return 0;
}
int b9p_mix(const double *ea, const double *l, int k, double *total, int nw)
{
    for (int w = 0; w < nw; ++w) {
        double mant[64], add[64];
        int expo[64];
        for (int ln = 0; ln < 64; ++ln) {
            mant[ln] = 0.5; expo[ln] = 1; add[ln] = 0.0;
            for (int j = 0; j < k; ++j) {
                const size_t i = ((size_t)w * k + j) * 64 + ln;
                const bool additive = ea[i] == 0.0 || l[i] > 600.0;
                const double u = additive ? 1.0 : ea[i] + exp_fast(l[i]);
                add[ln] += additive ? l[i] : 0.0;
                int e;
                mant[ln] = std::frexp(mant[ln] * u, &e); expo[ln] += e;
            }
        }
        for (int O = 32; O >= 1; O >>= 1)
            for (int ln = 0; ln < O; ++ln) {
                int e;
                mant[ln] = std::frexp(mant[ln] * mant[ln + O], &e); expo[ln] += expo[ln + O] + e; add[ln] += add[ln + O];
            }
        total[w] = (log_ge1(mant[0] + mant[0]) + (double)(expo[0] - 1) * 0.693147180559945309417) + add[0];
    }
    return 0;
}
int b9p_lse(const double *terms, int n_seq, int n_terms, int parts, double *mx, double *sm)
{
    if (parts < 1 || parts > 64) return 1;
    for (int s = 0; s < n_seq; ++s) {
        Lse a[64];
        for (int p = 0; p < parts; ++p) {
            a[p].mx = -INF; a[p].sm = 0.0;
            const int j0 = (int)((long long)n_terms * p / parts), j1 = (int)((long long)n_terms * (p + 1) / parts);
            for (int j = j0; j < j1; ++j) lse_add(a[p], terms[(size_t)s * n_terms + j]);
        }
        for (int st = 1; st < parts; st *= 2)
            for (int p = 0; p + st < parts; p += 2 * st) a[p] = lse_merge(a[p], a[p + st]);
        mx[s] = a[0].mx; sm[s] = a[0].sm;
    }
    return 0;
}
int b9p_box_store(int nfp, const double *lo, const double *hi, double *box, float *box_f, long long n_box)
{
    for (long long b = 0; b < n_box; ++b)
        for (int f = 0; f < nfp; ++f) {
            const double l = lo[b * nfp + f], h = hi[b * nfp + f];
            const bool any = l <= h;
            box[b * 2 * nfp + f] = any ? l : 0.0; box[b * 2 * nfp + nfp + f] = any ? h : 0.0;
            box_f[b * 2 * nfp + f] = any ? f32_below(l) : 0.0f; box_f[b * 2 * nfp + nfp + f] = any ? f32_above(h) : 0.0f;
        }
    return 0;
}
int b9p_box_bound(int nfp, const double *so, const double *sw, const double *box, const float *box_f, const double *nbm, const double *xcut,
                  double *lb64, double *lb32, double *slack, int *pass64, int *pass32, long long n_box)
{
    for (long long b = 0; b < n_box; ++b) {
        bool p64 = false, p32 = false;
        for (int ln = 0; ln < 64; ++ln) {
            const size_t i = (size_t)b * 64 + ln;
            const double *o = so + i * nfp, *w = sw + i * nfp;
            double lb = 0.0, s2 = 0.0;
            float acc[2] = {0.0f, 0.0f};
            for (int f = 0; f < nfp; ++f) {
                const double a = std::fma(w[f], box[b * 2 * nfp + f], -o[f]), c = std::fma(-w[f], box[b * 2 * nfp + nfp + f], o[f]);
                const double m = std::fmax(std::fmax(a, c), 0.0);
                lb = std::fma(m, m, lb);
                s2 = std::fma(o[f], o[f], s2);
                const float wf = (float)w[f], of = (float)o[f];
                const float af = std::fmaf(wf, box_f[b * 2 * nfp + f], -of), cf = std::fmaf(-wf, box_f[b * 2 * nfp + nfp + f], of);
                const float mf = std::fmax(std::fmax(af, cf), 0.0f);
                acc[f & 1] = std::fmaf(mf, mf, acc[f & 1]);
            }
            lb64[i] = lb;
            lb32[i] = (double)((acc[0] + acc[1]) * (g_mutant == MUT_BOX_NO_INV ? 1.0f : 0.9990234375f));
            slack[i] = s2 < 1e30 ? s2 * (2100.0 / 17592186044416.0) * (g_mutant == MUT_SLACK_SMALL ? 1e-3 : 1.0) : INF;
            p64 = p64 || lb64[i] + nbm[b] < xcut[b];
            p32 = p32 || lb32[i] + nbm[b] <= xcut[b] + slack[i];
        }
        pass64[b] = p64; pass32[b] = p32;
    }
    return 0;
}

}  // extern "C"
