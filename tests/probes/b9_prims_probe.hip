// b9_prims_probe.hip -- test-only probe of the device primitives the kernels share: it includes the SHIPPED headers,
// unchanged, in b9_kernels.hip's order, and wraps the primitives in kernels that only apply them to arrays.  No arithmetic
// is restated here.  Built by base_amd.build.build_probe() with exactly HIP_FLAGS (so -ffp-contract=off, no fast-math: the
// inlined functions perform the IEEE operations they perform in the shipped kernels) into build/probes/libb9prims.so; not
// part of libbase9hip.so, not part of the ABI, outside csrc/ (build.source_hash() does not cover it).
// tests/prims_probe.py holds the ctypes bindings, tests/test_gpu_prims.py the tests.
//
// Every host entry validates its lengths, allocates, copies in, launches ONCE, synchronises, copies out and returns the
// HIP status (hipErrorInvalidValue for a rejected argument).  No kernel indexes with a value it was given as data.
#include "../../base_amd/csrc/b9_device.h"
#include "../../base_amd/csrc/b9_launch.h"
#include <algorithm>
#include <cstring>
#include "../../include/base9_hip.h"

#include "../../base_amd/csrc/b9_diag.hip.h"
#include "../../base_amd/csrc/b9_common.hip.h"
#include "../../base_amd/csrc/b9_derive.hip.h"
#include "../../base_amd/csrc/b9_star.hip.h"
#include "../../base_amd/csrc/b9_star_like.hip.h"
#include "../../base_amd/csrc/b9_star_marg.hip.h"

#include <vector>

namespace {

// device buffer with the host copies around it; the first failing call's status sticks
struct Bufs {
    hipError_t e = hipSuccess;
    std::vector<void *> all;
    ~Bufs() { for (void *p : all) (void)hipFree(p); }
    template <class T> T *in(const T *h, size_t n)
    {
        T *d = out<T>(n);
        if (e == hipSuccess && n) e = hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice);
        return d;
    }
    template <class T> T *out(size_t n)
    {
        void *d = nullptr;
        if (e == hipSuccess) e = hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(T));
        if (e == hipSuccess) { all.push_back(d); e = hipMemset(d, 0xff, std::max<size_t>(n, 1) * sizeof(T)); }
        return (T *)d;
    }
    template <class T> void back(T *h, const T *d, size_t n)
    {
        if (e == hipSuccess && n) e = hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost);
    }
    void ran()
    {
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
};

constexpr long long MAX_N = 1ll << 22;
inline bool bad_n(long long n) { return n < 1 || n > MAX_N; }
inline int blocks(long long n) { return (int)((n + 255) / 256); }

// ---------------------------------------------------------------------------------------------------------------------
// element-wise maps
// ---------------------------------------------------------------------------------------------------------------------
enum { M1_LOG_GE1 = 0, M1_LOG_POS = 1, M1_EXP_FAST = 2, M1_LOG1PEXP = 3, M1_EXP10 = 4, M1_LOG10 = 5 };   // 4, 5: the library calls of wd_chain
template <int OP>
__global__ void k_map1(const double *__restrict__ x, double *__restrict__ y, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    y[i] = OP == M1_LOG_GE1 ? log_ge1(v) : OP == M1_LOG_POS ? log_pos(v) : OP == M1_EXP_FAST ? exp_fast(v) : OP == M1_LOG1PEXP ? log1pexp(v)
         : OP == M1_EXP10 ? exp10(v) : log10(v);
}

enum { M2_LOGADDEXP = 0, M2_FDIV = 1, M2_MIX_VALUE = 2 };
template <int OP>
__global__ void k_map2(const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ y, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    y[i] = OP == M2_LOGADDEXP ? logaddexp(a[i], b[i]) : OP == M2_FDIV ? fdiv(a[i], b[i]) : mix_value(a[i], b[i]);
}

__global__ void k_u01(const unsigned *__restrict__ hi, const unsigned *__restrict__ lo, double *__restrict__ u, double *__restrict__ lg, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = u01(hi[i], lo[i]);
    u[i] = v; lg[i] = log(v);          // (the library log, as metropolis_accept takes it)
}

__global__ void k_philox(const unsigned *__restrict__ ctr, const unsigned *__restrict__ key, unsigned *__restrict__ out, long long n)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned r[4];
    philox4x32(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3], key[2 * i], key[2 * i + 1], r);
    for (int k = 0; k < 4; ++k) out[4 * i + k] = r[k];
}

// ---------------------------------------------------------------------------------------------------------------------
// searches.  The axis holds n nodes in a column of `cap` doubles (what follows the nodes is the caller's padding); LDS = 1
// stages the whole column in LDS first, as the hot and heavy roles do.
// ---------------------------------------------------------------------------------------------------------------------
enum { S_BRACKET = 0, S_BRACKET8 = 1, S_BRACKET8_DESC = 2, S_FIND = 3 };
template <int OP>
__device__ __forceinline__ void search_one(const double *ax, int n, double x, int &lo, double &t)
{
    t = 0.0;
    if (OP == S_BRACKET) lo = bracket(ax, n, x);
    else if (OP == S_BRACKET8) lo = bracket8<false>(ax, n, x);
    else if (OP == S_BRACKET8_DESC) lo = bracket8<true>(ax, n, x);
    else find_bracket(ax, n, x, lo, t);
}
template <int OP, bool LDS>
__global__ void k_search(const double *__restrict__ ax, int n, int cap, const double *__restrict__ x, int *__restrict__ lo, double *__restrict__ t, long long nq)
{
    extern __shared__ __attribute__((aligned(16))) double s_ax[];
    if (LDS) {
        for (int j = threadIdx.x; j < cap; j += 256) s_ax[j] = ax[j];
        __syncthreads();
    }
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    int l; double tt;
    if (LDS) search_one<OP>(s_ax, n, x[i], l, tt); else search_one<OP>(ax, n, x[i], l, tt);
    lo[i] = l; t[i] = tt;
}

__global__ void k_lockstep2(const double *__restrict__ a0, int n0, const double *__restrict__ a1, int n1, const double *__restrict__ x,
                            int *__restrict__ lo0, int *__restrict__ lo1, long long nq)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq) return;
    const double *const axes[2] = {a0, a1};
    const int n[2] = {n0, n1};
    int lo[2];
    bracket8_lockstep<2>(axes, n, x[i], lo);
    lo0[i] = lo[0]; lo1[i] = lo[1];
}

// ---------------------------------------------------------------------------------------------------------------------
// wave primitives: one wave (64 threads) per block, full EXEC
// ---------------------------------------------------------------------------------------------------------------------
template <int O, class T>
__global__ __launch_bounds__(64) void k_lane_down(const T *__restrict__ in, T *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    out[i] = lane_down<O>(in[i]);
}

enum { W_SUM = 0, W_MAX_ALL = 1, W_BCAST0 = 2, W_UNIFORM = 3 };
template <int OP>
__global__ __launch_bounds__(64) void k_wave1(const double *__restrict__ in, double *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    const double v = in[i];
    out[i] = OP == W_SUM ? wave_sum(v) : OP == W_MAX_ALL ? wave_max_all(v) : OP == W_BCAST0 ? wave_bcast0(v) : wave_uniform(v);
}

__global__ __launch_bounds__(64) void k_wave_sum7(const double *__restrict__ in, double *__restrict__ out)      // [wave][7][64] both
{
    const size_t b = (size_t)blockIdx.x * 7 * 64 + threadIdx.x;
    double a[7], S[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) a[k] = in[b + (size_t)k * 64];
    wave_sum7(a, S);
#pragma unroll
    for (int k = 0; k < 7; ++k) out[b + (size_t)k * 64] = S[k];
}

// ---------------------------------------------------------------------------------------------------------------------
// accumulators
// ---------------------------------------------------------------------------------------------------------------------
// a wave multiplies k factors per lane into a MixAcc that starts at 1.0 the way hot_groups starts it; [wave][k][64] inputs
__global__ __launch_bounds__(64) void k_mix(const double *__restrict__ ea, const double *__restrict__ l, int k, double *__restrict__ total)
{
    const size_t b = (size_t)blockIdx.x * k * 64 + threadIdx.x;
    MixAcc acc;
    acc.mant = 0.5; acc.expo = 1; acc.add = 0.0;
    for (int j = 0; j < k; ++j) mix_add(acc, ea[b + (size_t)j * 64], l[b + (size_t)j * 64]);
    const double tot = mix_wave_total(acc);
    if (threadIdx.x == 0) total[blockIdx.x] = tot;
}

// sequence s: n_terms terms dealt in contiguous runs over `parts` accumulators (each from {-inf, 0}), merged in a tree
#define LSE_MAX_PARTS 64
__global__ void k_lse(const double *__restrict__ terms, int n_seq, int n_terms, int parts, double *__restrict__ mx, double *__restrict__ sm)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n_seq) return;
    Lse a[LSE_MAX_PARTS];
    for (int p = 0; p < parts; ++p) {
        a[p].mx = NEG_INF; a[p].sm = 0.0;
        const int j0 = (int)((long long)n_terms * p / parts), j1 = (int)((long long)n_terms * (p + 1) / parts);
        for (int j = j0; j < j1; ++j) lse_add(a[p], terms[(size_t)s * n_terms + j]);
    }
    for (int st = 1; st < parts; st *= 2)
        for (int p = 0; p + st < parts; p += 2 * st) a[p] = lse_merge(a[p], a[p + st]);
    mx[s] = a[0].mx; sm[s] = a[0].sm;
}

// ---------------------------------------------------------------------------------------------------------------------
// box pruning.  A wave holds 64 stars and tests ONE box (the box is wave-uniform in the kernels: a scalar operand), so
// box b pairs with stars [64 b, 64 b + 64).  The boxes are written by one launch (box_store, as the table builders do)
// and read by another (through the constant address space, as the star loop does).
// ---------------------------------------------------------------------------------------------------------------------
template <int NFP>
__global__ void k_box_store(const double *__restrict__ lo, const double *__restrict__ hi, double *__restrict__ box, double *__restrict__ box_f, long long n_box)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;          // (box, filter)
    if (i >= n_box * NFP) return;
    const long long b = i / NFP;
    const int f = (int)(i - b * NFP);
    box_store<NFP>(true, box + b * 2 * NFP, box_f + b * NFP, f, lo[i], hi[i]);
}

template <int NFP>
__global__ __launch_bounds__(64) void k_box_bound(const double *__restrict__ so_g, const double *__restrict__ sw_g, const double *box, const double *box_f,
                                                  const double *__restrict__ nbm, const double *__restrict__ xcut,
                                                  double *__restrict__ lb64, double *__restrict__ lb32, double *__restrict__ slack,
                                                  int *__restrict__ pass64, int *__restrict__ pass32)
{
    __shared__ b9_f4 s_sf[(NFP / 2) * 64];
    __shared__ double s_slack[64];
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x, i = b * 64 + lane;
    double so[NFP], sw[NFP];
#pragma unroll
    for (int f = 0; f < NFP; ++f) { so[f] = so_g[i * NFP + f]; sw[f] = sw_g[i * NFP + f]; }
    const double sl = box_stage<NFP>(s_sf, lane, true, so, sw);
    s_slack[lane] = sl;
    __syncthreads();
    const double nb = wave_uniform(nbm[b]), xc = wave_uniform(xcut[b]);
    lb64[i] = box_bound64<NFP>((b9_ctab)box + b * 2 * NFP, so, sw);
    lb32[i] = box_bound32<NFP>((b9_cbox)box_f + b * NFP, s_sf, lane);
    slack[i] = sl;
    const bool p64 = box_pass<NFP, false>((b9_ctab)box, b, nb, xc, so, sw, s_sf, s_slack, lane);
    const bool p32 = box_pass<NFP, true>((b9_ctab)box_f, b, nb, xc, so, sw, s_sf, s_slack, lane);
    if (lane == 0) { pass64[b] = p64 ? 1 : 0; pass32[b] = p32 ? 1 : 0; }
}

template <int NFP>
int run_box_store(const double *lo, const double *hi, double *box, float *box_f, long long n_box)
{
    Bufs B;
    const size_t n = (size_t)n_box * NFP;
    const double *d_lo = B.in(lo, n), *d_hi = B.in(hi, n);
    double *d_box = B.out<double>(2 * n), *d_bf = B.out<double>(n);
    if (B.e == hipSuccess) hipLaunchKernelGGL((k_box_store<NFP>), dim3(blocks((long long)n)), dim3(256), 0, 0, d_lo, d_hi, d_box, d_bf, n_box);
    B.ran();
    B.back(box, d_box, 2 * n);
    B.back(reinterpret_cast<double *>(box_f), d_bf, n);
    return (int)B.e;
}

template <int NFP>
int run_box_bound(const double *so, const double *sw, const double *box, const float *box_f, const double *nbm, const double *xcut,
                  double *lb64, double *lb32, double *slack, int *pass64, int *pass32, long long n_box)
{
    Bufs B;
    const size_t ns = (size_t)n_box * 64, nb = (size_t)n_box * NFP;
    const double *d_so = B.in(so, ns * NFP), *d_sw = B.in(sw, ns * NFP), *d_box = B.in(box, 2 * nb);
    const double *d_bf = B.in(reinterpret_cast<const double *>(box_f), nb), *d_nbm = B.in(nbm, (size_t)n_box), *d_xc = B.in(xcut, (size_t)n_box);
    double *d_64 = B.out<double>(ns), *d_32 = B.out<double>(ns), *d_sl = B.out<double>(ns);
    int *d_p64 = B.out<int>((size_t)n_box), *d_p32 = B.out<int>((size_t)n_box);
    if (B.e == hipSuccess) hipLaunchKernelGGL((k_box_bound<NFP>), dim3((unsigned)n_box), dim3(64), 0, 0, d_so, d_sw, d_box, d_bf, d_nbm, d_xc, d_64, d_32, d_sl, d_p64, d_p32);
    B.ran();
    B.back(lb64, d_64, ns); B.back(lb32, d_32, ns); B.back(slack, d_sl, ns);
    B.back(pass64, d_p64, (size_t)n_box); B.back(pass32, d_p32, (size_t)n_box);
    return (int)B.e;
}

template <int OP>
int run_map1(const double *x, double *y, long long n)
{
    Bufs B;
    const double *d_x = B.in(x, (size_t)n);
    double *d_y = B.out<double>((size_t)n);
    if (B.e == hipSuccess) hipLaunchKernelGGL((k_map1<OP>), dim3(blocks(n)), dim3(256), 0, 0, d_x, d_y, n);
    B.ran();
    B.back(y, d_y, (size_t)n);
    return (int)B.e;
}

template <int OP>
int run_map2(const double *a, const double *b, double *y, long long n)
{
    Bufs B;
    const double *d_a = B.in(a, (size_t)n), *d_b = B.in(b, (size_t)n);
    double *d_y = B.out<double>((size_t)n);
    if (B.e == hipSuccess) hipLaunchKernelGGL((k_map2<OP>), dim3(blocks(n)), dim3(256), 0, 0, d_a, d_b, d_y, n);
    B.ran();
    B.back(y, d_y, (size_t)n);
    return (int)B.e;
}

template <int OP, bool LDS>
int run_search(const double *ax, int n, int cap, const double *x, int *lo, double *t, long long nq)
{
    Bufs B;
    const double *d_ax = B.in(ax, (size_t)cap), *d_x = B.in(x, (size_t)nq);
    int *d_lo = B.out<int>((size_t)nq);
    double *d_t = B.out<double>((size_t)nq);
    if (B.e == hipSuccess)
        hipLaunchKernelGGL((k_search<OP, LDS>), dim3(blocks(nq)), dim3(256), LDS ? sizeof(double) * (size_t)cap : 0, 0, d_ax, n, cap, d_x, d_lo, d_t, nq);
    B.ran();
    B.back(lo, d_lo, (size_t)nq); B.back(t, d_t, (size_t)nq);
    return (int)B.e;
}

template <int O, class T>
int run_lane_down(const T *in, T *out, int n_waves)
{
    Bufs B;
    const T *d_in = B.in(in, (size_t)n_waves * 64);
    T *d_out = B.out<T>((size_t)n_waves * 64);
    if (B.e == hipSuccess) hipLaunchKernelGGL((k_lane_down<O, T>), dim3(n_waves), dim3(64), 0, 0, d_in, d_out);
    B.ran();
    B.back(out, d_out, (size_t)n_waves * 64);
    return (int)B.e;
}
template <class T>
int lane_down_any(int O, const T *in, T *out, int n_waves)
{
    if (n_waves < 1 || n_waves > 65536) return (int)hipErrorInvalidValue;
    switch (O) {
    case 1: return run_lane_down<1, T>(in, out, n_waves);
    case 2: return run_lane_down<2, T>(in, out, n_waves);
    case 4: return run_lane_down<4, T>(in, out, n_waves);
    case 8: return run_lane_down<8, T>(in, out, n_waves);
    case 16: return run_lane_down<16, T>(in, out, n_waves);
    case 32: return run_lane_down<32, T>(in, out, n_waves);
    default: return (int)hipErrorInvalidValue;
    }
}

template <int OP>
int run_wave1(const double *in, double *out, int n_waves)
{
    Bufs B;
    const double *d_in = B.in(in, (size_t)n_waves * 64);
    double *d_out = B.out<double>((size_t)n_waves * 64);
    if (B.e == hipSuccess) hipLaunchKernelGGL((k_wave1<OP>), dim3(n_waves), dim3(64), 0, 0, d_in, d_out);
    B.ran();
    B.back(out, d_out, (size_t)n_waves * 64);
    return (int)B.e;
}

}  // namespace

extern "C" {

int b9p_map1(int op, const double *x, double *y, long long n)
{
    if (bad_n(n) || !x || !y) return (int)hipErrorInvalidValue;
    switch (op) {
    case M1_LOG_GE1: return run_map1<M1_LOG_GE1>(x, y, n);
    case M1_LOG_POS: return run_map1<M1_LOG_POS>(x, y, n);
    case M1_EXP_FAST: return run_map1<M1_EXP_FAST>(x, y, n);
    case M1_LOG1PEXP: return run_map1<M1_LOG1PEXP>(x, y, n);
    case M1_EXP10: return run_map1<M1_EXP10>(x, y, n);
    case M1_LOG10: return run_map1<M1_LOG10>(x, y, n);
    default: return (int)hipErrorInvalidValue;
    }
}

int b9p_map2(int op, const double *a, const double *b, double *y, long long n)
{
    if (bad_n(n) || !a || !b || !y) return (int)hipErrorInvalidValue;
    switch (op) {
    case M2_LOGADDEXP: return run_map2<M2_LOGADDEXP>(a, b, y, n);
    case M2_FDIV: return run_map2<M2_FDIV>(a, b, y, n);
    case M2_MIX_VALUE: return run_map2<M2_MIX_VALUE>(a, b, y, n);
    default: return (int)hipErrorInvalidValue;
    }
}

int b9p_u01(const unsigned *hi, const unsigned *lo, double *u, double *log_u, long long n)
{
    if (bad_n(n) || !hi || !lo || !u || !log_u) return (int)hipErrorInvalidValue;
    Bufs B;
    const unsigned *d_hi = B.in(hi, (size_t)n), *d_lo = B.in(lo, (size_t)n);
    double *d_u = B.out<double>((size_t)n), *d_l = B.out<double>((size_t)n);
    if (B.e == hipSuccess) hipLaunchKernelGGL(k_u01, dim3(blocks(n)), dim3(256), 0, 0, d_hi, d_lo, d_u, d_l, n);
    B.ran();
    B.back(u, d_u, (size_t)n); B.back(log_u, d_l, (size_t)n);
    return (int)B.e;
}

// ctr[n][4], key[n][2] -> out[n][4]
int b9p_philox(const unsigned *ctr, const unsigned *key, unsigned *out, long long n)
{
    if (bad_n(n) || !ctr || !key || !out) return (int)hipErrorInvalidValue;
    Bufs B;
    const unsigned *d_c = B.in(ctr, (size_t)n * 4), *d_k = B.in(key, (size_t)n * 2);
    unsigned *d_o = B.out<unsigned>((size_t)n * 4);
    if (B.e == hipSuccess) hipLaunchKernelGGL(k_philox, dim3(blocks(n)), dim3(256), 0, 0, d_c, d_k, d_o, n);
    B.ran();
    B.back(out, d_o, (size_t)n * 4);
    return (int)B.e;
}

// ax[cap]: n nodes, then padding.  find_bracket's last round reads ax[lo + 1 .. lo + 7] with lo <= n - 2, so it needs
// n + 6 <= cap; the others never read past the nodes.  lds != 0: the column is staged in LDS first (cap <= 4096).
int b9p_search(int op, int lds, const double *ax, int n, int cap, const double *x, int *lo, double *t, long long nq)
{
    if (bad_n(nq) || !ax || !x || !lo || !t || n < 2 || cap < n || cap > 4096) return (int)hipErrorInvalidValue;
    if (op == S_FIND && cap < n + 6) return (int)hipErrorInvalidValue;
    switch (op * 2 + (lds ? 1 : 0)) {
    case S_BRACKET * 2: return run_search<S_BRACKET, false>(ax, n, cap, x, lo, t, nq);
    case S_BRACKET * 2 + 1: return run_search<S_BRACKET, true>(ax, n, cap, x, lo, t, nq);
    case S_BRACKET8 * 2: return run_search<S_BRACKET8, false>(ax, n, cap, x, lo, t, nq);
    case S_BRACKET8 * 2 + 1: return run_search<S_BRACKET8, true>(ax, n, cap, x, lo, t, nq);
    case S_BRACKET8_DESC * 2: return run_search<S_BRACKET8_DESC, false>(ax, n, cap, x, lo, t, nq);
    case S_BRACKET8_DESC * 2 + 1: return run_search<S_BRACKET8_DESC, true>(ax, n, cap, x, lo, t, nq);
    case S_FIND * 2: return run_search<S_FIND, false>(ax, n, cap, x, lo, t, nq);
    case S_FIND * 2 + 1: return run_search<S_FIND, true>(ax, n, cap, x, lo, t, nq);
    default: return (int)hipErrorInvalidValue;
    }
}

// bracket8_lockstep<2>, the one width the kernels instantiate (two cooling tracks)
int b9p_lockstep2(const double *a0, int n0, const double *a1, int n1, const double *x, int *lo0, int *lo1, long long nq)
{
    if (bad_n(nq) || !a0 || !a1 || !x || !lo0 || !lo1 || n0 < 2 || n1 < 2 || n0 > 4096 || n1 > 4096) return (int)hipErrorInvalidValue;
    Bufs B;
    const double *d_a0 = B.in(a0, (size_t)n0), *d_a1 = B.in(a1, (size_t)n1), *d_x = B.in(x, (size_t)nq);
    int *d_l0 = B.out<int>((size_t)nq), *d_l1 = B.out<int>((size_t)nq);
    if (B.e == hipSuccess) hipLaunchKernelGGL(k_lockstep2, dim3(blocks(nq)), dim3(256), 0, 0, d_a0, n0, d_a1, n1, d_x, d_l0, d_l1, nq);
    B.ran();
    B.back(lo0, d_l0, (size_t)nq); B.back(lo1, d_l1, (size_t)nq);
    return (int)B.e;
}

// in / out: [n_waves][64]
int b9p_lane_down_f64(int O, const double *in, double *out, int n_waves) { return (in && out) ? lane_down_any<double>(O, in, out, n_waves) : (int)hipErrorInvalidValue; }
int b9p_lane_down_i32(int O, const int *in, int *out, int n_waves) { return (in && out) ? lane_down_any<int>(O, in, out, n_waves) : (int)hipErrorInvalidValue; }

int b9p_wave1(int op, const double *in, double *out, int n_waves)
{
    if (n_waves < 1 || n_waves > 65536 || !in || !out) return (int)hipErrorInvalidValue;
    switch (op) {
    case W_SUM: return run_wave1<W_SUM>(in, out, n_waves);
    case W_MAX_ALL: return run_wave1<W_MAX_ALL>(in, out, n_waves);
    case W_BCAST0: return run_wave1<W_BCAST0>(in, out, n_waves);
    case W_UNIFORM: return run_wave1<W_UNIFORM>(in, out, n_waves);
    default: return (int)hipErrorInvalidValue;
    }
}

// in / out: [n_waves][7][64]
int b9p_wave_sum7(const double *in, double *out, int n_waves)
{
    if (n_waves < 1 || n_waves > 8192 || !in || !out) return (int)hipErrorInvalidValue;
    Bufs B;
    const size_t n = (size_t)n_waves * 7 * 64;
    const double *d_in = B.in(in, n);
    double *d_out = B.out<double>(n);
    if (B.e == hipSuccess) hipLaunchKernelGGL(k_wave_sum7, dim3(n_waves), dim3(64), 0, 0, d_in, d_out);
    B.ran();
    B.back(out, d_out, n);
    return (int)B.e;
}

// ea, l: [n_waves][k][64] -> total[n_waves]
int b9p_mix(const double *ea, const double *l, int k, double *total, int n_waves)
{
    if (n_waves < 1 || n_waves > 8192 || k < 1 || k > 1024 || !ea || !l || !total) return (int)hipErrorInvalidValue;
    Bufs B;
    const size_t n = (size_t)n_waves * k * 64;
    const double *d_ea = B.in(ea, n), *d_l = B.in(l, n);
    double *d_t = B.out<double>((size_t)n_waves);
    if (B.e == hipSuccess) hipLaunchKernelGGL(k_mix, dim3(n_waves), dim3(64), 0, 0, d_ea, d_l, k, d_t);
    B.ran();
    B.back(total, d_t, (size_t)n_waves);
    return (int)B.e;
}

// terms: [n_seq][n_terms] -> mx[n_seq], sm[n_seq]
int b9p_lse(const double *terms, int n_seq, int n_terms, int parts, double *mx, double *sm)
{
    if (n_seq < 1 || n_seq > 65536 || n_terms < 1 || n_terms > 65536 || parts < 1 || parts > LSE_MAX_PARTS || !terms || !mx || !sm) return (int)hipErrorInvalidValue;
    Bufs B;
    const double *d_t = B.in(terms, (size_t)n_seq * n_terms);
    double *d_mx = B.out<double>((size_t)n_seq), *d_sm = B.out<double>((size_t)n_seq);
    if (B.e == hipSuccess) hipLaunchKernelGGL(k_lse, dim3((n_seq + 63) / 64), dim3(64), 0, 0, d_t, n_seq, n_terms, parts, d_mx, d_sm);
    B.ran();
    B.back(mx, d_mx, (size_t)n_seq); B.back(sm, d_sm, (size_t)n_seq);
    return (int)B.e;
}

// lo, hi: [n_box][nfp] -> box [n_box][2][nfp] doubles, box_f [n_box][2][nfp] floats
int b9p_box_store(int nfp, const double *lo, const double *hi, double *box, float *box_f, long long n_box)
{
    if (n_box < 1 || n_box > 65536 || !lo || !hi || !box || !box_f) return (int)hipErrorInvalidValue;
    switch (nfp) {
    case 2: return run_box_store<2>(lo, hi, box, box_f, n_box);
    case 4: return run_box_store<4>(lo, hi, box, box_f, n_box);
    case 8: return run_box_store<8>(lo, hi, box, box_f, n_box);
    case 16: return run_box_store<16>(lo, hi, box, box_f, n_box);
    default: return (int)hipErrorInvalidValue;
    }
}

// so, sw: [n_box][64][nfp]; box, box_f as b9p_box_store wrote them; nbm, xcut: [n_box]
// -> lb64, lb32, slack: [n_box][64]; pass64, pass32: [n_box]
int b9p_box_bound(int nfp, const double *so, const double *sw, const double *box, const float *box_f, const double *nbm, const double *xcut,
                  double *lb64, double *lb32, double *slack, int *pass64, int *pass32, long long n_box)
{
    if (n_box < 1 || n_box > 65536 || !so || !sw || !box || !box_f || !nbm || !xcut || !lb64 || !lb32 || !slack || !pass64 || !pass32)
        return (int)hipErrorInvalidValue;
    switch (nfp) {
    case 2: return run_box_bound<2>(so, sw, box, box_f, nbm, xcut, lb64, lb32, slack, pass64, pass32, n_box);
    case 4: return run_box_bound<4>(so, sw, box, box_f, nbm, xcut, lb64, lb32, slack, pass64, pass32, n_box);
    case 8: return run_box_bound<8>(so, sw, box, box_f, nbm, xcut, lb64, lb32, slack, pass64, pass32, n_box);
    case 16: return run_box_bound<16>(so, sw, box, box_f, nbm, xcut, lb64, lb32, slack, pass64, pass32, n_box);
    default: return (int)hipErrorInvalidValue;
    }
}

}  // extern "C"
