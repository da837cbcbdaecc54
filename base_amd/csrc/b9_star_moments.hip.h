// b9_star_moments.hip.h -- b9_star_moments (the starSummary counterpart): k_star_moments (MS/RGB-stage stars, one LANE per star),
// k_star_moments_wd (WD-stage stars, one WAVE per star) and k_moments_accumulate (the per-star accumulators).
// Part of the single translation unit b9_kernels.hip (included there, after b9_star_marg.hip.h); gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------
// Exact per-star posterior moments over a chain ("Per-star posterior moments").  The grid, the node terms
// t_(k, n) and the membership p are b9_sample_mass's; where that call DRAWS one node per (row, star) these kernels form the
// conditional expectations over all of them:  w = exp(t - logsumexp t),  x = {1, p, p sum w M1, p sum w M1^2, p sum w q,
// p sum w q^2, p sum_{q > 0} w, p sum_{k = 1} w}  (B9_MOM_*), written per (row, star) to a scratch [row][star][B9_MOM_N] in the
// caller's star order and then added to the accumulators row by row in ascending order, one plain add each: the result is the
// same bits however the rows are chunked or split over continued calls.  No random numbers, no atomics.
//
// The node tables are k_marg_table's / k_marg_wd_table's (MargLayout), built by the call into buffers of its own.
//
// k_star_moments: grid (64-star chunk of the mg_* copy, row) x 256.  The four waves of a workgroup hold the SAME 64 stars and
// take the units (16 nodes x one mass ratio) of every 64-node chunk by k_star_marg's diagonal rule -- unit (sub, j) is wave
// (2 sub + j) mod 4's: a function of the layout only.  A unit's words are wave-uniform and reach the lanes as scalar loads
// through b9_ctab.  Per population a lane keeps an online log-sum-exp state: a reference, S0 = sum e^(t - ref) and the five
// weighted sums of M1, M1^2, q, q^2, [q > 0]; the four waves' states are merged through LDS in wave order 0..3 by wave 0, which
// mixes the populations, forms p and writes the eight increments.
//
// Pruning (rigorous, a function of the data only): every wave starts from the SAME lower bound of the star's largest term --
// the best term among every 16th node at mass ratio 0, the four waves' shares merged behind a barrier -- and from there on
// follows its own running maximum; a term counts while it lies within B9_MARG_CUT e-folds of that bound, and a chunk / a unit
// whose box (k_marg_table's fp64 boxes) excludes that for every lane is skipped.  What is dropped is below N_nodes e^-40 of the
// star's sum.  No field floor: the weights are conditional on membership, so a field star's posterior over the grid counts in full.
// ------------------------------------------------------------------------------------------
#define B9_MOM_SUMS 6            // S0, then the sums weighted by M1, M1^2, q, q^2, [q > 0]

// one more term t = -X / 2 of a node (m1, q): reference fixed while terms stay within 600 e-folds above it (lse_term's scheme)
__device__ __forceinline__ void mom_term(double t, double m1, double q, double bin, double &ref, double (&s)[B9_MOM_SUMS])
{
    const double d = t - ref;
    double e;
    if (__ballot(d > 600.0) != 0ull) {
        const bool up = d > 600.0;
        const double f = exp_marg(max_vs(up ? -d : d, -700.0));
        const double scale = up ? f : 1.0;
#pragma unroll
        for (int c = 0; c < B9_MOM_SUMS; ++c) s[c] *= scale;
        e = up ? 1.0 : f;
        ref = up ? t : ref;
    } else {
        e = exp_marg(max_vs(d, -700.0));
    }
    const double em = e * m1, eq = e * q;
    s[0] += e; s[1] += em; s[2] = fma(em, m1, s[2]); s[3] += eq; s[4] = fma(eq, q, s[4]); s[5] = fma(e, bin, s[5]);
}

// A star finished from its per-population log-sums lg[k] = log sum_n e^(t_(k, n)) (the star's constant c0m NOT included; -inf: no
// live node) and the populations' conditional means mean[k][0..4] of (M1, M1^2, q, q^2, [q > 0]): the eight increments.  The
// membership is finish_star's l and v, as b9_sample_mass forms it; the populations' weights e^(log lambda_k + lg_k) / sum do not
// need c0m, so a star with membership prior 0 still counts the row (B9_MOM_ROWS) with every other increment 0.
template <int NPOPS>
__device__ __forceinline__ void moments_finish(const double (&lg)[NPOPS], const double (&mean)[NPOPS][5], double c0m, double la,
                                               const double *par, double *__restrict__ out)
{
    double a[NPOPS], ll[NPOPS];
    bool any = false;
#pragma unroll
    for (int k = 0; k < NPOPS; ++k) {
        a[k] = lg[k];
        if (NPOPS == 2) { const double lam = par[B9_P_LAMBDA]; a[k] = (lg[k] == NEG_INF) ? NEG_INF : (k ? log1p(-lam) : log(lam)) + lg[k]; }
        ll[k] = (lg[k] == NEG_INF) ? NEG_INF : c0m + lg[k];
        any = any || a[k] != NEG_INF;
    }
    double x[B9_MOM_N];
#pragma unroll
    for (int c = 0; c < B9_MOM_N; ++c) x[c] = 0.0;
    if (any) {
        const StarFinish fin = finish_star<NPOPS>(ll, par, la);
        const double p = (fin.l == NEG_INF) ? 0.0 : exp(fin.l - fin.v);
        double wk[NPOPS];
        wk[0] = 1.0;
        if (NPOPS == 2) {
            const double A = logaddexp(a[0], a[NPOPS - 1]);
#pragma unroll
            for (int k = 0; k < NPOPS; ++k) wk[k] = (a[k] == NEG_INF) ? 0.0 : exp(a[k] - A);
        }
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < NPOPS; ++k)
            if (a[k] != NEG_INF) {
#pragma unroll
                for (int c = 0; c < 5; ++c) m[c] += wk[k] * mean[k][c];
            }
        x[B9_MOM_ROWS] = 1.0; x[B9_MOM_MEMBER] = p;
        x[B9_MOM_M1] = p * m[0]; x[B9_MOM_M1SQ] = p * m[1]; x[B9_MOM_Q] = p * m[2]; x[B9_MOM_QSQ] = p * m[3]; x[B9_MOM_BINARY] = p * m[4];
        x[B9_MOM_POP1] = NPOPS == 2 ? p * wk[NPOPS - 1] : 0.0;
    }
#pragma unroll
    for (int c = 0; c < B9_MOM_N; ++c) out[c] = x[c];
}

template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_moments(DevStars st, const IsoHdr *__restrict__ hdr, const double *__restrict__ iso_data,
                                                      long long iso_stride, int mass_cap, const double *__restrict__ params, int K, int Q,
                                                      const double *__restrict__ tab, MargLayout L, double cut2, double *__restrict__ scratch)
{
    __shared__ double s_seed[NPOPS][4][64];
    __shared__ double s_state[NPOPS][4][B9_MOM_SUMS + 1][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sc = blockIdx.x, w = blockIdx.y;
    const int slot = sc * 64 + lane, orig = st.mg_perm[slot];
    const bool dead = orig < 0;
    double so[NFP], sw[NFP];
#pragma unroll
    for (int f = 0; f < NFP; ++f) { so[f] = st.mg_so[B9_SIDX(NFP, f, slot)]; sw[f] = st.mg_sw[B9_SIDX(NFP, f, slot)]; }
    const double *par = params + (size_t)w * B9_NPARAM;
    double *__restrict__ const out = scratch + ((size_t)w * st.n + (dead ? 0 : orig)) * B9_MOM_N;
    IsoView<NFP> iso[NPOPS];
    double tip_min;
    const bool valid = load_iso_views<NFP, NPOPS>(hdr, iso_data, iso_stride, mass_cap, w, iso, tip_min);
    if (!valid) {                                        // a row outside the grid contributes nothing
        if (wave == 0 && !dead) {
#pragma unroll
            for (int c = 0; c < B9_MOM_N; ++c) out[c] = 0.0;
        }
        return;
    }

    // ---- the seed pass: this wave's share of every 16th node at mass ratio 0
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        const b9_ctab t_wp = (b9_ctab)(tab + (size_t)(w * NPOPS + kp) * L.total);
        const int n_units = (((iso[kp].n - 1) * K + 63) >> 6) * 4;
        double xmin = __builtin_inf();
        for (int u = wave; u < n_units; u += 4)
            xmin = __builtin_fmin(xmin, row_x<NFP>(t_wp + L.o_rows + (size_t)u * Q * 16 * NFP, t_wp[L.o_nb + u * 16], so, sw));
        s_seed[kp][wave][lane] = -0.5 * xmin;
    }
    __syncthreads();

    double ref[NPOPS], s[NPOPS][B9_MOM_SUMS];
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        const b9_ctab t_wp = (b9_ctab)(tab + (size_t)(w * NPOPS + kp) * L.total);
        const int n_nodes = (iso[kp].n - 1) * K, n_chunks = (n_nodes + 63) >> 6;
        // the lower bound every wave starts from, and the lane's running maximum
        double tmax = __builtin_fmax(__builtin_fmax(s_seed[kp][0][lane], s_seed[kp][1][lane]), __builtin_fmax(s_seed[kp][2][lane], s_seed[kp][3][lane]));
        ref[kp] = tmax;
#pragma unroll
        for (int c = 0; c < B9_MOM_SUMS; ++c) s[kp][c] = 0.0;
        for (int c = 0; c < n_chunks; ++c) {
            double xcut = dead ? NEG_INF : fma(-2.0, tmax, cut2);                 // a term counts while X < xcut
            if (__ballot(box_bound64<NFP>(t_wp + L.o_box1 + (size_t)c * 2 * NFP, so, sw) + t_wp[L.o_nbmin64 + c] < xcut) == 0ull) continue;
            for (int sub = 0; sub < 4; ++sub) {
                const int u = c * 4 + sub;
                const double nbm = t_wp[L.o_nbmin16 + u];
                for (int j = (wave - 2 * sub) & 3; j < Q; j += 4) {
                    if (__ballot(box_bound64<NFP>(t_wp + L.o_box2 + ((size_t)u * Q + j) * 2 * NFP, so, sw) + nbm < xcut) == 0ull) continue;
                    const b9_ctab rowp = t_wp + L.o_rows + ((size_t)u * Q + j) * 16 * NFP;
                    const double q = (double)j / (double)Q, bin = j > 0 ? 1.0 : 0.0;
                    for (int i = 0; i < 16; ++i) {
                        const int node = u * 16 + i;
                        const double x = row_x<NFP>(rowp + i * NFP, t_wp[L.o_nb + node], so, sw);
                        const bool live = x < xcut;
                        if (__ballot(live) == 0ull) continue;
                        const double m1 = marg_primary(iso[kp].mass, node, n_nodes, K, 0).m1;
                        if (live) {
                            const double t = -0.5 * x;
                            mom_term(t, m1, q, bin, ref[kp], s[kp]);
                            tmax = max_vv(tmax, t);
                        }
                    }
                    xcut = dead ? NEG_INF : fma(-2.0, tmax, cut2);
                }
            }
        }
        s_state[kp][wave][0][lane] = ref[kp];
#pragma unroll
        for (int c = 0; c < B9_MOM_SUMS; ++c) s_state[kp][wave][1 + c][lane] = s[kp][c];
    }
    __syncthreads();
    if (wave != 0 || dead) return;

    // ---- wave 0: the four shares merged in wave order, the star finished
    double lg[NPOPS], mean[NPOPS][5];
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        double r = NEG_INF;
#pragma unroll
        for (int k = 0; k < 4; ++k) r = (s_state[kp][k][1][lane] > 0.0 && s_state[kp][k][0][lane] > r) ? s_state[kp][k][0][lane] : r;
        double S[B9_MOM_SUMS];
#pragma unroll
        for (int c = 0; c < B9_MOM_SUMS; ++c) S[c] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (s_state[kp][k][1][lane] > 0.0) {
                const double f = exp_fast(s_state[kp][k][0][lane] - r);
#pragma unroll
                for (int c = 0; c < B9_MOM_SUMS; ++c) S[c] += s_state[kp][k][1 + c][lane] * f;
            }
        lg[kp] = (S[0] > 0.0) ? r + log(S[0]) : NEG_INF;
#pragma unroll
        for (int c = 0; c < 5; ++c) mean[kp][c] = (S[0] > 0.0) ? S[1 + c] / S[0] : 0.0;
    }
    moments_finish<NPOPS>(lg, mean, st.mg_c0m[slot], st.mg_la[slot], par, out);
}

// ------------------------------------------------------------------------------------------
// k_star_moments_wd: the WD-stage stars, one wavefront per (row, star) as in k_star_marg_wd: lanes stride over the 8 K steps
// m_j = tip + dM j (j = 1 .. 8 K) of k_marg_wd_table's rows; per lane an online log-sum-exp with the sums weighted by M1 and
// M1^2, merged by the wave's shuffle tree (a fixed order).  Mass ratio 0: the q sums and the binary weight are 0.
// Grid: (ceil(n_wd / 4), rows) x 256.
// ------------------------------------------------------------------------------------------
struct LseM { double mx, s0, s1, s2; };
__device__ __forceinline__ LseM lsem_merge(const LseM &a, const LseM &b)
{
    if (b.mx == NEG_INF) return a;
    if (a.mx == NEG_INF) return b;
    const bool a_hi = a.mx >= b.mx;
    const double f = exp_fast(a_hi ? b.mx - a.mx : a.mx - b.mx);
    const double fa = a_hi ? 1.0 : f, fb = a_hi ? f : 1.0;
    LseM r;
    r.mx = a_hi ? a.mx : b.mx;
    r.s0 = a.s0 * fa + b.s0 * fb; r.s1 = a.s1 * fa + b.s1 * fb; r.s2 = a.s2 * fa + b.s2 * fb;
    return r;
}

template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_moments_wd(DevStars st, double m_wd_up, const IsoHdr *__restrict__ hdr, const double *__restrict__ params,
                                                         int K, const double *__restrict__ wtab, double *__restrict__ scratch)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k_wd = blockIdx.x * 4 + wave, w = blockIdx.y, n_wp = gridDim.y * NPOPS, steps = 8 * K;
    if (k_wd >= st.n_wd) return;
    const int slot = st.wd_slot[k_wd], orig = st.perm[slot];
    double obs[NFP], wgt[NFP];
#pragma unroll
    for (int f = 0; f < NFP; ++f) { obs[f] = st.obs[B9_SIDX(NFP, f, slot)]; wgt[f] = st.w[B9_SIDX(NFP, f, slot)]; }
    const int wd_type = st.flags[slot] & 1;
    const double *par = params + (size_t)w * B9_NPARAM;
    double *__restrict__ const out = scratch + ((size_t)w * st.n + orig) * B9_MOM_N;
    bool valid = true;
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) valid = valid && hdr[w * NPOPS + kp].valid;
    if (!valid) {
        if (lane < B9_MOM_N) out[lane] = 0.0;
        return;
    }
    double lg[NPOPS], mean[NPOPS][5];
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        const int wp = w * NPOPS + kp;
        const double tip = hdr[wp].agb_tip, dM = (m_wd_up - tip) / steps;
        LseM acc; acc.mx = NEG_INF; acc.s0 = acc.s1 = acc.s2 = 0.0;
        if (dM > 0.0) {
            const double log_w = log(dM);
            const double *__restrict__ const rows = wtab + (((size_t)wp * 2 + wd_type) * steps) * NFP;      // k_marg_wd_table's
            const double *__restrict__ const lpm = wtab + (size_t)n_wp * 2 * steps * NFP + (size_t)wp * steps;
            for (int j = 1 + lane; j <= steps; j += 64) {
                const double *__restrict__ const r = rows + (size_t)(j - 1) * NFP;
                double chi2 = 0.0;
#pragma unroll
                for (int f = 0; f < NFP; ++f) { const double d = r[f] - obs[f]; chi2 = fma(wgt[f] * d, d, chi2); }
                if (isfinite(chi2)) {
                    const double term = (lpm[j - 1] - 0.5 * chi2) + log_w, m1 = tip + dM * j;
                    LseM b; b.mx = term; b.s0 = 1.0; b.s1 = m1; b.s2 = m1 * m1;
                    acc = lsem_merge(acc, b);
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            LseM b; b.mx = __shfl_down(acc.mx, o, 64); b.s0 = __shfl_down(acc.s0, o, 64); b.s1 = __shfl_down(acc.s1, o, 64); b.s2 = __shfl_down(acc.s2, o, 64);
            acc = lsem_merge(acc, b);
        }
        const bool has = acc.mx != NEG_INF;
        lg[kp] = has ? acc.mx + log(acc.s0) : NEG_INF;
        mean[kp][0] = has ? acc.s1 / acc.s0 : 0.0; mean[kp][1] = has ? acc.s2 / acc.s0 : 0.0;
        mean[kp][2] = mean[kp][3] = mean[kp][4] = 0.0;
    }
    if (lane == 0) moments_finish<NPOPS>(lg, mean, st.c0m[slot], st.la[slot], par, out);
}

// k_moments_accumulate: one lane per (star, component): acc += x_r for the chunk's rows r in ascending order, one plain add each
__global__ __launch_bounds__(256) void k_moments_accumulate(const double *__restrict__ scratch, int n_rows, long long n_words, double *__restrict__ acc)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_words) return;
    double a = acc[i];
    for (int r = 0; r < n_rows; ++r) a = a + scratch[(size_t)r * n_words + i];
    acc[i] = a;
}
