// b9_star_moments.hip.h -- b9_star_moments (the starSummary counterpart): k_star_moments (MS/RGB-stage stars, one LANE per star)
// and k_star_moments_wd (WD-stage stars, one WAVE per star).
// Part of the single translation unit b9_kernels.hip (included there, after b9_chain_walk.hip.h); gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------
// Exact per-star posterior moments over a chain ("Per-star posterior moments").  The grid, the node terms
// t_(k, n) and the membership p are b9_sample_mass's; where that call DRAWS one node per (row, star) these kernels form the
// conditional expectations over all of them:  w = exp(t - logsumexp t),  x = {1, p, p sum w M1, p sum w M1^2, p sum w q,
// p sum w q^2, p sum_{q > 0} w, p sum_{k = 1} w}  (B9_MOM_*), written per (row, star) to a scratch [row][star][B9_MOM_N] in the
// caller's star order and then added to the accumulators row by row in ascending order (k_chain_accumulate), one plain add each:
// the result is the same bits however the rows are chunked or split over continued calls.  No random numbers, no atomics.
//
// The node tables are k_marg_table's / k_marg_wd_table's (MargLayout), built by the call into buffers of its own.
//
// k_star_moments: grid (64-star chunk of the mg_* copy, row) x 256, the walk and the pruning of b9_chain_walk.hip.h.  Per
// population a lane keeps an online log-sum-exp state: a reference, S0 = sum e^(t - ref) and the five weighted sums of M1, M1^2,
// q, q^2, [q > 0]; the four waves' states are merged through LDS in wave order 0..3 by wave 0, which mixes the populations,
// forms p and writes the eight increments.
// ------------------------------------------------------------------------------------------
#define B9_MOM_SUMS 6            // S0, then the sums weighted by M1, M1^2, q, q^2, [q > 0]

// one more term t = -X / 2 of a node (m1, q)
__device__ __forceinline__ void mom_term(double t, double m1, double q, double bin, double &ref, double (&s)[B9_MOM_SUMS])
{
    const double e = lse_step(t, ref, [&](double scale) {
#pragma unroll
        for (int c = 0; c < B9_MOM_SUMS; ++c) s[c] *= scale;
    });
    const double em = e * m1, eq = e * q;
    s[0] += e; s[1] += em; s[2] = fma(em, m1, s[2]); s[3] += eq; s[4] = fma(eq, q, s[4]); s[5] = fma(e, bin, s[5]);
}

// A star finished from its per-population log-sums lg[k] (star_finish's) and the populations' conditional means mean[k][0..4] of
// (M1, M1^2, q, q^2, [q > 0]; 0 for a population without a live node): the eight increments.  A star with membership prior 0
// still counts the row (B9_MOM_ROWS) with every other increment 0.
template <int NPOPS>
__device__ __forceinline__ void moments_finish(const double (&lg)[NPOPS], const double (&mean)[NPOPS][5], double c0m, double la,
                                               const double *par, double *__restrict__ out)
{
    double x[B9_MOM_N];
#pragma unroll
    for (int c = 0; c < B9_MOM_N; ++c) x[c] = 0.0;
    double p, wk[NPOPS];
    if (star_finish<NPOPS>(lg, c0m, la, par, p, wk)) {
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < NPOPS; ++k) {
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
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp)
        s_seed[kp][wave][lane] = walk_seed<NFP>((b9_ctab)(tab + (size_t)(w * NPOPS + kp) * L.total), L, (iso[kp].n - 1) * K, Q, wave, so, sw);
    __syncthreads();

    double ref[NPOPS], s[NPOPS][B9_MOM_SUMS];
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        const b9_ctab t_wp = (b9_ctab)(tab + (size_t)(w * NPOPS + kp) * L.total);
        double tmax = walk_start(s_seed[kp], lane);
        ref[kp] = tmax;
#pragma unroll
        for (int c = 0; c < B9_MOM_SUMS; ++c) s[kp][c] = 0.0;
        walk_nodes<NFP>(t_wp, L, (iso[kp].n - 1) * K, Q, wave, dead, cut2, tmax, so, sw, [&](bool live, double x, int node, int j, b9_ctab) {
            const double m1 = marg_primary(iso[kp].mass, node, (iso[kp].n - 1) * K, K, 0).m1;
            if (live) mom_term(-0.5 * x, m1, (double)j / (double)Q, j > 0 ? 1.0 : 0.0, ref[kp], s[kp]);
        });
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
        const WaveMerge m = wave_merge(s_state[kp], lane);
        lg[kp] = (m.S0 > 0.0) ? m.r + log(m.S0) : NEG_INF;
#pragma unroll
        for (int c = 0; c < 5; ++c)
            mean[kp][c] = (m.S0 > 0.0) ? wave_sum(m, &s_state[kp][0][2 + c][lane], (B9_MOM_SUMS + 1) * 64) / m.S0 : 0.0;
    }
    moments_finish<NPOPS>(lg, mean, st.mg_c0m[slot], st.mg_la[slot], par, out);
}

// ------------------------------------------------------------------------------------------
// k_star_moments_wd: the WD-stage stars (b9_chain_walk.hip.h): per lane an online log-sum-exp with the sums weighted by 1, M1 and
// M1^2, merged by the wave's shuffle tree (a fixed order).  Mass ratio 0: the q sums and the binary weight are 0.
// ------------------------------------------------------------------------------------------
template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_moments_wd(DevStars st, double m_wd_up, const IsoHdr *__restrict__ hdr, const double *__restrict__ params,
                                                         int K, const double *__restrict__ wtab, double *__restrict__ scratch)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k_wd = blockIdx.x * 4 + wave, w = blockIdx.y, n_wp = gridDim.y * NPOPS;
    if (k_wd >= st.n_wd) return;
    const WdStar<NFP> ws = wd_star<NFP, NPOPS>(st, hdr, params, k_wd, w);
    double *__restrict__ const out = scratch + ((size_t)w * st.n + ws.orig) * B9_MOM_N;
    if (!ws.valid) {
        if (lane < B9_MOM_N) out[lane] = 0.0;
        return;
    }
    double lg[NPOPS], mean[NPOPS][5];
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        const WdSteps<NFP> sp = wd_steps<NFP>(ws, m_wd_up, hdr, K, wtab, w * NPOPS + kp, n_wp);
        double mx = NEG_INF, s[3] = {0.0, 0.0, 0.0};
        for (int j = 1 + lane; j <= sp.steps; j += 64) {
            const double m1 = sp.m1(j), b[3] = {1.0, m1, m1 * m1};
            lser_merge<3>(mx, s, sp.term(ws, j), b);
        }
        lser_wave<3>(mx, s);
        const bool has = mx != NEG_INF;
        lg[kp] = has ? mx + log(s[0]) : NEG_INF;
        mean[kp][0] = has ? s[1] / s[0] : 0.0; mean[kp][1] = has ? s[2] / s[0] : 0.0;
        mean[kp][2] = mean[kp][3] = mean[kp][4] = 0.0;
    }
    if (lane == 0) moments_finish<NPOPS>(lg, mean, st.c0m[ws.slot], st.la[ws.slot], ws.par, out);
}
