// b9_wd_moments.hip.h -- b9_wd_moments (the wdSummary counterpart): k_wd_moments, one LANE per WD-stage star against
// k_wd_node_table_status' table: k_wd_node_table's (the same body, b9_wd_sample.hip.h) with every node's wd_chain status kept.
// Part of the single translation unit b9_kernels.hip (included there, after b9_wd_sample.hip.h); gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------
// Exact per-WD posterior moments over a chain (include/base9_hip.h).  The grid, the terms and the membership
// are b9_sample_wd_mass's; where k_wd_sample keeps ONE node per (row, star), this kernel forms the conditional expectations over
// all of them:  w = exp(t - logsumexp t),  x = {1, p, p sum_{k = 1} w, p sum_cooled w, p sum w m, p sum w m^2, and p sum_cooled w v,
// p sum_cooled w v^2 for the five derived values v}  (B9_WDM_*), written per (row, star) to a scratch [row][n_wd][B9_WDM_N] in the
// order of b9_sample_wd_mass's columns; k_chain_accumulate adds the rows to the accumulators in ascending order.
//
// The table: k_wd_node_table's, built by its sibling k_wd_node_table_status with one more part behind `der`:
//   stat [wp][n_nodes]               wd_chain's status of the node as a double (2.0: a white dwarf with every derived value set)
// b9_sample_wd_mass builds and k_wd_sample reads the table without it, as before.
//
// k_wd_moments is wd_grid_walk's frame (b9_wd_sample.hip.h) on wd_star's lane, with the walk WRITTEN OUT and the derived values and
// the status of a tile's nodes staged beside the rows: through wd_grid_walk the call took 0.94 - 0.97 ms against 0.88 - 0.91 ms
// (1000 WD-stage stars, 256 rows, 512 nodes; docs/LABNOTES.md section 31), in both forms of its stage callback.  The loop below
// and wd_grid_walk's must stay the same statement: test_ties_to_wd_moments and test_ties_to_sample_wd_mass hold them together.
// ORDER OF THE SUMS (a function of the data only): a star's terms enter its population's online log-sum-exp (lse_step: the
// reference stays while terms lie within 600 e-folds above it; every sum is rescaled together on the rare jump) one by one in
// ascending node order j = 1 .. n_nodes, by this one lane; a lane that does not jump while a launch-mate does multiplies by 1.0.
// The populations are then mixed as b9_star_moments mixes them (star_finish).  Nothing depends on the chunk of rows, the grid,
// the call or the other lanes.
// ------------------------------------------------------------------------------------------
#define B9_WDM_SUMS 14           // S0, then the sums weighted by m, m^2, [cooled], and [cooled] (v, v^2) of the five derived values
#define B9_WDM_NODE_DOUBLES(nfp) (B9_WDS_NODE_DOUBLES(nfp) + 1)      // table doubles per (row, population, node), status included

template <int NFP, int NPOPS>
__global__ __launch_bounds__(64) void k_wd_moments(DevPack pk, DevStars st, const IsoHdr *__restrict__ hdr, const double *__restrict__ params,
                                                   int n_nodes, const double *__restrict__ tab, int n_wp, const int *__restrict__ wd_rank,
                                                   double *__restrict__ scratch)
{
    __shared__ __attribute__((aligned(16))) double s_rows[2 * B9_WDS_TYPE_STRIDE(NFP)];
    __shared__ double s_lpm[B9_WDS_TILE], s_der[B9_WDS_TILE * B9_WDS_DER], s_stat[B9_WDS_TILE];
    const int lane = threadIdx.x, r = blockIdx.y;
    const int k_wd = blockIdx.x * 64 + lane;
    const bool live = k_wd < st.n_wd;
    const WdStar<NFP> star = wd_star<NFP, NPOPS>(st, hdr, params, live ? k_wd : 0, r);
    const int slot = star.slot;
    double *__restrict__ const out = scratch + ((size_t)r * st.n_wd + wd_rank[star.orig]) * B9_WDM_N;
    if (!star.valid) {                                       // a row outside the grid contributes nothing
        if (live) {
#pragma unroll
            for (int c = 0; c < B9_WDM_N; ++c) out[c] = 0.0;
        }
        return;
    }
    const double *par = star.par;
    const WdTable<const double> t = wd_table_view(tab, NFP, n_wp, n_nodes);
    const double *__restrict__ const stat_all = t.der + (size_t)n_wp * n_nodes * B9_WDS_DER;
    double lg[NPOPS], mean[NPOPS][B9_WDM_SUMS - 1];
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        double ref = NEG_INF, s[B9_WDM_SUMS];
#pragma unroll
        for (int c = 0; c < B9_WDM_SUMS; ++c) s[c] = 0.0;
        const int wp = r * NPOPS + kp;
        const double tip = hdr[wp].agb_tip;
        const double dM = (pk.m_wd_up - tip) / n_nodes;
        if (dM > 0.0) {                                      // (wave-uniform: one row)
            const double log_w = log(dM);
            const double *__restrict__ const lpm = t.lpm + (size_t)wp * n_nodes;
            const double *__restrict__ const der = t.der + (size_t)wp * n_nodes * B9_WDS_DER;
            const double *__restrict__ const stat = stat_all + (size_t)wp * n_nodes;
            for (int t0 = 0; t0 < n_nodes; t0 += B9_WDS_TILE) {
                const int cnt = n_nodes - t0 < B9_WDS_TILE ? n_nodes - t0 : B9_WDS_TILE;
                __syncthreads();                             // (the previous tile's reads are done)
#pragma unroll
                for (int ty = 0; ty < 2; ++ty) {
                    const double *__restrict__ const src = t.rows + (((size_t)wp * 2 + ty) * n_nodes + t0) * NFP;
                    for (int x = lane; x < cnt * NFP; x += 64) s_rows[ty * B9_WDS_TYPE_STRIDE(NFP) + x] = src[x];
                }
                for (int x = lane; x < cnt * B9_WDS_DER; x += 64) s_der[x] = der[(size_t)t0 * B9_WDS_DER + x];
                if (lane < cnt) { s_lpm[lane] = lpm[t0 + lane]; s_stat[lane] = stat[t0 + lane]; }
                __syncthreads();
                const double *const mine = s_rows + star.wd_type * B9_WDS_TYPE_STRIDE(NFP);
                for (int i = 0; i < cnt; ++i) {
                    const double *const row = mine + i * NFP;
                    double chi2 = 0.0;
#pragma unroll
                    for (int f = 0; f < NFP; ++f) { const double d = row[f] - star.obs[f]; chi2 = fma(star.wgt[f] * d, d, chi2); }
                    if (live && isfinite(chi2)) {
                        const double term = (s_lpm[i] - 0.5 * chi2) + log_w;
                        const double e = lse_step(term, ref, [&](double scale) {
#pragma unroll
                            for (int c = 0; c < B9_WDM_SUMS; ++c) s[c] *= scale;
                        });
                        const double m = tip + dM * (double)(t0 + i + 1), em = e * m;
                        const bool cooled = s_stat[i] == 2.0;
                        const double ec = cooled ? e : 0.0;
                        s[0] += e; s[1] += em; s[2] = fma(em, m, s[2]); s[3] += ec;
#pragma unroll
                        for (int q = 0; q < B9_WDS_DER; ++q) {
                            const double v = cooled ? s_der[i * B9_WDS_DER + q] : 0.0, ev = ec * v;
                            s[4 + 2 * q] += ev; s[5 + 2 * q] = fma(ev, v, s[5 + 2 * q]);
                        }
                    }
                }
            }
        }
        const bool has = ref != NEG_INF;
        lg[kp] = has ? ref + log(s[0]) : NEG_INF;
#pragma unroll
        for (int c = 0; c < B9_WDM_SUMS - 1; ++c) mean[kp][c] = has ? s[1 + c] / s[0] : 0.0;
    }
    if (!live) return;
    // the star finished: membership and the populations' weights, the sixteen increments
    double x[B9_WDM_N];
#pragma unroll
    for (int c = 0; c < B9_WDM_N; ++c) x[c] = 0.0;
    double p, wk[NPOPS];
    if (star_finish<NPOPS>(lg, st.c0m[slot], st.la[slot], par, p, wk)) {
        double m[B9_WDM_SUMS - 1];
#pragma unroll
        for (int c = 0; c < B9_WDM_SUMS - 1; ++c) {
            m[c] = 0.0;
#pragma unroll
            for (int k = 0; k < NPOPS; ++k) m[c] += wk[k] * mean[k][c];
        }
        x[B9_WDM_ROWS] = 1.0; x[B9_WDM_MEMBER] = p;
        x[B9_WDM_POP1] = NPOPS == 2 ? p * wk[NPOPS - 1] : 0.0;
        x[B9_WDM_COOLED] = p * m[2]; x[B9_WDM_M1] = p * m[0]; x[B9_WDM_M1SQ] = p * m[1];
#pragma unroll
        for (int c = 0; c < 2 * B9_WDS_DER; ++c) x[B9_WDM_WDMASS + c] = p * m[3 + c];
    }
#pragma unroll
    for (int c = 0; c < B9_WDM_N; ++c) out[c] = x[c];
}
