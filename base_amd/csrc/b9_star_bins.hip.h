// b9_star_bins.hip.h -- b9_star_bins (the starIntervals counterpart): k_star_bins (MS/RGB-stage stars, one LANE per star) and
// k_star_bins_wd (WD-stage stars, one WAVE per star).  Part of the single translation unit b9_kernels.hip (included there,
// after b9_mass_hist.hip.h); gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------
// Per-star bins over a chain ("Per-star bins and credible intervals").  Everything but the edges is
// b9_mass_hist's: the grid, the terms, the weights, the membership, the pruning and the node value (hist_value), the online
// log-sum-exp with its bins (hist_term), the merge and the finish.  Star i has its OWN edges e_i0 < ... < e_iB, and the two open
// ends are bins like the others: column 0 holds the nodes below e_i0, column 1 + b bin b, column B + 1 the nodes at or above
// e_iB, column B + 2 the total p.  Increments go per (row, star) to a scratch [row][star][B + 3] in the caller's star order and
// k_chain_accumulate adds the rows.
//
// k_star_bins: grid (64-star chunk of the mg_* copy, row) x 256.  A node's value is wave-uniform as in k_star_hist, its bin is
// not: every lane keeps its current bin and that bin's two edges in registers and searches its own column of the edges, staged
// once per workgroup in LDS as [edge][64] (the lane is the bank: conflict-free for any per-lane index), only when a value leaves
// them.  A wave's histogram is [B + 2][64] in LDS, again a bank per lane.  With B <= B9_SBIN_MAX_BINS = 30 that is one tile of
// at most 32 columns: no tiling over blockIdx.z.  With every star on the same edges, columns 1 .. B take exactly the adds that
// k_star_hist's bins take, in the same order: the same bits.
// ------------------------------------------------------------------------------------------

// the number of the lane's edges <= v, less one (-1: below e_0; n_bins: at or above the last edge); e: the lane's column, stride 64
__device__ __forceinline__ int sbin_search(const double *e, int n_bins, double v)
{
    int lo = 0, hi = n_bins + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid * 64] <= v) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_bins(DevStars st, const IsoHdr *__restrict__ hdr, const double *__restrict__ iso_data,
                                                   long long iso_stride, int mass_cap, const double *__restrict__ params, int K, int Q,
                                                   const double *__restrict__ tab, MargLayout L, double cut2, const double *__restrict__ edges,
                                                   int n_bins, int quantity, double *__restrict__ scratch)
{
    // all LDS is dynamic (the opt-in above 64 KB counts it whole): [seeds][states][edges][histograms]
    extern __shared__ __attribute__((aligned(16))) double s_lds[];
    double (*const s_seed)[4][64] = reinterpret_cast<double (*)[4][64]>(s_lds);                       // [NPOPS][wave][lane]
    double (*const s_state)[2][64] = reinterpret_cast<double (*)[2][64]>(s_lds + NPOPS * 4 * 64);     // [wave]{reference, S0}[lane]
    double *const s_edge = s_lds + (NPOPS * 4 + 4 * 2) * 64;                                           // [edge][lane]
    double *const s_hist = s_edge + (size_t)(n_bins + 1) * 64;                                         // [wave][column < n_bins + 2][64]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sc = blockIdx.x, w = blockIdx.y;
    const int tb = n_bins + 2, ncol = n_bins + 3;
    const int slot = sc * 64 + lane, orig = st.mg_perm[slot];
    const bool dead = orig < 0;
    double so[NFP], sw[NFP];
#pragma unroll
    for (int f = 0; f < NFP; ++f) { so[f] = st.mg_so[B9_SIDX(NFP, f, slot)]; sw[f] = st.mg_sw[B9_SIDX(NFP, f, slot)]; }
    const double *par = params + (size_t)w * B9_NPARAM;
    double *const out = scratch + ((size_t)w * st.n + (dead ? 0 : orig)) * ncol;
    IsoView<NFP> iso[NPOPS];
    double tip_min;
    const bool valid = load_iso_views<NFP, NPOPS>(hdr, iso_data, iso_stride, mass_cap, w, iso, tip_min);
    if (!valid) {                                        // a row outside the grid contributes nothing
        if (wave == 0 && !dead)
            for (int c = 0; c < ncol; ++c) out[c] = 0.0;
        return;
    }
    // the 64 stars' edges, gathered through mg_perm from the caller's order (a padding lane: zeros, never counted)
    for (int i = threadIdx.x; i < (n_bins + 1) * 64; i += 256) {
        const int o = st.mg_perm[sc * 64 + (i & 63)];
        s_edge[i] = o < 0 ? 0.0 : edges[(size_t)o * (n_bins + 1) + (i >> 6)];
    }
    double *const h_mine = s_hist + (size_t)wave * tb * 64 + lane;
    const double *const e_mine = s_edge + lane;

#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp)
        s_seed[kp][wave][lane] = walk_seed<NFP>((b9_ctab)(tab + (size_t)(w * NPOPS + kp) * L.total), L, (iso[kp].n - 1) * K, Q, wave, so, sw);
    __syncthreads();

    double lg[NPOPS];
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        const b9_ctab t_wp = (b9_ctab)(tab + (size_t)(w * NPOPS + kp) * L.total);
        double tmax = walk_start(s_seed[kp], lane);
        double ref = tmax, s0 = 0.0;
        for (int b = 0; b < tb; ++b) h_mine[b * 64] = 0.0;
        // the bin the lane's last node fell in: c_lo <= v < c_hi keeps it (an empty interval to start with)
        double c_lo = __builtin_inf(), c_hi = NEG_INF;
        int c_b = -1;
        walk_nodes<NFP>(t_wp, L, (iso[kp].n - 1) * K, Q, wave, dead, cut2, tmax, so, sw, [&](bool live, double x, int node, int j, b9_ctab) {
            const double v = uniform_f64(hist_value(quantity, marg_primary(iso[kp].mass, node, (iso[kp].n - 1) * K, K, 0).m1, j, Q));
            if (!(v >= c_lo && v < c_hi)) {
                c_b = sbin_search(e_mine, n_bins, v);
                c_lo = c_b >= 0 ? e_mine[c_b * 64] : NEG_INF;
                c_hi = c_b < n_bins ? e_mine[(c_b + 1) * 64] : __builtin_inf();
            }
            const bool counts = quantity != B9_HQ_SECONDARY || j > 0;
            if (live) hist_term(-0.5 * x, counts ? c_b + 1 : -1, tb, ref, s0, h_mine);
        });
        s_state[wave][0][lane] = ref;
        s_state[wave][1][lane] = s0;
        __syncthreads();

        // ---- wave 0: the four shares merged in wave order, as k_star_hist does
        if (wave == 0 && !dead) {
            const WaveMerge mg = wave_merge(s_state, lane);
            lg[kp] = (mg.S0 > 0.0) ? mg.r + log(mg.S0) : NEG_INF;
            double p = 0.0, wk[NPOPS];
            bool any = false;
            if (kp == NPOPS - 1) any = star_finish<NPOPS>(lg, st.mg_c0m[slot], st.mg_la[slot], par, p, wk);
            for (int b = 0; b < tb; ++b) {
                const double hn = (mg.S0 > 0.0) ? wave_sum(mg, s_hist + (size_t)b * 64 + lane, (size_t)tb * 64) / mg.S0 : 0.0;
                if (kp < NPOPS - 1) { out[b] = hn; continue; }
                double m = wk[NPOPS - 1] * hn;
                if (NPOPS == 2) m = wk[0] * out[b] + m;
                out[b] = any ? p * m : 0.0;
            }
            if (kp == NPOPS - 1) out[tb] = any ? p : 0.0;
        }
        if (kp + 1 < NPOPS) __syncthreads();             // the histograms are cleared for the next population
    }
}

// ------------------------------------------------------------------------------------------
// k_star_bins_wd: the WD-stage stars, k_star_hist_wd's frame and ordered read-out.  The star's edges are wave-uniform (read from
// the caller's order); lane c owns column c: 0 below, 1 + b bin b, n_bins + 1 at or above.  B9_HQ_SECONDARY: no node counts,
// the total still does.
// ------------------------------------------------------------------------------------------
template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_bins_wd(DevStars st, double m_wd_up, const IsoHdr *__restrict__ hdr, const double *__restrict__ params,
                                                      int K, const double *__restrict__ wtab, const double *__restrict__ edges, int n_bins, int quantity,
                                                      double *__restrict__ scratch)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k_wd = blockIdx.x * 4 + wave, w = blockIdx.y, n_wp = gridDim.y * NPOPS;
    const int tb = n_bins + 2, ncol = n_bins + 3;
    if (k_wd >= st.n_wd) return;
    const WdStar<NFP> ws = wd_star<NFP, NPOPS>(st, hdr, params, k_wd, w);
    double *__restrict__ const out = scratch + ((size_t)w * st.n + ws.orig) * ncol;
    if (!ws.valid) {
        for (int c = lane; c < ncol; c += 64) out[c] = 0.0;
        return;
    }
    const double *__restrict__ const e = edges + (size_t)ws.orig * (n_bins + 1);
    double lg[NPOPS], hk[NPOPS];                         // hk: the lane's column under population k, normalised
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        const WdSteps<NFP> sp = wd_steps<NFP>(ws, m_wd_up, hdr, K, wtab, w * NPOPS + kp, n_wp);
        Lse acc; acc.mx = NEG_INF; acc.sm = 0.0;
        for (int j = 1 + lane; j <= sp.steps; j += 64) lse_add(acc, sp.term(ws, j));
        acc = lse_wave(acc);
        acc.mx = __shfl(acc.mx, 0, 64); acc.sm = __shfl(acc.sm, 0, 64);
        const bool has = acc.mx != NEG_INF;
        const double Lk = has ? acc.mx + log(acc.sm) : NEG_INF;
        lg[kp] = Lk;
        double h = 0.0;
        if (has && quantity != B9_HQ_SECONDARY) {
            for (int jb = 0; jb < sp.steps; jb += 64) {
                const int j = jb + 1 + lane;
                const double t = sp.term(ws, j);
                const double wj = t == NEG_INF ? 0.0 : exp(t - Lk);
                int cj = -1;                             // the step's column
                if (t != NEG_INF) {
                    const double v = sp.m1(j);
                    int lo = 0, hi = n_bins + 1;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (e[mid] <= v) lo = mid + 1; else hi = mid;
                    }
                    cj = lo;
                }
                for (int l = 0; l < 64; ++l) {
                    const double wl = __shfl(wj, l, 64);
                    const int cl = __shfl(cj, l, 64);
                    if (cl == lane) h = h + wl;
                }
            }
        }
        hk[kp] = h;
    }
    double p, wk[NPOPS];
    const bool any = star_finish<NPOPS>(lg, st.c0m[ws.slot], st.la[ws.slot], ws.par, p, wk);
    double m = wk[0] * hk[0];
    if (NPOPS == 2) m = m + wk[NPOPS - 1] * hk[NPOPS - 1];
    if (lane < tb) out[lane] = any ? p * m : 0.0;
    if (lane == 0) out[tb] = any ? p : 0.0;
}
