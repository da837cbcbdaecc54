// b9_ratio_hist.hip.h -- b9_ratio_hist (the binaryStats counterpart): k_star_ratio (MS/RGB-stage stars, one LANE per star) and
// k_star_ratio_wd (WD-stage stars, one WAVE per star).  The rows' sums over the stars are k_hist_rows', the accumulation
// k_chain_accumulate's.  Part of the single translation unit b9_kernels.hip (included there, after b9_mass_hist.hip.h); gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------
// Exact mass-ratio posteriors by primary mass over a chain ("Mass-ratio posteriors by primary mass").  The
// grid, the node terms, the weights w, the membership p and the pruning are b9_mass_hist's; where that call bins one value of a
// node, these kernels keep the JOINT table of the node's primary-mass bin b (n_mbins bins [e_b, e_b+1) of M1) and its ratio node
// j of Q: x[b Q + j] = p sum_{nodes of ratio j with M1 in bin b} w, and the total column x[n_mbins Q] = p.  They go per (row, star)
// to a scratch [row][star][n_mbins Q + 1] in the caller's star order.  No random numbers, no atomics.
//
// k_star_ratio: k_star_hist's frame -- grid (64-star chunk of the mg_* copy, row, column tile) x 256, the seeds, walk_nodes, the
// wave-uniform mass bin cached in scalar registers with its two edges, one LDS histogram [columns of the tile][64] per wave (a
// bank per lane pair), the four waves merged in wave order by wave 0, divided by the merged S0, the populations mixed with
// star_finish's weights, times p.  The column of a node inside its tile is (b - m0) Q + j: both parts are wave-uniform (j is the
// unit's, a function of the wave).  A tile holds WHOLE mass bins, mpt = max(1, floor(B9_HIST_TILE / Q)) of them, so its columns
// are contiguous in the output ([m0 Q, (m0 + tm) Q)) and number at most B9_HIST_TILE for Q <= B9_HIST_TILE, Q above that.  The
// reference's evolution and the pruning depend on the terms only: a cell's bits are the same in any tile and among any other bins.
// ------------------------------------------------------------------------------------------
template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_ratio(DevStars st, const IsoHdr *__restrict__ hdr, const double *__restrict__ iso_data,
                                                    long long iso_stride, int mass_cap, const double *__restrict__ params, int K, int Q,
                                                    const double *__restrict__ tab, MargLayout L, double cut2, HistEdges ed, int mpt, int tc_cap,
                                                    double *__restrict__ scratch)
{
    // all LDS is dynamic (the opt-in above 64 KB counts it whole): [seeds][states][histograms]
    extern __shared__ __attribute__((aligned(16))) double s_lds[];
    double (*const s_seed)[4][64] = reinterpret_cast<double (*)[4][64]>(s_lds);                       // [NPOPS][wave][lane]
    double (*const s_state)[2][64] = reinterpret_cast<double (*)[2][64]>(s_lds + NPOPS * 4 * 64);     // [wave]{reference, S0}[lane]
    double *const s_hist = s_lds + (NPOPS * 4 + 4 * 2) * 64;                                           // [wave][column of the tile][64]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sc = blockIdx.x, w = blockIdx.y, m0 = blockIdx.z * mpt;                        // m0: the tile's first mass bin
    const int n_mbins = ed.n_bins, n_cells = n_mbins * Q, ncol = n_cells + 1;
    const int tm = min(n_mbins - m0, mpt), c0 = m0 * Q, tc = tm * Q;                         // (host: tc <= tc_cap, the LDS's columns)
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
    if (!valid || tc > tc_cap) {                         // a row outside the grid contributes nothing
        if (wave == 0 && !dead) {
            for (int c = 0; c < tc; ++c) out[c0 + c] = 0.0;
            if (m0 == 0) out[n_cells] = 0.0;
        }
        return;
    }
    double *const h_mine = s_hist + (size_t)wave * tc * 64 + lane;

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
        for (int c = 0; c < tc; ++c) h_mine[c * 64] = 0.0;
        // the mass bin the last node fell in, wave-uniform: c_lo <= M1 < c_hi keeps it (an empty interval to start with)
        double c_lo = __builtin_inf(), c_hi = NEG_INF;
        int c_b = -1;
        walk_nodes<NFP>(t_wp, L, (iso[kp].n - 1) * K, Q, wave, dead, cut2, tmax, so, sw, [&](bool live, double x, int node, int j, b9_ctab) {
            const double v = uniform_f64(hist_value(B9_HQ_PRIMARY, marg_primary(iso[kp].mass, node, (iso[kp].n - 1) * K, K, 0).m1, j, Q));
            if (!(v >= c_lo && v < c_hi)) {
                c_b = hist_bin(ed, v);
                c_lo = c_b >= 0 ? ed.e[c_b] : NEG_INF;
                c_hi = c_b < n_mbins ? ed.e[c_b + 1] : __builtin_inf();
            }
            const int hc = (c_b >= m0 && c_b < m0 + tm) ? (c_b - m0) * Q + j : -1;
            if (live) hist_term(-0.5 * x, hc, tc, ref, s0, h_mine);
        });
        s_state[wave][0][lane] = ref;
        s_state[wave][1][lane] = s0;
        __syncthreads();

        // ---- wave 0: the four shares merged in wave order.  A population before the last parks its normalised columns in the
        // output (a lane reads back only what it wrote itself); the last one mixes them with star_finish's weights
        if (wave == 0 && !dead) {
            const WaveMerge mg = wave_merge(s_state, lane);
            lg[kp] = (mg.S0 > 0.0) ? mg.r + log(mg.S0) : NEG_INF;
            double p = 0.0, wk[NPOPS];
            bool any = false;
            if (kp == NPOPS - 1) any = star_finish<NPOPS>(lg, st.mg_c0m[slot], st.mg_la[slot], par, p, wk);
            for (int c = 0; c < tc; ++c) {
                const double hn = (mg.S0 > 0.0) ? wave_sum(mg, s_hist + (size_t)c * 64 + lane, (size_t)tc * 64) / mg.S0 : 0.0;
                if (kp < NPOPS - 1) { out[c0 + c] = hn; continue; }
                double m = wk[NPOPS - 1] * hn;
                if (NPOPS == 2) m = wk[0] * out[c0 + c] + m;
                out[c0 + c] = any ? p * m : 0.0;
            }
            if (kp == NPOPS - 1 && m0 == 0) out[n_cells] = any ? p : 0.0;
        }
        if (kp + 1 < NPOPS) __syncthreads();             // the histograms are cleared for the next population
    }
}

// ------------------------------------------------------------------------------------------
// k_star_ratio_wd: the WD-stage stars (b9_chain_walk.hip.h), k_star_hist_wd with lane b owning MASS bin b (n_mbins <= 16 lanes
// of the wave): every step's w = exp(t - L) goes to the lane that owns the bin of its M1 = tip + dM j, in ascending step order.  A
// WD-stage star has mass ratio 0 only: lane b's value is column b Q, and the line's other n_mbins (Q - 1) columns are written 0.
// ------------------------------------------------------------------------------------------
template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_ratio_wd(DevStars st, double m_wd_up, const IsoHdr *__restrict__ hdr, const double *__restrict__ params,
                                                       int K, int Q, const double *__restrict__ wtab, HistEdges ed, double *__restrict__ scratch)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k_wd = blockIdx.x * 4 + wave, w = blockIdx.y, n_wp = gridDim.y * NPOPS;
    const int n_mbins = ed.n_bins, n_cells = n_mbins * Q, ncol = n_cells + 1;
    if (k_wd >= st.n_wd) return;
    const WdStar<NFP> ws = wd_star<NFP, NPOPS>(st, hdr, params, k_wd, w);
    double *__restrict__ const out = scratch + ((size_t)w * st.n + ws.orig) * ncol;
    if (!ws.valid) {
        for (int c = lane; c < ncol; c += 64) out[c] = 0.0;
        return;
    }
    double lg[NPOPS], hk[NPOPS];                         // hk: the lane's mass bin under population k, normalised
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
        if (has) {
            for (int jb = 0; jb < sp.steps; jb += 64) {
                const int j = jb + 1 + lane;
                const double t = sp.term(ws, j);
                const double wj = t == NEG_INF ? 0.0 : exp(t - Lk);
                const int bj = t == NEG_INF ? -1 : hist_bin(ed, sp.m1(j));
                for (int l = 0; l < 64; ++l) {
                    const double wl = __shfl(wj, l, 64);
                    const int bl = __shfl(bj, l, 64);
                    if (bl == lane) h = h + wl;
                }
            }
        }
        hk[kp] = h;
    }
    double p, wk[NPOPS];
    const bool any = star_finish<NPOPS>(lg, st.c0m[ws.slot], st.la[ws.slot], ws.par, p, wk);
    double m = wk[0] * hk[0];
    if (NPOPS == 2) m = m + wk[NPOPS - 1] * hk[NPOPS - 1];
    const double mine = any ? p * m : 0.0;               // lane b < n_mbins: column b Q
    for (int cb = 0; cb < n_cells; cb += 64) {           // every column of the line: lane b's value at b Q, zeros between
        const int c = cb + lane, b = c / Q;
        const double v = __shfl(mine, min(b, 63), 64);
        if (c < n_cells) out[c] = (c - b * Q == 0) ? v : 0.0;
    }
    if (lane == 0) out[n_cells] = any ? p : 0.0;
}
