// b9_mass_hist.hip.h -- b9_mass_hist (the massFunction counterpart): k_star_hist (MS/RGB-stage stars, one LANE per star),
// k_star_hist_wd (WD-stage stars, one WAVE per star) and k_hist_rows (a row's sum over the stars).  Part of the single
// translation unit b9_kernels.hip (included there, after b9_star_moments.hip.h); gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------
// Exact binned mass posteriors over a chain ("Binned mass posteriors").  The grid, the node terms t_(k, n),
// the weights w = exp(t - logsumexp t) and the membership p are b9_star_moments'; where that call keeps five weighted sums, these
// kernels keep, for n_bins bins [e_b, e_b+1) of the node value v (primary mass M1, secondary mass (j / Q) M1 of the nodes with
// j > 0, or the system's M1 + m2), x[b] = p sum_{v in bin b} w and the total column x[n_bins] = p.  They go per (row, star) to
// a scratch [row][star][n_bins + 1] in the caller's star order; k_chain_accumulate adds the rows to the per-star accumulators
// in ascending row order and k_hist_rows sums a row over the stars in ascending star order, one plain add each: the same bits
// for any chunking.  No random numbers, no atomics.
//
// k_star_hist: grid (64-star chunk of the mg_* copy, row, bin tile) x 256, the walk and the pruning of b9_chain_walk.hip.h
// (walk_nodes calls back for all 64 lanes of a wave that has a live node: the bin search is wave-uniform).  A node's value and
// therefore its bin are wave-uniform: the bin is kept in scalar registers with its two edges, and searched again (a binary
// search over the edges in the kernel's arguments) only when a node's value leaves it.  A lane's accumulators live in LDS, one
// histogram [bins of the tile][64] per wave (a bank per lane pair: conflict-free), S0 and the reference in registers.  The
// online log-sum-exp is lse_step's; its rare rescale walks the wave's LDS bins.  Per population the four waves' histograms are merged in wave order 0..3 by wave 0 and divided by the
// merged S0; the populations are mixed with star_finish's weights and multiplied by p.  A tile holds at most
// B9_HIST_TILE bins (64 KB of LDS); the reference's evolution and the pruning depend on the terms only, never on the bins,
// so a bin's bits are the same in any tile and among any other bins.
// ------------------------------------------------------------------------------------------
#define B9_HIST_TILE 32

struct HistEdges { double e[B9_HIST_MAX_BINS + 1]; int n_bins, quantity; };

// the value of node (m1, j of Q): every product and sum rounded on its own (the table builder's m2; no fma)
__device__ __forceinline__ double hist_value(int quantity, double m1, int j, int Q)
{
#pragma clang fp contract(off)
    const double m2 = ((double)j / (double)Q) * m1;
    return quantity == B9_HQ_PRIMARY ? m1 : quantity == B9_HQ_SECONDARY ? m2 : m1 + m2;
}

// the number of edges <= v, less one: the bin of v (-1: below e_0; n_bins: at or above the last edge)
__device__ __forceinline__ int hist_bin(const HistEdges &ed, double v)
{
    int lo = 0, hi = ed.n_bins + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ed.e[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

__device__ __forceinline__ double uniform_f64(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// one more term t = -X / 2 whose node falls in bin `hb` of the wave's tile (hb < 0: in none of them).
// h: the lane's column of the wave's LDS histogram, [tb][64].
__device__ __forceinline__ void hist_term(double t, int hb, int tb, double &ref, double &s0, double *h)
{
    const double e = lse_step(t, ref, [&](double scale) {
        s0 *= scale;
        for (int b = 0; b < tb; ++b) h[b * 64] *= scale;
    });
    s0 += e;
    if (hb >= 0) h[hb * 64] += e;
}

template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_hist(DevStars st, const IsoHdr *__restrict__ hdr, const double *__restrict__ iso_data,
                                                   long long iso_stride, int mass_cap, const double *__restrict__ params, int K, int Q,
                                                   const double *__restrict__ tab, MargLayout L, double cut2, HistEdges ed, int tb_cap,
                                                   double *__restrict__ scratch)
{
    // all LDS is dynamic (the opt-in above 64 KB counts it whole): [seeds][states][histograms]
    extern __shared__ __attribute__((aligned(16))) double s_lds[];
    double (*const s_seed)[4][64] = reinterpret_cast<double (*)[4][64]>(s_lds);                       // [NPOPS][wave][lane]
    double (*const s_state)[2][64] = reinterpret_cast<double (*)[2][64]>(s_lds + NPOPS * 4 * 64);     // [wave]{reference, S0}[lane]
    double *const s_hist = s_lds + (NPOPS * 4 + 4 * 2) * 64;                                           // [wave][bin of the tile][64]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sc = blockIdx.x, w = blockIdx.y, b0 = blockIdx.z * B9_HIST_TILE;
    const int n_bins = ed.n_bins, ncol = n_bins + 1, tb = min(n_bins - b0, B9_HIST_TILE);   // (host: tb <= tb_cap, the LDS's bins)
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
    if (!valid || tb > tb_cap) {                         // a row outside the grid contributes nothing
        if (wave == 0 && !dead) {
            for (int b = 0; b < tb; ++b) out[b0 + b] = 0.0;
            if (b0 == 0) out[n_bins] = 0.0;
        }
        return;
    }
    double *const h_mine = s_hist + (size_t)wave * tb * 64 + lane;

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
        // the bin the last node fell in, wave-uniform: c_lo <= v < c_hi keeps it (an empty interval to start with)
        double c_lo = __builtin_inf(), c_hi = NEG_INF;
        int c_b = -1;
        walk_nodes<NFP>(t_wp, L, (iso[kp].n - 1) * K, Q, wave, dead, cut2, tmax, so, sw, [&](bool live, double x, int node, int j, b9_ctab) {
            const double v = uniform_f64(hist_value(ed.quantity, marg_primary(iso[kp].mass, node, (iso[kp].n - 1) * K, K, 0).m1, j, Q));
            if (!(v >= c_lo && v < c_hi)) {
                c_b = hist_bin(ed, v);
                c_lo = c_b >= 0 ? ed.e[c_b] : NEG_INF;
                c_hi = c_b < n_bins ? ed.e[c_b + 1] : __builtin_inf();
            }
            const bool counts = ed.quantity != B9_HQ_SECONDARY || j > 0;
            const int hb = (counts && c_b >= b0 && c_b < b0 + tb) ? c_b - b0 : -1;
            if (live) hist_term(-0.5 * x, hb, tb, ref, s0, h_mine);
        });
        s_state[wave][0][lane] = ref;
        s_state[wave][1][lane] = s0;
        __syncthreads();

        // ---- wave 0: the four shares merged in wave order.  A population before the last parks its normalised bins in the
        // output (a lane reads back only what it wrote itself); the last one mixes them with star_finish's weights
        if (wave == 0 && !dead) {
            const WaveMerge mg = wave_merge(s_state, lane);
            lg[kp] = (mg.S0 > 0.0) ? mg.r + log(mg.S0) : NEG_INF;
            double p = 0.0, wk[NPOPS];
            bool any = false;
            if (kp == NPOPS - 1) any = star_finish<NPOPS>(lg, st.mg_c0m[slot], st.mg_la[slot], par, p, wk);
            for (int b = 0; b < tb; ++b) {
                const double hn = (mg.S0 > 0.0) ? wave_sum(mg, s_hist + (size_t)b * 64 + lane, (size_t)tb * 64) / mg.S0 : 0.0;
                if (kp < NPOPS - 1) { out[b0 + b] = hn; continue; }
                double m = wk[NPOPS - 1] * hn;
                if (NPOPS == 2) m = wk[0] * out[b0 + b] + m;
                out[b0 + b] = any ? p * m : 0.0;
            }
            if (kp == NPOPS - 1 && b0 == 0) out[n_bins] = any ? p : 0.0;
        }
        if (kp + 1 < NPOPS) __syncthreads();             // the histograms are cleared for the next population
    }
}

// ------------------------------------------------------------------------------------------
// k_star_hist_wd: the WD-stage stars (b9_chain_walk.hip.h).  Here the bin is per lane.  Per population: L first (an online
// log-sum-exp per lane, merged by the wave's shuffle tree and broadcast), then every step's w = exp(t - L) goes to the lane that
// owns its bin -- lane b holds bin b -- in ascending step order: a block of 64 steps at a time, the block's lanes read out one
// after the other.  The order depends on the layout only.  B9_HQ_SECONDARY: no node counts, the total still does.
// ------------------------------------------------------------------------------------------
template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_hist_wd(DevStars st, double m_wd_up, const IsoHdr *__restrict__ hdr, const double *__restrict__ params,
                                                      int K, const double *__restrict__ wtab, HistEdges ed, double *__restrict__ scratch)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k_wd = blockIdx.x * 4 + wave, w = blockIdx.y, n_wp = gridDim.y * NPOPS;
    const int n_bins = ed.n_bins, ncol = n_bins + 1;
    if (k_wd >= st.n_wd) return;
    const WdStar<NFP> ws = wd_star<NFP, NPOPS>(st, hdr, params, k_wd, w);
    double *__restrict__ const out = scratch + ((size_t)w * st.n + ws.orig) * ncol;
    if (!ws.valid) {
        for (int c = lane; c < ncol; c += 64) out[c] = 0.0;
        return;
    }
    double lg[NPOPS], hk[NPOPS];                         // hk: the lane's bin under population k, normalised
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
        if (has && ed.quantity != B9_HQ_SECONDARY) {
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
    if (lane < n_bins) out[lane] = any ? p * m : 0.0;
    if (lane == 0) out[n_bins] = any ? p : 0.0;
}

// k_hist_rows: one lane per (row, column): the row's increments summed over the stars in ascending (the caller's) order, one plain
// add each.  Neighbouring lanes read neighbouring columns of the same star.  A chunk has few lanes (rows x columns) and each
// walks every star, so the walk is bound by the loads' latency: B9_HIST_ROWS_AHEAD independent loads are in flight per lane
// before the adds that consume them, which stay in star order.
#define B9_HIST_ROWS_AHEAD 64
__global__ __launch_bounds__(256) void k_hist_rows(const double *__restrict__ scratch, int n_rows, int n_stars, int ncol, double *__restrict__ rows)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows * ncol) return;
    const int r = i / ncol, c = i - r * ncol;
    const double *__restrict__ const x = scratch + (size_t)r * n_stars * ncol + c;
    double a = 0.0;
    int s = 0;
    for (; s + B9_HIST_ROWS_AHEAD <= n_stars; s += B9_HIST_ROWS_AHEAD) {
        double v[B9_HIST_ROWS_AHEAD];
#pragma unroll
        for (int k = 0; k < B9_HIST_ROWS_AHEAD; ++k) v[k] = x[(size_t)(s + k) * ncol];
#pragma unroll
        for (int k = 0; k < B9_HIST_ROWS_AHEAD; ++k) a = a + v[k];
    }
    for (; s < n_stars; ++s) a = a + x[(size_t)s * ncol];
    rows[i] = a;
}
