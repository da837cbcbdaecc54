// b9_wd_sample.hip.h -- b9_sample_wd_mass (the sampleWDMass counterpart): k_wd_node_table (the WD chain once per node, derived
// values kept), wd_grid_walk (the frame of the three star kernels against that table: k_wd_sample, k_wd_moments, k_wd_bins) and
// k_wd_sample (one LANE per WD-stage star: Gumbel-max draw, membership, derived values).
// Part of the single translation unit b9_kernels.hip (included there, after b9_chain_walk.hip.h); gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------
// The grid is the call's own (n_nodes equal steps in (AGB tip, M_wd_up] per population; include/base9_hip.h, DESIGN.md
// section 2).  As in k_marg_wd_table, nothing about a node depends on the star: the WD chain runs once per (row, population,
// DA / DB, node) and the stars scan the table.  One chunk of rows' table, wp = row * n_pops + population:
//   rows [wp][type][n_nodes][NFP]   apparent magnitudes of node j = 1 .. n_nodes (modulus and absorption added)
//   lpm  [wp][n_nodes]              log mass prior of the node
//   der  [wp][n_nodes][5]           wd_mass, precursor log-age, log cooling age, log Teff, log g: what the row's magnitudes
//                                   were computed FROM (wd_chain's values, not a second evaluation)
// and, in the table b9_wd_moments builds (k_wd_node_table_status: the same body with STATUS), behind them
//   stat [wp][n_nodes]              wd_chain's status of the node, as a double (b9_wd_moments.hip.h)
// ------------------------------------------------------------------------------------------
#define B9_WDS_DER 5
#define B9_WDS_NODE_DOUBLES(nfp) (2 * (nfp) + 1 + B9_WDS_DER)       // table doubles per (row, population, node)

template <class T> struct WdTable { T *rows, *lpm, *der; };       // T = double (the builder) or const double (the star kernel)
template <class T>
__host__ __device__ static inline WdTable<T> wd_table_view(T *tab, int nfp, long long n_wp, long long n_nodes)
{
    WdTable<T> t;
    t.rows = tab; t.lpm = tab + n_wp * 2 * n_nodes * nfp; t.der = t.lpm + n_wp * n_nodes;
    return t;
}

// one node of the table, by one lane of grid (ceil(n_nodes / 64), rows * pops) x 128 threads: lane = node, wave = DA / DB
template <int NFP, bool STATUS>
__device__ __forceinline__ void wd_node_table_body(const DevPack &pk, const IsoHdr *__restrict__ hdr, const double *__restrict__ iso_data,
                                                   long long iso_stride, int mass_cap, int n_pops, const double *__restrict__ params,
                                                   int n_nodes, double *__restrict__ tab, int n_wp)
{
    const int wp = blockIdx.y, w = wp / n_pops, type = threadIdx.x >> 6;
    const long long j = 1 + (long long)blockIdx.x * 64 + (threadIdx.x & 63);
    const IsoHdr h = hdr[wp];
    if (!h.valid) return;
    const double *par = params + (size_t)w * B9_NPARAM;
    const double dM = (pk.m_wd_up - h.agb_tip) / n_nodes;
    if (!(dM > 0.0) || j > n_nodes) return;
    const WdAxes ax = wd_axes_global(pk, h.i_feh, h.i_y);
    const double m1 = h.agb_tip + dM * (double)j, mod = par[B9_P_MOD], av = par[B9_P_ABS];
    const WdTable<double> t = wd_table_view(tab, NFP, n_wp, n_nodes);
    // star_mags' branches: rounding can put the last node a bit above M_wd_up (no flux, as everywhere in this code base) and,
    // for a step below the mass's spacing, a node on the tip itself (the isochrone's last point); neither has derived values
    WdChain c; c.status = 0; c.wd_mass = 0.0; c.prec = 0.0; c.log_cool = 0.0; c.log_teff = 0.0; c.logg = 0.0;
    const bool is_wd = m1 > h.agb_tip && m1 <= pk.m_wd_up;
    if (is_wd) c = wd_chain(pk, ax, h.t_feh, h.t_y, par, m1);
    double p[NFP];
    if (!is_wd && m1 <= h.agb_tip) {
        const double *g = iso_data + (size_t)wp * iso_stride;
        msrgb_mags<NFP>(iso_view_of<NFP>(h, g, g + mass_cap), m1, p);
    } else if (c.status == 2) {            // the atmosphere lookup wd_mags does, on the same wd_chain values
        wd_atmosphere<NFP>(pk, ax, c, type, p);
    } else {
        fill<NFP>(p, c.status == 1 ? -4.0 : B9_MAG_NOFLUX);
    }
    double *row = t.rows + (((size_t)wp * 2 + type) * n_nodes + (size_t)(j - 1)) * NFP;
#pragma unroll
    for (int f = 0; f < NFP; ++f) row[f] = p[f] + (mod + pk.abs_m1[f] * av);
    if (type == 0) {
        const size_t n = (size_t)wp * n_nodes + (size_t)(j - 1);
        t.lpm[n] = log_prior_mass_dev(pk.log_mass_norm, m1);
        double *d = t.der + n * B9_WDS_DER;
        d[0] = c.wd_mass; d[1] = c.prec; d[2] = c.log_cool; d[3] = c.log_teff; d[4] = c.logg;
        if (STATUS) t.der[(size_t)n_wp * n_nodes * B9_WDS_DER + n] = (double)c.status;
    }
}

template <int NFP>
__global__ __launch_bounds__(128) void k_wd_node_table(DevPack pk, const IsoHdr *__restrict__ hdr, const double *__restrict__ iso_data,
                                                       long long iso_stride, int mass_cap, int n_pops, const double *__restrict__ params,
                                                       int n_nodes, double *__restrict__ tab, int n_wp)
{
    wd_node_table_body<NFP, false>(pk, hdr, iso_data, iso_stride, mass_cap, n_pops, params, n_nodes, tab, n_wp);
}
// ... and its sibling for b9_wd_moments: the same table with every node's status behind it
template <int NFP>
__global__ __launch_bounds__(128) void k_wd_node_table_status(DevPack pk, const IsoHdr *__restrict__ hdr, const double *__restrict__ iso_data,
                                                              long long iso_stride, int mass_cap, int n_pops, const double *__restrict__ params,
                                                              int n_nodes, double *__restrict__ tab, int n_wp)
{
    wd_node_table_body<NFP, true>(pk, hdr, iso_data, iso_stride, mass_cap, n_pops, params, n_nodes, tab, n_wp);
}

// where the draws go (device pointers, [rows][n_wd] in the caller's star order); the five derived ones and pop may be null
struct WdSampleOut {
    double *zams, *member;
    double *der[B9_WDS_DER];
    int *pop;
    const int *wd_rank;              // [n_stars] column of a WD-stage star: the WD-stage stars before it in the caller's catalogue
    unsigned k0, k1;
    long long row0;
};

// ------------------------------------------------------------------------------------------
// The star kernels' frame, stated once for k_wd_sample and k_wd_bins; k_wd_moments keeps the walk written out, for its speed
// (b9_wd_moments.hip.h).  The three must agree in it to the bit (test_ties_to_wd_moments, test_ties_to_sample_wd_mass): one LANE per WD-stage star (wd_star, b9_chain_walk.hip.h; a padding lane
// reads star 0 and is never `live`), one wave per (64 stars, row); the wave stages 64-node tiles of the row's table (both
// atmosphere types) in LDS and every lane reads the SAME node -- a broadcast read -- so a node row is fetched once per 64 stars.
//
// wd_grid_walk: one population's walk over (row, population) wp.  Per tile, between the two barriers, the rows of both types and
// the log prior go to the kernel's s_rows / s_lpm, and lane i of the tile's nodes calls stage(i, j) to put the call's own columns
// of ITS node j at slot i (beside the log prior's load, under the one guard: the loads share one wait, as in the kernels before);
// then on_node(i, j, term) is called in ascending node order j = t0 + i + 1 = 1 .. n_nodes for exactly the lanes where the star is
// live and the node's chi-square finite, with term = (log prior - chi^2 / 2) + log dM.  tip, dM: out, the grid m_j = tip + dM j
// (set before the first on_node; without steps, dM <= 0, nothing is called).
// ------------------------------------------------------------------------------------------
#define B9_WDS_TILE 64
#define B9_WDS_TYPE_STRIDE(NFP) (B9_WDS_TILE * (NFP) + 2)            // (+ 2: the DB tile starts on other banks than the DA tile)
template <int NFP, class S, class F>
__device__ __forceinline__ void wd_grid_walk(const WdTable<const double> &t, const WdStar<NFP> &s, bool live, const IsoHdr *__restrict__ hdr, int wp,
                                             int n_nodes, double m_wd_up, double *s_rows, double *s_lpm, double &tip, double &dM, S stage, F on_node)
{
    const int lane = threadIdx.x;
    tip = hdr[wp].agb_tip;
    dM = (m_wd_up - tip) / n_nodes;
    if (!(dM > 0.0)) return;                                 // (wave-uniform: one row)
    const double log_w = log(dM);
    const double *__restrict__ const lpm = t.lpm + (size_t)wp * n_nodes;
    for (int t0 = 0; t0 < n_nodes; t0 += B9_WDS_TILE) {
        const int cnt = n_nodes - t0 < B9_WDS_TILE ? n_nodes - t0 : B9_WDS_TILE;
        __syncthreads();                                     // (the previous tile's reads are done)
#pragma unroll
        for (int ty = 0; ty < 2; ++ty) {
            const double *__restrict__ const src = t.rows + (((size_t)wp * 2 + ty) * n_nodes + t0) * NFP;
            for (int x = lane; x < cnt * NFP; x += 64) s_rows[ty * B9_WDS_TYPE_STRIDE(NFP) + x] = src[x];
        }
        if (lane < cnt) { s_lpm[lane] = lpm[t0 + lane]; stage(lane, t0 + lane + 1); }
        __syncthreads();
        const double *const mine = s_rows + s.wd_type * B9_WDS_TYPE_STRIDE(NFP);
        for (int i = 0; i < cnt; ++i) {
            const double *const row = mine + i * NFP;
            double chi2 = 0.0;
#pragma unroll
            for (int f = 0; f < NFP; ++f) { const double d = row[f] - s.obs[f]; chi2 = fma(s.wgt[f] * d, d, chi2); }
            if (live && isfinite(chi2)) on_node(i, t0 + i + 1, (s_lpm[i] - 0.5 * chi2) + log_w);
        }
    }
}

// k_wd_sample: per lane a running log-sum-exp and the best (key, k, j) over the walk.
// ORDER OF THE SUM (out_member is a function of the data only): a star's terms enter its population's log-sum-exp one
// by one in ascending node order j = 1 .. n_nodes, by this one lane; the populations are then mixed as b9_sample_mass
// mixes them.  Nothing of it depends on the chunk of rows, the grid or the call.  Equal keys keep the first one met:
// lowest population, then lowest node.
template <int NFP, int NPOPS>
__global__ __launch_bounds__(64) void k_wd_sample(DevPack pk, DevStars st, const IsoHdr *__restrict__ hdr, const double *__restrict__ params,
                                                  int n_nodes, const double *__restrict__ tab, int n_wp, WdSampleOut out)
{
    __shared__ __attribute__((aligned(16))) double s_rows[2 * B9_WDS_TYPE_STRIDE(NFP)];
    __shared__ double s_lpm[B9_WDS_TILE];
    const int r = blockIdx.y;
    const int k_wd = blockIdx.x * 64 + threadIdx.x;
    const bool live = k_wd < st.n_wd;
    const WdStar<NFP> s = wd_star<NFP, NPOPS>(st, hdr, params, live ? k_wd : 0, r);
    const int orig = s.orig;
    const double c0m = st.c0m[s.slot], la = st.la[s.slot];
    if (!s.valid) return;                                    // a row outside the grid: the outputs stay 0
    const double *par = s.par;
    const WdTable<const double> t = wd_table_view(tab, NFP, n_wp, n_nodes);
    const unsigned long long g_row = (unsigned long long)(out.row0 + r);
    double lw_pop[2] = {0.0, 0.0};
    if (NPOPS == 2) { const double lam = par[B9_P_LAMBDA]; lw_pop[0] = log(lam); lw_pop[1] = log1p(-lam); }
    double ll[NPOPS];
    double best_key = NEG_INF, best_mass = 0.0;
    int best_j = 0, best_k = 0;
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        Lse acc; acc.mx = NEG_INF; acc.sm = 0.0;
        double tip, dM;
        wd_grid_walk<NFP>(t, s, live, hdr, r * NPOPS + kp, n_nodes, pk.m_wd_up, s_rows, s_lpm, tip, dM, [](int, int) {}, [&](int, int j, double term) {
            lse_add(acc, term);
            const double key = term + lw_pop[kp] + gumbel(out.k0, out.k1, g_row, (unsigned)orig, (unsigned long long)j, (unsigned)kp);
            if (key > best_key) { best_key = key; best_mass = tip + dM * (double)j; best_j = j; best_k = kp; }
        });
        ll[kp] = (acc.mx == NEG_INF) ? NEG_INF : c0m + (acc.mx + log(acc.sm));
    }
    if (!live) return;
    const StarFinish fin = finish_star<NPOPS>(ll, par, la);
    const double l = fin.l, v = fin.v;
    const size_t o = (size_t)r * st.n_wd + out.wd_rank[orig];
    const bool any = best_key != NEG_INF;
    out.zams[o] = any ? best_mass : 0.0;
    out.member[o] = (l == NEG_INF) ? 0.0 : exp(l - v);           // p L_cluster / (p L_cluster + (1 - p) L_field)
    if (out.pop) out.pop[o] = any ? best_k : 0;
    // the winner's derived values: gathered from the table by node index
    const double *d = t.der + ((size_t)(r * NPOPS + best_k) * n_nodes + (size_t)(any ? best_j - 1 : 0)) * B9_WDS_DER;
#pragma unroll
    for (int q = 0; q < B9_WDS_DER; ++q)
        if (out.der[q]) out.der[q][o] = any ? d[q] : 0.0;
}
