// b9_wd_bins.hip.h -- b9_wd_bins (the wdIntervals counterpart): k_wd_bins, one LANE per WD-stage star against
// k_wd_node_table_status' table, every star's node weights binned on that star's OWN edges, one selected quantity per blockIdx.z.
// Part of the single translation unit b9_kernels.hip (included there, after b9_wd_moments.hip.h and b9_star_bins.hip.h); gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------
// Per-WD bins over a chain (include/base9_hip.h, DESIGN.md section 2, "Per-WD bins and credible intervals").  The grid, the
// terms, the weights, the membership and a node's COOLED status are b9_wd_moments'; the columns are b9_star_bins': line
// (star i, selected quantity s) has its OWN edges e_0 < ... < e_B, column 0 holds the nodes below e_0, column 1 + b bin b, column
// B + 1 the nodes at or above e_B, column B + 2 the total p.  A node's value is m_j = tip + dM j under B9_WQ_ZAMS and the table's
// derived value under the other five, where only COOLED nodes count: any other node enters no column but the total.
// Increments go per (row, star, selected quantity) to a scratch [row][n_wd][n_sel][B + 3] in the order of b9_sample_wd_mass's
// columns and k_chain_accumulate adds the rows.
//
// k_wd_bins goes through wd_grid_walk (b9_wd_sample.hip.h: the lane's star, the tiles, the terms) with blockIdx.z the selected
// quantity: beside the walk's rows and log prior a block stages the status and that quantity's derived column alone.  The binning is k_star_bins': the 64 lanes' edges staged once per block as [edge][64]
// (gathered from the caller's order through wd_rank; the lane is the bank), the wave's histogram [B + 2][64] in LDS, a bank per
// lane; a lane keeps its current bin and that bin's two edges in registers and searches its own column (sbin_search) only when
// a value leaves them -- neighbouring nodes have neighbouring values.
// ORDER OF THE SUMS (a function of the data only): k_wd_moments' -- a star's terms enter its population's online log-sum-exp one
// by one in ascending node order by this one lane (hist_term: lse_step, every column rescaled together on a jump); each column
// is divided by the population's S0, the populations are mixed with star_finish's weights in population order and multiplied
// by p: the sequence k_wd_moments applies to its cooled sum.  Hence the total is B9_WDM_MEMBER and, with one bin that encloses
// every value, column 1 of a derived quantity is B9_WDM_COOLED, bit for bit.
// Dynamic LDS: [edges (n_bins + 1)][64], [histogram (n_bins + 2)][64] doubles.
// ------------------------------------------------------------------------------------------
template <int NFP, int NPOPS>
__global__ __launch_bounds__(64) void k_wd_bins(DevPack pk, DevStars st, const IsoHdr *__restrict__ hdr, const double *__restrict__ params,
                                                int n_nodes, const double *__restrict__ tab, int n_wp, const int *__restrict__ wd_rank,
                                                int quantity_mask, int n_sel, const double *__restrict__ edges, int n_bins,
                                                double *__restrict__ scratch)
{
    __shared__ __attribute__((aligned(16))) double s_rows[2 * B9_WDS_TYPE_STRIDE(NFP)];
    __shared__ double s_lpm[B9_WDS_TILE], s_val[B9_WDS_TILE], s_stat[B9_WDS_TILE];
    extern __shared__ __attribute__((aligned(16))) double s_lds[];
    double *const s_edge = s_lds;                                            // [edge][lane]
    double *const s_hist = s_lds + (size_t)(n_bins + 1) * 64;               // [column < n_bins + 2][lane]
    const int lane = threadIdx.x, r = blockIdx.y, sel = blockIdx.z;
    const int tb = n_bins + 2, ncol = n_bins + 3;
    // the sel-th quantity of the mask, ascending (wave-uniform)
    int quantity = 0;
    for (int q = 0, k = 0; q < B9_WQ_N; ++q)
        if (quantity_mask >> q & 1) { if (k == sel) quantity = q; ++k; }
    const bool zams = quantity == B9_WQ_ZAMS;
    const int k_wd = blockIdx.x * 64 + lane;
    const bool live = k_wd < st.n_wd;
    const WdStar<NFP> star = wd_star<NFP, NPOPS>(st, hdr, params, live ? k_wd : 0, r);
    const int slot = star.slot;
    const size_t line = (size_t)wd_rank[star.orig] * n_sel + sel;            // the caller's line (a padding lane: star 0's, never written)
    double *__restrict__ const out = scratch + ((size_t)r * st.n_wd * n_sel + line) * ncol;
    if (!star.valid) {                                       // a row outside the grid contributes nothing
        if (live)
            for (int c = 0; c < ncol; ++c) out[c] = 0.0;
        return;
    }
    // the lane's own edges (a padding lane: zeros, never counted); every lane reads its own column alone
    for (int b = 0; b <= n_bins; ++b) s_edge[b * 64 + lane] = live ? edges[line * (n_bins + 1) + b] : 0.0;
    double *const h_mine = s_hist + lane;
    const double *const e_mine = s_edge + lane;
    const double *par = star.par;
    const WdTable<const double> t = wd_table_view(tab, NFP, n_wp, n_nodes);
    const double *__restrict__ const stat_all = t.der + (size_t)n_wp * n_nodes * B9_WDS_DER;
    double lg[NPOPS];
    bool has_k[NPOPS];
    double s0_k[NPOPS];
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        double ref = NEG_INF, s0 = 0.0;
        for (int b = 0; b < tb; ++b) h_mine[b * 64] = 0.0;
        // the bin the lane's last node fell in: c_lo <= v < c_hi keeps it (an empty interval to start with)
        double c_lo = __builtin_inf(), c_hi = NEG_INF;
        int c_b = -1;
        const int wp = r * NPOPS + kp;
        const double *__restrict__ const der = t.der + (size_t)wp * n_nodes * B9_WDS_DER;
        const double *__restrict__ const stat = stat_all + (size_t)wp * n_nodes;
        double tip, dM;
        wd_grid_walk<NFP>(t, star, live, hdr, wp, n_nodes, pk.m_wd_up, s_rows, s_lpm, tip, dM, [&](int i, int j) {
            s_stat[i] = stat[j - 1];
            s_val[i] = zams ? 0.0 : der[(size_t)(j - 1) * B9_WDS_DER + (quantity - 1)];
        }, [&](int i, int j, double term) {
            const bool counts = zams || s_stat[i] == 2.0;
            const double v = zams ? tip + dM * (double)j : s_val[i];
            if (counts && !(v >= c_lo && v < c_hi)) {
                c_b = sbin_search(e_mine, n_bins, v);
                c_lo = c_b >= 0 ? e_mine[c_b * 64] : NEG_INF;
                c_hi = c_b < n_bins ? e_mine[(c_b + 1) * 64] : __builtin_inf();
            }
            hist_term(term, counts ? c_b + 1 : -1, tb, ref, s0, h_mine);
        });
        const bool has = ref != NEG_INF;
        lg[kp] = has ? ref + log(s0) : NEG_INF;
        has_k[kp] = has; s0_k[kp] = s0;
        // every population but the last: its normalised columns wait in the line's own scratch words (this lane wrote them)
        if (kp < NPOPS - 1 && live)
            for (int b = 0; b < tb; ++b) out[b] = has ? h_mine[b * 64] / s0 : 0.0;
    }
    if (!live) return;
    // the star finished: membership and the populations' weights, the columns mixed in population order
    double p, wk[NPOPS];
    const bool any = star_finish<NPOPS>(lg, st.c0m[slot], st.la[slot], par, p, wk);
    for (int b = 0; b < tb; ++b) {
        const double hn = has_k[NPOPS - 1] ? h_mine[b * 64] / s0_k[NPOPS - 1] : 0.0;
        double m = 0.0;
        if (NPOPS == 2) m += wk[0] * out[b];
        m += wk[NPOPS - 1] * hn;
        out[b] = any ? p * m : 0.0;
    }
    out[tb] = any ? p : 0.0;
}
