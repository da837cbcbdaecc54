// b9_filter_loo.hip.h -- b9_filter_loo (the filterCheck counterpart): k_star_loo (MS/RGB-stage stars, one LANE per star),
// k_star_loo_wd (WD-stage stars, one WAVE per star) and k_loo_rows (a row's sums over the stars).  The call's pivots and
// log(sigma sqrt(2 pi)) words are staged by b9_phot_resid's k_resid_stage.  Part of the single translation unit b9_kernels.hip
// (included there, after b9_phot_resid.hip.h); gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------
// Exact leave-one-filter-out predictions over a chain ("Leave-one-filter-out predictions").  The grid,
// the node terms t_(k, n), L, the FULL-DATA membership p and the WD-stage steps are b9_star_moments'.  For a filter f the star
// uses, g_f(n) = ((sw_f pred_f - so_f)^2) / 2 is the node's share of its own chi^2 (the scaled pair the chi^2 is formed from);
// g_f = 0 for an unused filter.  Leave-out f has the terms t^f = t + g_f, L^f = logsumexp t^f (the populations mixed by that
// leave-out's own weights) and w^f = exp(t^f - L^f).  With d_f = pred_f - c_f (b9_phot_resid's pivot)
//     x = {1, p, then per filter  p sum w^f d_f,  p sum w^f d_f^2,  p l_f},   l_f = (L - L^f) - log(sigma_f sqrt(2 pi))   (2 + 3 nf columns)
// per (row, star) in a scratch [row][star][2 + 3 nf] in the caller's star order; l_f = 0 exactly for an unused filter.
// k_chain_accumulate adds the rows in ascending row order, k_loo_rows sums a row over the stars in ascending star order.
//
// The full-data sum (ref, S0) adds exactly the terms walk_nodes calls live, in its order: walk_nodes_loo visits a SUPERSET of
// walk_nodes' units and forms `live` by the same comparison against the same bound at the same moments, so x[0] and x[1] are
// b9_phot_resid's bits.  Every leave-out has its own online log-sum-exp (ref_f, S0_f, sum e d_f, sum e d_f^2: lse_step, whose
// jump rescales these three sums only) and its own running maximum tmax_f, which starts from walk_start's seed -- a valid
// lower bound of max t^f because t^f >= t -- and follows that leave-out's terms: a node enters leave-out f while
// t^f > tmax_f - B9_MARG_CUT.  What is dropped is below N_nodes e^-40 of that sum's weight.
//
// Box pruning (rigorous, built: it spares the chi^2 of most of the table at real sigmas).  For the rows of a box the scaled
// distances m_g bound every |sw_g pred_g - so_g| from below, so X - 2 g_f >= sum_g m_g^2 - max_f m_f^2 + nbmin for every
// leave-out f of the tile: a chunk or a unit is skipped only when that bound excludes it for the LARGEST of the tile's cuts
// (cut2 - 2 min_f tmax_f) and the plain bound excludes it for the full-data cut, in every lane.  marg_no_pruning: cut2 = inf,
// nothing is dropped.
//
// Filter tiling.  A wave's state is 2 + 4 LT doubles per lane and population for a tile of LT leave-outs.  At 16 filters the
// whole set would be 66 doubles (135 KB for the four wave states, 132 VGPRs of sums); the 16-filter instances therefore tile the
// leave-outs in two tiles of 8 over gridDim.z (70 KB of dynamic LDS).  Every leave-out has its own exponent anyway, so a tile
// repeats only the node's chi^2 and the full-data sum.  4 and 8 filters: one tile.  Tile 0 writes x[0] and x[1]; a tile writes
// the three columns of its own filters only.  Populations one after the other through the one LDS block, as k_star_resid.
// ------------------------------------------------------------------------------------------
template <int NFP> struct LooTile { static constexpr int LT = NFP >= 16 ? 8 : NFP; };

// A = logsumexp_k(log lambda_k + lg_k) and the populations' weights e^(log lambda_k + lg_k - A): star_finish's expressions, so
// that a leave-out whose lg equal the full-data ones mixes by the same bits
template <int NPOPS>
__device__ __forceinline__ double loo_mix(const double (&lg)[NPOPS], const double *par, double (&wk)[NPOPS])
{
    double a[NPOPS];
#pragma unroll
    for (int k = 0; k < NPOPS; ++k) {
        a[k] = lg[k];
        if (NPOPS == 2) { const double lam = par[B9_P_LAMBDA]; a[k] = (lg[k] == NEG_INF) ? NEG_INF : (k ? log1p(-lam) : log(lam)) + lg[k]; }
        wk[k] = 0.0;
    }
    wk[0] = 1.0;
    double A = a[0];
    if (NPOPS == 2) {
        A = logaddexp(a[0], a[NPOPS - 1]);
#pragma unroll
        for (int k = 0; k < NPOPS; ++k) wk[k] = (a[k] == NEG_INF) ? 0.0 : exp(a[k] - A);
    }
    return A;
}

// box_bound64 and, in lb_loo, the same bound less the largest part among the filters [f0, f0 + LT)
template <int NFP, int LT>
__device__ __forceinline__ double loo_box_bound(b9_ctab box, const double (&so)[NFP], const double (&sw)[NFP], int f0, double &lb_loo)
{
    double lb = 0.0, mx = 0.0;
#pragma unroll
    for (int f = 0; f < NFP; ++f) {
        double a, b;
        asm("v_fma_f64 %0, %1, %2, -%3" : "=v"(a) : "v"(sw[f]), "s"(box[f]), "v"(so[f]));          // sw lo - so
        asm("v_fma_f64 %0, -%1, %2, %3" : "=v"(b) : "v"(sw[f]), "s"(box[NFP + f]), "v"(so[f]));   // so - sw hi
        double m = max_vv(a, b);
        asm("v_max_f64 %0, %1, 0" : "=v"(m) : "v"(m));
        const double m2 = m * m;
        lb = fma(m, m, lb);
        if (LT == NFP || (f >= f0 && f < f0 + LT)) mx = max_vv(mx, m2);
    }
    lb_loo = lb - mx;
    return lb;
}

// walk_nodes' walk over a superset of its units.  `live` is walk_nodes' own: the same comparison against the same bound, which
// moves at the same moments (a unit walk_nodes skips has no live node and leaves tmax alone).  xcut_loo(): the largest of the
// tile's leave-out cuts, as a bound on X - 2 g_f; on_node(live, x, row) for every node of a unit that is not skipped.
template <int NFP, int LT, class C, class F>
__device__ __forceinline__ void walk_nodes_loo(b9_ctab t_wp, const MargLayout &L, int n_nodes, int Q, int wave, bool dead, double cut2, double &tmax,
                                               const double (&so)[NFP], const double (&sw)[NFP], int f0, C xcut_loo, F on_node)
{
    const int n_chunks = (n_nodes + 63) >> 6;
    for (int c = 0; c < n_chunks; ++c) {
        double xcut = dead ? NEG_INF : fma(-2.0, tmax, cut2);
        double xcl = dead ? NEG_INF : xcut_loo();
        {
            double lbl;
            const double lb = loo_box_bound<NFP, LT>(t_wp + L.o_box1 + (size_t)c * 2 * NFP, so, sw, f0, lbl), nbm = t_wp[L.o_nbmin64 + c];
            if (__ballot(lb + nbm < xcut || lbl + nbm < xcl) == 0ull) continue;
        }
        for (int sub = 0; sub < 4; ++sub) {
            const int u = c * 4 + sub;
            const double nbm = t_wp[L.o_nbmin16 + u];
            for (int j = (wave - 2 * sub) & 3; j < Q; j += 4) {
                double lbl;
                const double lb = loo_box_bound<NFP, LT>(t_wp + L.o_box2 + ((size_t)u * Q + j) * 2 * NFP, so, sw, f0, lbl);
                if (__ballot(lb + nbm < xcut || lbl + nbm < xcl) == 0ull) continue;
                const b9_ctab rowp = t_wp + L.o_rows + ((size_t)u * Q + j) * 16 * NFP;
                for (int i = 0; i < 16; ++i) {
                    const int node = u * 16 + i;
                    const double x = row_x<NFP>(rowp + i * NFP, t_wp[L.o_nb + node], so, sw);
                    const bool live = x < xcut;
                    on_node(live, x, rowp + i * NFP);
                    tmax = max_vv(tmax, live ? -0.5 * x : tmax);
                }
                xcut = dead ? NEG_INF : fma(-2.0, tmax, cut2);
                xcl = dead ? NEG_INF : xcut_loo();
            }
        }
    }
}

// piv_mg / lsn_mg: the pivots and log(sigma sqrt(2 pi)) (0 for an unused filter) in the mg_* copy's layout (k_resid_stage)
template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_loo(DevStars st, int nf, const double *__restrict__ piv_mg, const double *__restrict__ lsn_mg,
                                                  const IsoHdr *__restrict__ hdr, const double *__restrict__ iso_data, long long iso_stride, int mass_cap,
                                                  const double *__restrict__ params, int K, int Q, const double *__restrict__ tab, MargLayout L,
                                                  double cut2, double *__restrict__ scratch)
{
    constexpr int LT = LooTile<NFP>::LT, NW = 2 + 4 * LT;     // a state: {ref, S0, then per leave-out ref_f, S0_f, sum e d, sum e d^2}
    extern __shared__ __attribute__((aligned(16))) double s_lds[];
    double (*const s_seed)[4][64] = reinterpret_cast<double (*)[4][64]>(s_lds);                          // [NPOPS][wave][lane]
    double (*const s_state)[NW][64] = reinterpret_cast<double (*)[NW][64]>(s_lds + NPOPS * 4 * 64);      // [wave][word][lane]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sc = blockIdx.x, w = blockIdx.y, f0 = blockIdx.z * LT, ncol = 2 + 3 * nf;
    const int slot = sc * 64 + lane, orig = st.mg_perm[slot];
    const bool dead = orig < 0;
    double so[NFP], sw[NFP], piv[LT];
#pragma unroll
    for (int f = 0; f < NFP; ++f) { so[f] = st.mg_so[B9_SIDX(NFP, f, slot)]; sw[f] = st.mg_sw[B9_SIDX(NFP, f, slot)]; }
#pragma unroll
    for (int j = 0; j < LT; ++j) piv[j] = piv_mg[B9_SIDX(NFP, f0 + j, slot)];
    const double *par = params + (size_t)w * B9_NPARAM;
    double *const out = scratch + ((size_t)w * st.n + (dead ? 0 : orig)) * ncol;
    IsoView<NFP> iso[NPOPS];
    double tip_min;
    const bool valid = load_iso_views<NFP, NPOPS>(hdr, iso_data, iso_stride, mass_cap, w, iso, tip_min);
    if (!valid) {                                        // a row outside the grid contributes nothing (tile 0 clears the line)
        if (wave == 0 && !dead && blockIdx.z == 0)
            for (int c = 0; c < ncol; ++c) out[c] = 0.0;
        return;
    }

#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp)
        s_seed[kp][wave][lane] = walk_seed<NFP>((b9_ctab)(tab + (size_t)(w * NPOPS + kp) * L.total), L, (iso[kp].n - 1) * K, Q, wave, so, sw);
    __syncthreads();

    const double cut = 0.5 * cut2;
    double lg[NPOPS];
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        const b9_ctab t_wp = (b9_ctab)(tab + (size_t)(w * NPOPS + kp) * L.total);
        double tmax = walk_start(s_seed[kp], lane);
        double ref = tmax, S0 = 0.0;
        double tmf[LT], rf[LT], s0f[LT], s1f[LT], s2f[LT];
#pragma unroll
        for (int j = 0; j < LT; ++j) { tmf[j] = tmax; rf[j] = tmax; s0f[j] = 0.0; s1f[j] = 0.0; s2f[j] = 0.0; }
        walk_nodes_loo<NFP, LT>(t_wp, L, (iso[kp].n - 1) * K, Q, wave, dead, cut2, tmax, so, sw, f0, [&]() {
            double mn = tmf[0];
#pragma unroll
            for (int j = 1; j < LT; ++j) mn = __builtin_fmin(mn, tmf[j]);
            return fma(-2.0, mn, cut2);
        }, [&](bool live, double x, b9_ctab row) {
            const double t = -0.5 * x;
            if (live) {
                const double e = lse_step(t, ref, [&](double scale) { S0 *= scale; });
                S0 += e;
            }
#pragma unroll
            for (int j = 0; j < LT; ++j) {
                // (the tile's filter f0 + j: so / sw are indexed by a select chain only where the kernel is tiled)
                double sof = so[j], swf = sw[j];
                if (LT != NFP) {
#pragma unroll
                    for (int z = 1; z < NFP / LT; ++z) { sof = (f0 == z * LT) ? so[z * LT + j] : sof; swf = (f0 == z * LT) ? sw[z * LT + j] : swf; }
                }
                const double rw = (LT == NFP) ? row[j] : row[f0 + j];
                const double dd = fma(swf, rw, -sof);
                const double tf = fma(0.5 * dd, dd, t);
                const bool lf = !dead && tf > tmf[j] - cut;
                if (lf) {
                    const double e = lse_step(tf, rf[j], [&](double scale) { s0f[j] *= scale; s1f[j] *= scale; s2f[j] *= scale; });
                    s0f[j] += e;
                    const double d = rw - piv[j], ed = e * d;
                    s1f[j] += ed;
                    s2f[j] = fma(ed, d, s2f[j]);
                    tmf[j] = max_vv(tmf[j], tf);
                }
            }
        });
        s_state[wave][0][lane] = ref; s_state[wave][1][lane] = S0;
#pragma unroll
        for (int j = 0; j < LT; ++j) {
            s_state[wave][2 + 4 * j][lane] = rf[j]; s_state[wave][3 + 4 * j][lane] = s0f[j];
            s_state[wave][4 + 4 * j][lane] = s1f[j]; s_state[wave][5 + 4 * j][lane] = s2f[j];
        }
        __syncthreads();

        // ---- wave 0: the four shares merged in wave order, the full-data pair and each leave-out's group on its own.  A population
        // before the last parks the leave-out's normalised sums and its log-sum in the output's three columns (a lane reads back
        // only what it wrote itself); the last one mixes them with that leave-out's own weights
        if (wave == 0 && !dead) {
            const WaveMerge mg = wave_merge(s_state, lane);
            lg[kp] = (mg.S0 > 0.0) ? mg.r + log(mg.S0) : NEG_INF;
            double p = 0.0, wk[NPOPS], A = 0.0;
            bool any = false;
            if (kp == NPOPS - 1) { any = star_finish<NPOPS>(lg, st.mg_c0m[slot], st.mg_la[slot], par, p, wk); A = loo_mix<NPOPS>(lg, par, wk); }
            for (int j = 0; j < LT; ++j) {
                const int f = f0 + j;
                if (f >= nf) break;
                const WaveMerge mf = wave_merge(reinterpret_cast<const double (*)[NW][64]>(&s_state[0][2 + 4 * j][0]), lane);
                const double lgf = (mf.S0 > 0.0) ? mf.r + log(mf.S0) : NEG_INF;
                const double mn1 = (mf.S0 > 0.0) ? wave_sum(mf, &s_state[0][4 + 4 * j][lane], NW * 64) / mf.S0 : 0.0;
                const double mn2 = (mf.S0 > 0.0) ? wave_sum(mf, &s_state[0][5 + 4 * j][lane], NW * 64) / mf.S0 : 0.0;
                double *const o = out + 2 + 3 * f;
                if (kp < NPOPS - 1) { o[0] = mn1; o[1] = mn2; o[2] = lgf; continue; }
                double lf[NPOPS], wf[NPOPS];
                lf[NPOPS - 1] = lgf;
                if (NPOPS == 2) lf[0] = o[2];
                const double Af = loo_mix<NPOPS>(lf, par, wf);
                double m1 = wf[NPOPS - 1] * mn1, m2 = wf[NPOPS - 1] * mn2;
                if (NPOPS == 2) { m1 = wf[0] * o[0] + m1; m2 = wf[0] * o[1] + m2; }
                const bool used = st.mg_sw[B9_SIDX(NFP, f, slot)] > 0.0;
                const double lpd = used ? (A - Af) - lsn_mg[B9_SIDX(NFP, f, slot)] : 0.0;
                o[0] = any ? p * m1 : 0.0; o[1] = any ? p * m2 : 0.0; o[2] = any ? p * lpd : 0.0;
            }
            if (kp == NPOPS - 1 && blockIdx.z == 0) { out[0] = any ? 1.0 : 0.0; out[1] = any ? p : 0.0; }
        }
        if (kp + 1 < NPOPS) __syncthreads();             // the block is the next population's
    }
}

// ------------------------------------------------------------------------------------------
// k_star_loo_wd: the WD-stage stars (b9_chain_walk.hip.h), no pruning.  Per lane the full-data pair (mx, S0), then ONE lser group
// {S0_f, sum d_f, sum d_f^2} with its own maximum per leave-out -- lser_merge shares one maximum among its sums --, merged by the
// wave's shuffle tree; the leave-outs in the tiles of k_star_loo (all 16 groups at once carry scratch: docs/LABNOTES.md).
// g_f = ((wgt_f d_f) d_f) / 2, the product the chi^2 adds.  lsn: [n_stars][nf], the caller's order.
// ------------------------------------------------------------------------------------------
// what lane 0 needs to finish a WD-stage star's leave-outs
struct LooWdStar { int nf, lane; bool any; double p, A; const double *lsn; double *out; };
// the leave-outs [F0, F0 + LT) of population KP: the wave's steps, the groups' merge, and lane 0's finish -- a population before
// the last parks the leave-out's normalised sums and its log-sum in the output, as k_star_loo does
template <int NFP, int NPOPS, int F0, int KP>
__device__ __forceinline__ void loo_wd_tile(const WdStar<NFP> &ws, const WdSteps<NFP> &sp, const LooWdStar &fin)
{
    constexpr int LT = LooTile<NFP>::LT;
    double mxf[LT], sf[LT][3];
#pragma unroll
    for (int q = 0; q < LT; ++q) { mxf[q] = NEG_INF; sf[q][0] = 0.0; sf[q][1] = 0.0; sf[q][2] = 0.0; }
    if (sp.on) {
        for (int j = 1 + fin.lane; j <= sp.steps; j += 64) {
            const double *__restrict__ const r = sp.rows + (size_t)(j - 1) * NFP;
            double d[NFP], chi2 = 0.0;
#pragma unroll
            for (int f = 0; f < NFP; ++f) { d[f] = r[f] - ws.obs[f]; chi2 = fma(ws.wgt[f] * d[f], d[f], chi2); }
            if (isfinite(chi2)) {
                const double term = (sp.lpm[j - 1] - 0.5 * chi2) + sp.log_w;
                if (term == NEG_INF) continue;
#pragma unroll
                for (int q = 0; q < LT; ++q) {
                    const double dq = d[F0 + q], b[3] = {1.0, dq, dq * dq};
                    lser_merge<3>(mxf[q], sf[q], fma(0.5 * (ws.wgt[F0 + q] * dq), dq, term), b);
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < LT; ++q) {
        lser_wave<3>(mxf[q], sf[q]);
        const int f = F0 + q;
        if (fin.lane == 0 && f < fin.nf) {
            const bool has = mxf[q] != NEG_INF && sf[q][0] > 0.0;
            const double lgf = has ? mxf[q] + log(sf[q][0]) : NEG_INF;
            const double mn1 = has ? sf[q][1] / sf[q][0] : 0.0, mn2 = has ? sf[q][2] / sf[q][0] : 0.0;
            double *const o = fin.out + 2 + 3 * f;
            if (KP < NPOPS - 1) { o[0] = mn1; o[1] = mn2; o[2] = lgf; }
            else {
                double lf[NPOPS], wf[NPOPS];
                lf[NPOPS - 1] = lgf;
                if (NPOPS == 2) lf[0] = o[2];
                const double Af = loo_mix<NPOPS>(lf, ws.par, wf);
                double m1 = wf[NPOPS - 1] * mn1, m2 = wf[NPOPS - 1] * mn2;
                if (NPOPS == 2) { m1 = wf[0] * o[0] + m1; m2 = wf[0] * o[1] + m2; }
                const double lpd = ws.wgt[f] > 0.0 ? (fin.A - Af) - fin.lsn[f] : 0.0;
                o[0] = fin.any ? fin.p * m1 : 0.0; o[1] = fin.any ? fin.p * m2 : 0.0; o[2] = fin.any ? fin.p * lpd : 0.0;
            }
        }
    }
}

template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_loo_wd(DevStars st, int nf, double m_wd_up, const IsoHdr *__restrict__ hdr,
                                                     const double *__restrict__ params, int K, const double *__restrict__ wtab,
                                                     const double *__restrict__ lsn, double *__restrict__ scratch)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k_wd = blockIdx.x * 4 + wave, w = blockIdx.y, n_wp = gridDim.y * NPOPS, ncol = 2 + 3 * nf;
    if (k_wd >= st.n_wd) return;
    const WdStar<NFP> ws = wd_star<NFP, NPOPS>(st, hdr, params, k_wd, w);
    double *__restrict__ const out = scratch + ((size_t)w * st.n + ws.orig) * ncol;
    if (!ws.valid) {
        for (int c = lane; c < ncol; c += 64) out[c] = 0.0;
        return;
    }
    // ---- the full-data sums: k_star_resid_wd's S0, term for term
    double lg[NPOPS];
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        const WdSteps<NFP> sp = wd_steps<NFP>(ws, m_wd_up, hdr, K, wtab, w * NPOPS + kp, n_wp);
        double mx = NEG_INF, s[1] = {0.0};
        if (sp.on) {
            for (int j = 1 + lane; j <= sp.steps; j += 64) {
                const double term = sp.term(ws, j);
                if (term == NEG_INF) continue;
                const double one[1] = {1.0};
                lser_merge<1>(mx, s, term, one);
            }
        }
        lser_wave<1>(mx, s);
        lg[kp] = (mx != NEG_INF && s[0] > 0.0) ? mx + log(s[0]) : NEG_INF;
    }
    double p, wk[NPOPS];
    const bool any = star_finish<NPOPS>(lg, st.c0m[ws.slot], st.la[ws.slot], ws.par, p, wk);
    const double A = loo_mix<NPOPS>(lg, ws.par, wk);
    // ---- the leave-outs, a tile of LT at a time (the steps are walked again per tile: 8 K of them)
    const LooWdStar fin{nf, lane, any, p, A, lsn + (size_t)ws.orig * nf, out};
    constexpr int LT = LooTile<NFP>::LT;
    loo_wd_tile<NFP, NPOPS, 0, 0>(ws, wd_steps<NFP>(ws, m_wd_up, hdr, K, wtab, w * NPOPS, n_wp), fin);
    if constexpr (NPOPS == 2) loo_wd_tile<NFP, NPOPS, 0, 1>(ws, wd_steps<NFP>(ws, m_wd_up, hdr, K, wtab, w * NPOPS + 1, n_wp), fin);
    if constexpr (LT < NFP) {
        loo_wd_tile<NFP, NPOPS, LT, 0>(ws, wd_steps<NFP>(ws, m_wd_up, hdr, K, wtab, w * NPOPS, n_wp), fin);
        if constexpr (NPOPS == 2) loo_wd_tile<NFP, NPOPS, LT, 1>(ws, wd_steps<NFP>(ws, m_wd_up, hdr, K, wtab, w * NPOPS + 1, n_wp), fin);
    }
    if (lane == 0) { out[0] = any ? 1.0 : 0.0; out[1] = any ? p : 0.0; }
}

// k_loo_rows: k_resid_rows with the sixth column.  A row's sums over the stars in ascending (the caller's) order, one plain add
// each, from the scratch values x [n_stars][2 + 3 nf] and s = 1 / sigma (isig, 0 = filter unused: the star is left out of that
// filter's sums):  N += p,  R += -(x[2 + 3f] s),  C += (x[3 + 3f] s) s,  W += (p s) s,  D += -((x[2 + 3f] s) s),  E += x[4 + 3f];
// column 0 += p (every star).  One workgroup per row, one OWNER lane per output column (6 nf + 1), the row's words streamed
// through LDS in tiles of B9_LOO_TILE stars as k_resid_rows does (two buffers: 135 KB of dynamic LDS at 16 filters, 69 KB at 8).
// rows: [n_rows][1 + 6 nf].
#define B9_LOO_TILE 128
#define B9_LOO_TILE_LOADS ((B9_LOO_TILE * (2 + 4 * B9_MAX_FILT) + 255) / 256)      // words of a tile per lane, at most
__global__ __launch_bounds__(256) void k_loo_rows(const double *__restrict__ scratch, const double *__restrict__ isig, int n_stars, int nf,
                                                  double *__restrict__ rows)
{
    extern __shared__ __attribute__((aligned(16))) double s_tile[];       // two buffers of {x [TILE][ncol], s [TILE][nf]}
    const int tid = threadIdx.x, r = blockIdx.x, ncol = 2 + 3 * nf, tile_words = B9_LOO_TILE * (ncol + nf);
    const double *__restrict__ const x = scratch + (size_t)r * n_stars * ncol;
    // the owner's column: o = 6 f + q (q: N, R, C, W, D, E) or 6 nf (column 0)
    const int n_owner = 6 * nf + 1;
    const bool owner = tid < n_owner, total = tid == 6 * nf;
    const int f = total ? 0 : tid / 6, q = tid - 6 * f;
    const int word = (total || q == 0 || q == 3) ? 1 : (q == 1 || q == 4) ? 2 + 3 * f : (q == 2) ? 3 + 3 * f : 4 + 3 * f;
    const bool plain = total || q == 0 || q == 5, twice = q >= 2, neg = q == 1 || q == 4;
    double acc = 0.0, v[B9_LOO_TILE_LOADS];
    auto fetch = [&](int s0) {                          // tile [s0, s0 + tn) -> registers: the x words, then the s words
        const int tn = min(B9_LOO_TILE, n_stars - s0), nx = tn * ncol, ns = tn * nf;
        const double *__restrict__ const xb = x + (size_t)s0 * ncol, *__restrict__ const sb = isig + (size_t)s0 * nf;
#pragma unroll
        for (int k = 0; k < B9_LOO_TILE_LOADS; ++k) {
            if (k * 256 < nx + ns) {                    // (wave-uniform)
                const int w = tid + k * 256;
                const double *ptr = w < nx ? xb + w : sb + min(w - nx, ns - 1);
                v[k] = *ptr;
            }
        }
    };
    auto stash = [&](int s0, double *buf) {             // registers -> LDS: x at 0, s at TILE * ncol
        const int tn = min(B9_LOO_TILE, n_stars - s0), nx = tn * ncol, ns = tn * nf;
#pragma unroll
        for (int k = 0; k < B9_LOO_TILE_LOADS; ++k) {
            const int w = tid + k * 256;
            if (k * 256 < nx + ns && w < nx + ns) buf[w < nx ? w : B9_LOO_TILE * ncol + (w - nx)] = v[k];
        }
    };
    if (n_stars > 0) { fetch(0); stash(0, s_tile); }
    __syncthreads();
    for (int s0 = 0, t = 0; s0 < n_stars; s0 += B9_LOO_TILE, ++t) {
        const double *cur = s_tile + (size_t)(t & 1) * tile_words;
        double *nxt = s_tile + (size_t)((t + 1) & 1) * tile_words;
        const bool more = s0 + B9_LOO_TILE < n_stars;
        if (more) fetch(s0 + B9_LOO_TILE);
        if (owner) {
            const int tn = min(B9_LOO_TILE, n_stars - s0);
            const double *xw = cur + word, *sw = cur + B9_LOO_TILE * ncol + f;
            auto add = [&](double p, double s) {         // one star, in order: the only chain is acc
                const double a = p * s, b = a * s;
                double val = plain ? p : (twice ? b : a);
                val = neg ? -val : val;
                acc = s > 0.0 ? acc + val : acc;
            };
            // (B9_RESID_AHEAD stars' LDS words are read before the adds that consume them, as in k_resid_rows)
            int k = 0;
            for (; k + B9_RESID_AHEAD <= tn; k += B9_RESID_AHEAD) {
                double pv[B9_RESID_AHEAD], sv[B9_RESID_AHEAD];
#pragma unroll
                for (int u = 0; u < B9_RESID_AHEAD; ++u) { pv[u] = xw[(k + u) * ncol]; sv[u] = total ? 1.0 : sw[(k + u) * nf]; }
#pragma unroll
                for (int u = 0; u < B9_RESID_AHEAD; ++u) add(pv[u], sv[u]);
            }
            for (; k < tn; ++k) add(xw[k * ncol], total ? 1.0 : sw[k * nf]);
        }
        if (more) stash(s0 + B9_LOO_TILE, nxt);
        __syncthreads();
    }
    if (owner) rows[(size_t)r * n_owner + (total ? 0 : 1 + tid)] = acc;
}
