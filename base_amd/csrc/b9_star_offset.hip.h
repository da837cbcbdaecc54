// b9_star_offset.hip.h -- b9_star_offset (the starOffsets counterpart): k_offset_stage (the call's scaled directions in the mg_*
// order, and every star's C, V, pruning factor and Occam term), k_star_off (MS/RGB-stage stars, one LANE per star), k_star_off_wd
// (WD-stage stars, one WAVE per star) and k_off_rows (a row's sums over the stars).  Part of the single translation unit
// b9_kernels.hip (included there, after b9_filter_loo.hip.h); gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------
// Exact per-star offsets over a chain ("Per-star offsets").  The grid, the node terms t_(k, n), L, the
// FULL-DATA membership p and the WD-stage steps are b9_star_moments'.  Direction j is a vector k[f] over the filters and a prior
// width tau: the star's magnitudes are taken to be off by delta k[f], delta ~ N(0, tau^2).  With c_f = k_f / sigma_f (0 for an
// unused filter), C = sum c_f^2, V = 1 / (C + tau^-2) and dd_f = fma(sw_f, pred_f, -so_f) (the scaled pair the node's chi^2 is
// formed from), delta integrates out of every node:
//     B~ = -sum_f c_f dd_f (one fma chain),  mu = V B~ (the node's posterior mean of delta),  t' = t + (mu B~) / 2,
// L' = logsumexp t' (the populations mixed by that direction's own weights: loo_mix) and w' = exp(t' - L'):
//     x = {1, p, then per direction  p sum w' mu,  p sum w' mu^2,  p ((L' - L) - log1p(C tau^2) / 2)}        (2 + 3 D columns)
// per (row, star) in a scratch [row][star][2 + 3 D] in the caller's star order; a direction with C = 0 has exact zeros.
// k_chain_accumulate adds the rows in ascending row order, k_off_rows sums a row over the stars in ascending star order.
//
// The full-data sum (ref, S0) adds exactly the terms walk_nodes calls live, in its order: walk_nodes_off visits a SUPERSET of
// walk_nodes' units and forms `live` by the same comparison against the same bound at the same moments, so x[0] and x[1] are
// b9_phot_resid's bits.  Every direction has its own online log-sum-exp (ref', S0', sum e mu, sum e mu^2: lse_step) and its own
// running maximum, which starts from walk_start's seed -- a valid lower bound of max t' because t' >= t -- and follows that
// direction's terms: a node enters direction j's sums while t' > tmax'_j - B9_MARG_CUT.  What a node adds to a direction depends
// on that direction alone, so its columns do not depend on which other directions the call (or the tile) holds.
//
// Box pruning (rigorous, bound (a) of the issue; the dual certificate is not built).  By Cauchy-Schwarz B~^2 <= C sum dd^2, so
// X - 2 g >= (1 - rho) sum dd^2 + nb with rho = C V, and over a box X - 2 g >= (1 - rho) lb + nbmin.  1 - rho = tau^-2 V is formed
// without the cancellation (and shaved by 2^-40, which covers its two roundings).  A chunk or a unit is skipped only when that
// bound excludes it for every direction of the tile and the plain bound excludes it for the full-data cut, in every lane.  At
// real sigmas rho reaches 0.998 and the bound spares next to nothing (docs/LABNOTES.md section 38).  marg_no_pruning: cut2 = inf,
// nothing is dropped.
//
// Direction tiling.  A wave's state is 2 + 4 DT doubles per lane and population for a tile of DT directions; a lane also keeps
// the DT x NFP words c_f.  DT is 1, 2 or 4 (three directions run the four-direction instance with the last one idle); the
// 16-filter instances stop at DT = 2 and tile the directions over gridDim.z.  Tile 0 writes x[0] and x[1]; a tile writes the three
// columns of its own directions only.  Populations one after the other through the one LDS block, as k_star_loo.
// ------------------------------------------------------------------------------------------
#define B9_OFF_MAX_DIR 4
template <int NFP> struct OffTile { static constexpr int DT_MAX = NFP >= 16 ? 2 : 4; };

// the call's directions as the WD-stage kernel takes them (by value): k [direction][filter] (0 past nf), tau^2 and tau^-2
struct OffDirs { double k[B9_OFF_MAX_DIR][B9_MAX_FILT]; double tau2[B9_OFF_MAX_DIR], itau2[B9_OFF_MAX_DIR]; };

// k_offset_stage.  blockIdx.y == 0: c [D][n][nf] in the caller's order (host-formed: k_f / sigma_f where sigma_f > 0, else 0) into
// the mg_* copy's order and layout [D][mg_pad / 64][NFP][64], empty slots and padded filters 0; one lane per (direction, slot,
// filter).  blockIdx.y == 1: one lane per (star, direction) in the caller's order: cv = {C, V} with C = sum_f c_f^2 over f
// ascending and V = 1 / (C + tau^-2); ob = {(tau^-2 V) (1 - 2^-40), log1p(C tau^2) / 2}: the pruning factor and the Occam term.
template <int NFP>
__global__ __launch_bounds__(256) void k_offset_stage(DevStars st, int nf, int D, OffDirs dirs, const double *__restrict__ c_in, double *__restrict__ c_mg,
                                                      double *__restrict__ cv, double *__restrict__ ob)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.y == 0) {
        const long long per = (long long)st.mg_pad * NFP;
        if (i >= per * D) return;
        const int j = (int)(i / per), rem = (int)(i - (long long)j * per);
        const int slot = rem / NFP, f = rem - slot * NFP, orig = st.mg_perm[slot];
        c_mg[(size_t)j * per + B9_SIDX(NFP, f, slot)] = (orig >= 0 && f < nf) ? c_in[((size_t)j * st.n + orig) * nf + f] : 0.0;
        return;
    }
    if (i >= (long long)st.n * D) return;
    const int s = (int)(i / D), j = (int)(i - (long long)s * D);
    const double *__restrict__ const c = c_in + ((size_t)j * st.n + s) * nf;
    double C = 0.0;
    for (int f = 0; f < nf; ++f) C = C + c[f] * c[f];
    const double V = 1.0 / (C + dirs.itau2[j]);
    cv[2 * i] = C; cv[2 * i + 1] = V;
    ob[2 * i] = (dirs.itau2[j] * V) * (1.0 - 0x1p-40); ob[2 * i + 1] = 0.5 * log1p(C * dirs.tau2[j]);
}

// walk_nodes' walk over a superset of its units.  `live` is walk_nodes' own: the same comparison against the same bound, which
// moves at the same moments (a unit walk_nodes skips has no live node and leaves tmax alone).  need(lb, nbm): does any of the
// lane's directions still want a box whose chi^2 is at least lb and whose nb at least nbm; on_node(live, x, row) for every node
// of a unit that is not skipped.
template <int NFP, class N, class F>
__device__ __forceinline__ void walk_nodes_off(b9_ctab t_wp, const MargLayout &L, int n_nodes, int Q, int wave, bool dead, double cut2, double &tmax,
                                               const double (&so)[NFP], const double (&sw)[NFP], N need, F on_node)
{
    const int n_chunks = (n_nodes + 63) >> 6;
    for (int c = 0; c < n_chunks; ++c) {
        double xcut = dead ? NEG_INF : fma(-2.0, tmax, cut2);
        {
            const double lb = box_bound64<NFP>(t_wp + L.o_box1 + (size_t)c * 2 * NFP, so, sw), nbm = t_wp[L.o_nbmin64 + c];
            if (__ballot(lb + nbm < xcut || need(lb, nbm)) == 0ull) continue;
        }
        for (int sub = 0; sub < 4; ++sub) {
            const int u = c * 4 + sub;
            const double nbm = t_wp[L.o_nbmin16 + u];
            for (int j = (wave - 2 * sub) & 3; j < Q; j += 4) {
                const double lb = box_bound64<NFP>(t_wp + L.o_box2 + ((size_t)u * Q + j) * 2 * NFP, so, sw);
                if (__ballot(lb + nbm < xcut || need(lb, nbm)) == 0ull) continue;
                const b9_ctab rowp = t_wp + L.o_rows + ((size_t)u * Q + j) * 16 * NFP;
                for (int i = 0; i < 16; ++i) {
                    const int node = u * 16 + i;
                    const double x = row_x<NFP>(rowp + i * NFP, t_wp[L.o_nb + node], so, sw);
                    const bool live = x < xcut;
                    on_node(live, x, rowp + i * NFP);
                    tmax = max_vv(tmax, live ? -0.5 * x : tmax);
                }
                xcut = dead ? NEG_INF : fma(-2.0, tmax, cut2);
            }
        }
    }
}

// c_mg: k_offset_stage's [D][mg_pad / 64][NFP][64]; cv / ob: its [n][D][2] in the caller's star order
template <int NFP, int NPOPS, int DT>
__global__ __launch_bounds__(256) void k_star_off(DevStars st, int D, const double *__restrict__ c_mg, const double *__restrict__ cv, const double *__restrict__ ob,
                                                  const IsoHdr *__restrict__ hdr, const double *__restrict__ iso_data, long long iso_stride, int mass_cap,
                                                  const double *__restrict__ params, int K, int Q, const double *__restrict__ tab, MargLayout L,
                                                  double cut2, double *__restrict__ scratch)
{
    constexpr int NW = 2 + 4 * DT;                             // a state: {ref, S0, then per direction ref', S0', sum e mu, sum e mu^2}
    extern __shared__ __attribute__((aligned(16))) double s_lds[];
    double (*const s_seed)[4][64] = reinterpret_cast<double (*)[4][64]>(s_lds);                          // [NPOPS][wave][lane]
    double (*const s_state)[NW][64] = reinterpret_cast<double (*)[NW][64]>(s_lds + NPOPS * 4 * 64);      // [wave][word][lane]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sc = blockIdx.x, w = blockIdx.y, d0 = blockIdx.z * DT, ncol = 2 + 3 * D;
    const int slot = sc * 64 + lane, orig = st.mg_perm[slot];
    const bool dead = orig < 0;
    double so[NFP], sw[NFP], cf[DT][NFP], V[DT], omr[DT];
#pragma unroll
    for (int f = 0; f < NFP; ++f) { so[f] = st.mg_so[B9_SIDX(NFP, f, slot)]; sw[f] = st.mg_sw[B9_SIDX(NFP, f, slot)]; }
#pragma unroll
    for (int j = 0; j < DT; ++j) {
        const bool on = !dead && d0 + j < D;                  // (an idle direction: c = 0, so t' = t; it is never written)
        const size_t q = on ? 2 * ((size_t)orig * D + d0 + j) : 0;
#pragma unroll
        for (int f = 0; f < NFP; ++f) cf[j][f] = (d0 + j < D) ? c_mg[(size_t)(d0 + j) * st.mg_pad * NFP + B9_SIDX(NFP, f, slot)] : 0.0;
        V[j] = on ? cv[q + 1] : 0.0;
        omr[j] = on ? ob[q] : 1.0;
    }
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
        double tmf[DT], rf[DT], s0f[DT], s1f[DT], s2f[DT];
#pragma unroll
        for (int j = 0; j < DT; ++j) { tmf[j] = tmax; rf[j] = tmax; s0f[j] = 0.0; s1f[j] = 0.0; s2f[j] = 0.0; }
        walk_nodes_off<NFP>(t_wp, L, (iso[kp].n - 1) * K, Q, wave, dead, cut2, tmax, so, sw, [&](double lb, double nbm) {
            bool any = false;
#pragma unroll
            for (int j = 0; j < DT; ++j) any = any || omr[j] * lb + nbm < fma(-2.0, tmf[j], cut2);
            return !dead && any;
        }, [&](bool live, double x, b9_ctab row) {
            const double t = -0.5 * x;
            if (live) {
                const double e = lse_step(t, ref, [&](double scale) { S0 *= scale; });
                S0 += e;
            }
            double dd[NFP];
#pragma unroll
            for (int f = 0; f < NFP; ++f) dd[f] = fma(sw[f], row[f], -so[f]);
#pragma unroll
            for (int j = 0; j < DT; ++j) {
                double b = 0.0;
#pragma unroll
                for (int f = 0; f < NFP; ++f) b = fma(cf[j][f], dd[f], b);
                const double B = -b, mu = V[j] * B;
                const double tf = fma(0.5 * mu, B, t);
                const bool lf = !dead && tf > tmf[j] - cut;
                if (lf) {
                    const double e = lse_step(tf, rf[j], [&](double scale) { s0f[j] *= scale; s1f[j] *= scale; s2f[j] *= scale; });
                    s0f[j] += e;
                    const double em = e * mu;
                    s1f[j] += em;
                    s2f[j] = fma(em, mu, s2f[j]);
                    tmf[j] = max_vv(tmf[j], tf);
                }
            }
        });
        s_state[wave][0][lane] = ref; s_state[wave][1][lane] = S0;
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            s_state[wave][2 + 4 * j][lane] = rf[j]; s_state[wave][3 + 4 * j][lane] = s0f[j];
            s_state[wave][4 + 4 * j][lane] = s1f[j]; s_state[wave][5 + 4 * j][lane] = s2f[j];
        }
        __syncthreads();

        // ---- wave 0: the four shares merged in wave order, the full-data pair and each direction's group on its own.  A population
        // before the last parks the direction's normalised sums and its log-sum in the output's three columns (a lane reads back
        // only what it wrote itself); the last one mixes them with that direction's own weights
        if (wave == 0 && !dead) {
            const WaveMerge mg = wave_merge(s_state, lane);
            lg[kp] = (mg.S0 > 0.0) ? mg.r + log(mg.S0) : NEG_INF;
            double p = 0.0, wk[NPOPS], A = 0.0;
            bool any = false;
            if (kp == NPOPS - 1) { any = star_finish<NPOPS>(lg, st.mg_c0m[slot], st.mg_la[slot], par, p, wk); A = loo_mix<NPOPS>(lg, par, wk); }
            for (int j = 0; j < DT; ++j) {
                const int jd = d0 + j;
                if (jd >= D) break;
                const WaveMerge mf = wave_merge(reinterpret_cast<const double (*)[NW][64]>(&s_state[0][2 + 4 * j][0]), lane);
                const double lgf = (mf.S0 > 0.0) ? mf.r + log(mf.S0) : NEG_INF;
                const double mn1 = (mf.S0 > 0.0) ? wave_sum(mf, &s_state[0][4 + 4 * j][lane], NW * 64) / mf.S0 : 0.0;
                const double mn2 = (mf.S0 > 0.0) ? wave_sum(mf, &s_state[0][5 + 4 * j][lane], NW * 64) / mf.S0 : 0.0;
                double *const o = out + 2 + 3 * jd;
                if (kp < NPOPS - 1) { o[0] = mn1; o[1] = mn2; o[2] = lgf; continue; }
                double lf[NPOPS], wf[NPOPS];
                lf[NPOPS - 1] = lgf;
                if (NPOPS == 2) lf[0] = o[2];
                const double Af = loo_mix<NPOPS>(lf, par, wf);
                double m1 = wf[NPOPS - 1] * mn1, m2 = wf[NPOPS - 1] * mn2;
                if (NPOPS == 2) { m1 = wf[0] * o[0] + m1; m2 = wf[0] * o[1] + m2; }
                const size_t q = 2 * ((size_t)orig * D + jd);
                const bool has = any && cv[q] > 0.0;                   // C = 0: the direction does not touch this star
                o[0] = has ? p * m1 : 0.0; o[1] = has ? p * m2 : 0.0; o[2] = has ? p * ((Af - A) - ob[q + 1]) : 0.0;
            }
            if (kp == NPOPS - 1 && blockIdx.z == 0) { out[0] = any ? 1.0 : 0.0; out[1] = any ? p : 0.0; }
        }
        if (kp + 1 < NPOPS) __syncthreads();             // the block is the next population's
    }
}

// ------------------------------------------------------------------------------------------
// k_star_off_wd: the WD-stage stars (b9_chain_walk.hip.h), no pruning.  Per lane the full-data pair (mx, S0), then per direction
// ONE lser group {S0', sum mu, sum mu^2} with its own maximum, merged by the wave's shuffle tree; the directions one after the
// other (the steps are walked again per direction: 8 K of them).  Here the quantities come from d_f = pred_f - obs_f and wgt_f:
// B = -sum k_f (wgt_f d_f),  C = sum k_f^2 wgt_f,  V = 1 / (C + tau^-2),  mu = V B,  t' = t + (mu B) / 2.
// ------------------------------------------------------------------------------------------
// what lane 0 needs to finish a WD-stage star's directions
struct OffWdStar { int lane; bool any; double p, A; double *out; };
// direction j (its k, C, V and Occam term) of population KP: the wave's steps, the group's merge, and lane 0's finish -- a
// population before the last parks the direction's normalised sums and its log-sum in the output, as k_star_off does
template <int NFP, int NPOPS, int KP>
__device__ __forceinline__ void off_wd_dir(const WdStar<NFP> &ws, const WdSteps<NFP> &sp, const OffWdStar &fin, const double (&kd)[NFP], double C, double V,
                                           double occ, int j)
{
    double mx = NEG_INF, s[3] = {0.0, 0.0, 0.0};
    if (sp.on) {
        for (int q = 1 + fin.lane; q <= sp.steps; q += 64) {
            const double *__restrict__ const r = sp.rows + (size_t)(q - 1) * NFP;
            double chi2 = 0.0, b = 0.0;
#pragma unroll
            for (int f = 0; f < NFP; ++f) {
                const double d = r[f] - ws.obs[f], wd = ws.wgt[f] * d;
                chi2 = fma(wd, d, chi2);
                b = fma(kd[f], wd, b);
            }
            if (isfinite(chi2)) {
                const double term = (sp.lpm[q - 1] - 0.5 * chi2) + sp.log_w;
                if (term == NEG_INF) continue;
                const double B = -b, mu = V * B, v[3] = {1.0, mu, mu * mu};
                lser_merge<3>(mx, s, fma(0.5 * mu, B, term), v);
            }
        }
    }
    lser_wave<3>(mx, s);
    if (fin.lane == 0) {
        const bool has = mx != NEG_INF && s[0] > 0.0;
        const double lgf = has ? mx + log(s[0]) : NEG_INF;
        const double mn1 = has ? s[1] / s[0] : 0.0, mn2 = has ? s[2] / s[0] : 0.0;
        double *const o = fin.out + 2 + 3 * j;
        if (KP < NPOPS - 1) { o[0] = mn1; o[1] = mn2; o[2] = lgf; }
        else {
            double lf[NPOPS], wf[NPOPS];
            lf[NPOPS - 1] = lgf;
            if (NPOPS == 2) lf[0] = o[2];
            const double Af = loo_mix<NPOPS>(lf, ws.par, wf);
            double m1 = wf[NPOPS - 1] * mn1, m2 = wf[NPOPS - 1] * mn2;
            if (NPOPS == 2) { m1 = wf[0] * o[0] + m1; m2 = wf[0] * o[1] + m2; }
            const bool on = fin.any && C > 0.0;
            o[0] = on ? fin.p * m1 : 0.0; o[1] = on ? fin.p * m2 : 0.0; o[2] = on ? fin.p * ((Af - fin.A) - occ) : 0.0;
        }
    }
}

template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_off_wd(DevStars st, int D, OffDirs dirs, double m_wd_up, const IsoHdr *__restrict__ hdr,
                                                     const double *__restrict__ params, int K, const double *__restrict__ wtab, double *__restrict__ scratch)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k_wd = blockIdx.x * 4 + wave, w = blockIdx.y, n_wp = gridDim.y * NPOPS, ncol = 2 + 3 * D;
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
    const OffWdStar fin{lane, any, p, A, out};
    for (int j = 0; j < D; ++j) {
        double kd[NFP], C = 0.0;
#pragma unroll
        for (int f = 0; f < NFP; ++f) { kd[f] = dirs.k[j][f]; C = fma(kd[f] * kd[f], ws.wgt[f], C); }
        const double V = 1.0 / (C + dirs.itau2[j]), occ = 0.5 * log1p(C * dirs.tau2[j]);
        off_wd_dir<NFP, NPOPS, 0>(ws, wd_steps<NFP>(ws, m_wd_up, hdr, K, wtab, w * NPOPS, n_wp), fin, kd, C, V, occ, j);
        if constexpr (NPOPS == 2) off_wd_dir<NFP, NPOPS, 1>(ws, wd_steps<NFP>(ws, m_wd_up, hdr, K, wtab, w * NPOPS + 1, n_wp), fin, kd, C, V, occ, j);
    }
    if (lane == 0) { out[0] = any ? 1.0 : 0.0; out[1] = any ? p : 0.0; }
}

// k_off_rows: k_loo_rows' pattern.  A row's sums over the stars in ascending (the caller's) order, one plain add each, from the
// scratch values x [n_stars][2 + 3 D] and k_offset_stage's cv = {C, V} [n_stars][D][2] (C = 0: the star is left out of that
// direction's sums):  N += p,  M1 += x[2 + 3j],  M2 += (x[3 + 3j] + p V),  E += x[4 + 3j];  column 0 += p (every star).  One
// workgroup per row, one OWNER lane per output column (4 D + 1), the row's words streamed through LDS in tiles of B9_OFF_TILE
// stars (two buffers: 45 KB of dynamic LDS at four directions).  rows: [n_rows][1 + 4 D].
#define B9_OFF_TILE 128
#define B9_OFF_TILE_LOADS ((B9_OFF_TILE * (2 + 5 * B9_OFF_MAX_DIR) + 255) / 256)      // words of a tile per lane, at most
__global__ __launch_bounds__(256) void k_off_rows(const double *__restrict__ scratch, const double *__restrict__ cv, int n_stars, int D,
                                                  double *__restrict__ rows)
{
    extern __shared__ __attribute__((aligned(16))) double s_tile[];       // two buffers of {x [TILE][ncol], cv [TILE][2 D]}
    const int tid = threadIdx.x, r = blockIdx.x, ncol = 2 + 3 * D, tile_words = B9_OFF_TILE * (ncol + 2 * D);
    const double *__restrict__ const x = scratch + (size_t)r * n_stars * ncol;
    // the owner's column: o = 4 j + q (q: N, M1, M2, E) or 4 D (column 0)
    const int n_owner = 4 * D + 1;
    const bool owner = tid < n_owner, total = tid == 4 * D;
    const int j = total ? 0 : tid / 4, q = tid - 4 * j;
    const int word = (total || q == 0) ? 1 : 1 + 3 * j + q;
    const bool with_v = !total && q == 2;
    double acc = 0.0, v[B9_OFF_TILE_LOADS];
    auto fetch = [&](int s0) {                          // tile [s0, s0 + tn) -> registers: the x words, then the cv words
        const int tn = min(B9_OFF_TILE, n_stars - s0), nx = tn * ncol, ns = tn * 2 * D;
        const double *__restrict__ const xb = x + (size_t)s0 * ncol, *__restrict__ const sb = cv + (size_t)s0 * 2 * D;
#pragma unroll
        for (int k = 0; k < B9_OFF_TILE_LOADS; ++k) {
            if (k * 256 < nx + ns) {                    // (wave-uniform)
                const int w = tid + k * 256;
                const double *ptr = w < nx ? xb + w : sb + min(w - nx, ns - 1);
                v[k] = *ptr;
            }
        }
    };
    auto stash = [&](int s0, double *buf) {             // registers -> LDS: x at 0, cv at TILE * ncol
        const int tn = min(B9_OFF_TILE, n_stars - s0), nx = tn * ncol, ns = tn * 2 * D;
#pragma unroll
        for (int k = 0; k < B9_OFF_TILE_LOADS; ++k) {
            const int w = tid + k * 256;
            if (k * 256 < nx + ns && w < nx + ns) buf[w < nx ? w : B9_OFF_TILE * ncol + (w - nx)] = v[k];
        }
    };
    if (n_stars > 0) { fetch(0); stash(0, s_tile); }
    __syncthreads();
    for (int s0 = 0, t = 0; s0 < n_stars; s0 += B9_OFF_TILE, ++t) {
        const double *cur = s_tile + (size_t)(t & 1) * tile_words;
        double *nxt = s_tile + (size_t)((t + 1) & 1) * tile_words;
        const bool more = s0 + B9_OFF_TILE < n_stars;
        if (more) fetch(s0 + B9_OFF_TILE);
        if (owner) {
            const int tn = min(B9_OFF_TILE, n_stars - s0);
            const double *xs = cur, *cs = cur + B9_OFF_TILE * ncol + 2 * j;
            for (int k = 0; k < tn; ++k) {              // one star, in order: the only chain is acc
                const double p = xs[k * ncol + 1], xv = xs[k * ncol + word], C = cs[k * 2 * D], Vv = cs[k * 2 * D + 1];
                const double val = with_v ? xv + p * Vv : xv;
                acc = (total || C > 0.0) ? acc + val : acc;
            }
        }
        if (more) stash(s0 + B9_OFF_TILE, nxt);
        __syncthreads();
    }
    if (owner) rows[(size_t)r * n_owner + (total ? 0 : 1 + tid)] = acc;
}
