// b9_chain_walk.hip.h -- what the four reductions over a saved chain share (b9_star_moments, b9_mass_hist, b9_phot_resid,
// b9_pointwise): the pruned walk over the MS/RGB node table, the online log-sum-exp step, the merge of the four waves' shares,
// the star's membership and population weights, the WD-stage stars' steps, and the accumulation of a chunk's rows.  Each is
// stated here ONCE: the four calls must agree in these to the bit (tests/test_gpu_chain_ties.py, test_ties_to_star_moments).
// Part of the single translation unit b9_kernels.hip (included there, after b9_star_marg.hip.h); gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------
// The walk.  A workgroup's four waves hold the SAME 64 stars, one per lane, and take the units (16 nodes x one mass ratio) of
// every 64-node chunk by k_star_marg's diagonal rule -- unit (sub, j) is wave (2 sub + j) mod 4's: a function of the layout only.
// A unit's words are wave-uniform and reach the lanes as scalar loads through b9_ctab.
//
// Pruning (rigorous, a function of the data only): every wave starts from the SAME lower bound of the star's largest term --
// the best term among every 16th node at mass ratio 0, the four waves' shares merged behind a barrier (walk_seed, walk_start)
// -- and from there on follows its own running maximum; a term counts while it lies within B9_MARG_CUT e-folds of that bound,
// and a chunk / a unit whose box (k_marg_table's fp64 boxes) excludes that for every lane is skipped.  What is dropped is below
// N_nodes e^-40 of the star's sum.  No field floor: the weights are conditional on membership.
// ------------------------------------------------------------------------------------------

// the seed pass of one population: this wave's share of every 16th node at mass ratio 0, as a term.  The kernel stores it to its
// seeds [NPOPS][wave][lane] and places the barrier (a form that takes the LDS block and all populations costs the two-population
// instances up to 32 VGPRs and an occupancy step: docs/LABNOTES.md section 25)
template <int NFP>
__device__ __forceinline__ double walk_seed(b9_ctab t_wp, const MargLayout &L, int n_nodes, int Q, int wave, const double (&so)[NFP], const double (&sw)[NFP])
{
    const int n_units = ((n_nodes + 63) >> 6) * 4;
    double xmin = __builtin_inf();
    for (int u = wave; u < n_units; u += 4)
        xmin = __builtin_fmin(xmin, row_x<NFP>(t_wp + L.o_rows + (size_t)u * Q * 16 * NFP, t_wp[L.o_nb + u * 16], so, sw));
    return -0.5 * xmin;
}
// the lower bound every wave starts from (a population's seeds [wave][lane]): the lane's running maximum and first reference
__device__ __forceinline__ double walk_start(const double (*seed)[64], int lane)
{
    return __builtin_fmax(__builtin_fmax(seed[0][lane], seed[1][lane]), __builtin_fmax(seed[2][lane], seed[3][lane]));
}

// One population's pruned walk for this wave.  on_node(live, x, node, j, row) is called for every node (mass ratio j / Q, its
// NFP magnitudes at row) that is live for SOME lane of the wave -- for all 64 lanes, so that it may do wave-uniform work; the
// lane's own term t = -x / 2 counts only where `live`.  tmax: in, walk_start's bound; it follows the lane's live terms.
template <int NFP, class F>
__device__ __forceinline__ void walk_nodes(b9_ctab t_wp, const MargLayout &L, int n_nodes, int Q, int wave, bool dead, double cut2, double &tmax,
                                           const double (&so)[NFP], const double (&sw)[NFP], F on_node)
{
    const int n_chunks = (n_nodes + 63) >> 6;
    for (int c = 0; c < n_chunks; ++c) {
        double xcut = dead ? NEG_INF : fma(-2.0, tmax, cut2);                 // a term counts while X < xcut
        if (__ballot(box_bound64<NFP>(t_wp + L.o_box1 + (size_t)c * 2 * NFP, so, sw) + t_wp[L.o_nbmin64 + c] < xcut) == 0ull) continue;
        for (int sub = 0; sub < 4; ++sub) {
            const int u = c * 4 + sub;
            const double nbm = t_wp[L.o_nbmin16 + u];
            for (int j = (wave - 2 * sub) & 3; j < Q; j += 4) {
                if (__ballot(box_bound64<NFP>(t_wp + L.o_box2 + ((size_t)u * Q + j) * 2 * NFP, so, sw) + nbm < xcut) == 0ull) continue;
                const b9_ctab rowp = t_wp + L.o_rows + ((size_t)u * Q + j) * 16 * NFP;
                for (int i = 0; i < 16; ++i) {
                    const int node = u * 16 + i;
                    const double x = row_x<NFP>(rowp + i * NFP, t_wp[L.o_nb + node], so, sw);
                    const bool live = x < xcut;
                    if (__ballot(live) == 0ull) continue;
                    on_node(live, x, node, j, rowp + i * NFP);
                    tmax = max_vv(tmax, live ? -0.5 * x : tmax);          // (a select, not a second `if (live)`: that one costs the row loop four instructions)
                }
                xcut = dead ? NEG_INF : fma(-2.0, tmax, cut2);
            }
        }
    }
}

// One more term t of an online log-sum-exp whose reference stays while terms lie within 600 e-folds above it (lse_term's scheme):
// returns e = e^(t - ref), which the caller adds to S0 and, weighted, to its other sums.  The rare jump of the reference calls
// rescale(f) first: every sum is multiplied by f (1.0 in the lanes that did not jump).
template <class R>
__device__ __forceinline__ double lse_step(double t, double &ref, R rescale)
{
    const double d = t - ref;
    if (__ballot(d > 600.0) != 0ull) {
        const bool up = d > 600.0;
        const double f = exp_marg(max_vs(up ? -d : d, -700.0));
        rescale(up ? f : 1.0);
        ref = up ? t : ref;
        return up ? 1.0 : f;
    }
    return exp_marg(max_vs(d, -700.0));
}

// The four waves' shares (ref, S0) of a lane -- words 0 and 1 of state [wave][NW words][64] -- merged in wave order 0..3.  A share
// counts (on[k]) only if its S0 > 0: r the largest such reference, f[k] = e^(ref_k - r) (0 for a share that does not count),
// S0 = sum f[k] S0_k.  Any further word is merged the same way (wave_sum).  log sum = r + log(S0) where S0 > 0, else no live node.
struct WaveMerge { double r, S0, f[4]; bool on[4]; };
template <int NW>
__device__ __forceinline__ WaveMerge wave_merge(const double (*state)[NW][64], int lane)
{
    WaveMerge m;
    m.r = NEG_INF; m.S0 = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { m.on[k] = state[k][1][lane] > 0.0; m.r = (m.on[k] && state[k][0][lane] > m.r) ? state[k][0][lane] : m.r; }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        m.f[k] = m.on[k] ? exp_fast(state[k][0][lane] - m.r) : 0.0;
        if (m.on[k]) m.S0 += state[k][1][lane] * m.f[k];
    }
    return m;
}
// ... and another of the lane's sums: x [wave] at a stride of `stride` doubles
__device__ __forceinline__ double wave_sum(const WaveMerge &m, const double *x, size_t stride)
{
    double S = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (m.on[k]) S += x[k * stride] * m.f[k];
    return S;
}

// The membership p and the populations' weights wk of a star from its per-population log-sums lg[k] = log sum_n e^(t_(k, n)) (the
// star's constant c0m NOT included; -inf: no live node).  The membership is finish_star's l and v, as b9_sample_mass forms it;
// the weights e^(log lambda_k + lg_k) / sum do not need c0m (0 for a population without a live node).  false: no live node in
// any population -- the (row, star) contributes nothing.
template <int NPOPS>
__device__ __forceinline__ bool star_finish(const double (&lg)[NPOPS], double c0m, double la, const double *par, double &p, double (&wk)[NPOPS])
{
    double a[NPOPS], ll[NPOPS];
    bool any = false;
#pragma unroll
    for (int k = 0; k < NPOPS; ++k) {
        a[k] = lg[k];
        if (NPOPS == 2) { const double lam = par[B9_P_LAMBDA]; a[k] = (lg[k] == NEG_INF) ? NEG_INF : (k ? log1p(-lam) : log(lam)) + lg[k]; }
        ll[k] = (lg[k] == NEG_INF) ? NEG_INF : c0m + lg[k];
        any = any || a[k] != NEG_INF;
        wk[k] = 0.0;
    }
    p = 0.0;
    if (!any) return false;
    const StarFinish fin = finish_star<NPOPS>(ll, par, la);
    p = (fin.l == NEG_INF) ? 0.0 : exp(fin.l - fin.v);
    wk[0] = 1.0;
    if (NPOPS == 2) {
        const double A = logaddexp(a[0], a[NPOPS - 1]);
#pragma unroll
        for (int k = 0; k < NPOPS; ++k) wk[k] = (a[k] == NEG_INF) ? 0.0 : exp(a[k] - A);
    }
    return true;
}

// ------------------------------------------------------------------------------------------
// The WD-stage stars, one wavefront per (row, star) as in k_star_marg_wd, grid (ceil(n_wd / 4), rows) x 256: lanes stride over the
// 8 K steps m_j = tip + dM j (j = 1 .. 8 K) of k_marg_wd_table's rows (the star's own wd_type), mass ratio 0.
// ------------------------------------------------------------------------------------------
template <int NFP>
struct WdStar {                      // WD-stage star k_wd (< st.n_wd) under row w
    int slot, orig, wd_type;
    bool valid;                      // the row lies inside the grid
    const double *par;
    double obs[NFP], wgt[NFP];
};
template <int NFP, int NPOPS>
__device__ __forceinline__ WdStar<NFP> wd_star(const DevStars &st, const IsoHdr *__restrict__ hdr, const double *__restrict__ params, int k_wd, int w)
{
    WdStar<NFP> s;
    s.slot = st.wd_slot[k_wd]; s.orig = st.perm[s.slot];
#pragma unroll
    for (int f = 0; f < NFP; ++f) { s.obs[f] = st.obs[B9_SIDX(NFP, f, s.slot)]; s.wgt[f] = st.w[B9_SIDX(NFP, f, s.slot)]; }
    s.wd_type = st.flags[s.slot] & 1;
    s.par = params + (size_t)w * B9_NPARAM;
    s.valid = true;
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) s.valid = s.valid && hdr[w * NPOPS + kp].valid;
    return s;
}

template <int NFP>
struct WdSteps {                     // the steps of (row, population) wp of n_wp for a star
    double tip, dM, log_w;
    int steps;
    bool on;                         // dM > 0: the population has WD-stage steps at all
    const double *__restrict__ rows, *__restrict__ lpm;      // k_marg_wd_table's
    __device__ __forceinline__ double m1(int j) const { return tip + dM * j; }
    // step j's term (log prior - chi^2 / 2) + log dM; -inf: the step does not take part.  (k_star_lpd_wd and k_star_resid_wd
    // write this loop body out over the same members: through term() they lose an occupancy step at 8 and 4 filters)
    __device__ __forceinline__ double term(const WdStar<NFP> &s, int j) const
    {
        if (!on || j > steps) return NEG_INF;
        const double *__restrict__ const r = rows + (size_t)(j - 1) * NFP;
        double chi2 = 0.0;
#pragma unroll
        for (int f = 0; f < NFP; ++f) { const double d = r[f] - s.obs[f]; chi2 = fma(s.wgt[f] * d, d, chi2); }
        return isfinite(chi2) ? (lpm[j - 1] - 0.5 * chi2) + log_w : NEG_INF;
    }
};
template <int NFP>
__device__ __forceinline__ WdSteps<NFP> wd_steps(const WdStar<NFP> &s, double m_wd_up, const IsoHdr *__restrict__ hdr, int K,
                                                 const double *__restrict__ wtab, int wp, int n_wp)
{
    WdSteps<NFP> p;
    p.steps = 8 * K;
    p.tip = hdr[wp].agb_tip; p.dM = (m_wd_up - p.tip) / p.steps;
    p.on = p.dM > 0.0;
    p.log_w = p.on ? log(p.dM) : 0.0;
    p.rows = wtab + (((size_t)wp * 2 + s.wd_type) * p.steps) * NFP;
    p.lpm = wtab + (size_t)n_wp * 2 * p.steps * NFP + (size_t)wp * p.steps;
    return p;
}

// an online log-sum-exp with NS sums (mx, s) takes another one's (the lanes' states through the wave's shuffle tree: a fixed order)
template <int NS>
__device__ __forceinline__ void lser_merge(double &amx, double (&as)[NS], double bmx, const double (&bs)[NS])
{
    if (bmx == NEG_INF) return;
    if (amx == NEG_INF) {
        amx = bmx;
#pragma unroll
        for (int c = 0; c < NS; ++c) as[c] = bs[c];
        return;
    }
    const bool a_hi = amx >= bmx;
    const double f = exp_fast(a_hi ? bmx - amx : amx - bmx);
    const double fa = a_hi ? 1.0 : f, fb = a_hi ? f : 1.0;
    amx = a_hi ? amx : bmx;
#pragma unroll
    for (int c = 0; c < NS; ++c) as[c] = as[c] * fa + bs[c] * fb;
}
template <int NS>
__device__ __forceinline__ void lser_wave(double &mx, double (&s)[NS])
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        double b[NS];
        const double bmx = __shfl_down(mx, o, 64);
#pragma unroll
        for (int c = 0; c < NS; ++c) b[c] = __shfl_down(s[c], o, 64);
        lser_merge<NS>(mx, s, bmx, b);
    }
}
// ... and the plain pair's (Lse, b9_star_marg.hip.h)
__device__ __forceinline__ Lse lse_wave(Lse acc)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Lse b; b.mx = __shfl_down(acc.mx, o, 64); b.sm = __shfl_down(acc.sm, o, 64);
        acc = lse_merge(acc, b);
    }
    return acc;
}

// k_chain_accumulate: one lane per (star, column): acc += x_r for the chunk's rows r in ascending order, one plain add each
__global__ __launch_bounds__(256) void k_chain_accumulate(const double *__restrict__ scratch, int n_rows, long long n_words, double *__restrict__ acc)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_words) return;
    double a = acc[i];
    for (int r = 0; r < n_rows; ++r) a = a + scratch[(size_t)r * n_words + i];
    acc[i] = a;
}
