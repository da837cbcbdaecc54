// b9_pointwise.hip.h -- b9_pointwise (the modelScore counterpart): k_star_lpd (MS/RGB-stage stars, one LANE per star),
// k_star_lpd_wd (WD-stage stars, one WAVE per star), k_pw_accumulate (the per-star state), k_pw_tail (the per-star largest
// values of -v), k_pw_transpose / k_pw_fill (the tail between the caller's layout and the device's; its -inf start) and k_pw_rows
// (a row's sum over the stars).
// Part of the single translation unit b9_kernels.hip (included there, after b9_phot_resid.hip.h); gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------
// Pointwise predictive densities over a chain ("Pointwise predictive densities").  The grid, the node terms
// t_(k, n) and the pruning are b9_star_moments'; where that call forms conditional expectations under the node weights, these
// kernels keep only the star's marginal log-likelihood v = finish_star().v = logaddexp(la, l) -- the value b9_logpost reports per
// star in marginalised mode -- one double per (row, star) in a scratch [row][star] in the caller's star order.  A star with no
// live node has v = la, the field term (-inf at membership prior 1).  A row outside the grid writes no value: it is flagged in
// row_in[row] (1 inside, 0 outside), so no value of v has a second meaning.  The reducers then walk the scratch in a fixed
// order: k_pw_accumulate the rows of a star ascending, k_pw_rows the stars of a row ascending; k_pw_tail keeps a function of
// the multiset of a star's values.  No random numbers, no atomics.
//
// k_star_lpd: k_star_moments' frame -- grid (64-star chunk of the mg_* copy, row) x 256, the walk and the pruning of
// b9_chain_walk.hip.h, the merge through LDS in wave order by wave 0 -- with a lane's state cut down to the log-sum-exp pair
// (ref, S0) per population: no weighted sums, no marg_primary call in the row loop.
// ------------------------------------------------------------------------------------------

// one more term t = -X / 2: lse_step's scheme on S0 alone, written out: at a jump of the reference fma(s0, f, 1.0) rounds once
// where lse_step's rescale-then-add rounds twice
__device__ __forceinline__ void lpd_term(double t, double &ref, double &s0)
{
    const double d = t - ref;
    if (__ballot(d > 600.0) != 0ull) {
        const bool up = d > 600.0;
        const double f = exp_marg(max_vs(up ? -d : d, -700.0));
        s0 = up ? fma(s0, f, 1.0) : s0 + f;
        ref = up ? t : ref;
    } else {
        s0 += exp_marg(max_vs(d, -700.0));
    }
}

template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_lpd(DevStars st, const IsoHdr *__restrict__ hdr, const double *__restrict__ iso_data,
                                                  long long iso_stride, int mass_cap, const double *__restrict__ params, int K, int Q,
                                                  const double *__restrict__ tab, MargLayout L, double cut2, double *__restrict__ scratch,
                                                  int *__restrict__ row_in)
{
    __shared__ double s_seed[NPOPS][4][64];
    __shared__ double s_state[NPOPS][4][2][64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sc = blockIdx.x, w = blockIdx.y;
    const int slot = sc * 64 + lane, orig = st.mg_perm[slot];
    const bool dead = orig < 0;
    double so[NFP], sw[NFP];
#pragma unroll
    for (int f = 0; f < NFP; ++f) { so[f] = st.mg_so[B9_SIDX(NFP, f, slot)]; sw[f] = st.mg_sw[B9_SIDX(NFP, f, slot)]; }
    const double *par = params + (size_t)w * B9_NPARAM;
    IsoView<NFP> iso[NPOPS];
    double tip_min;
    const bool valid = load_iso_views<NFP, NPOPS>(hdr, iso_data, iso_stride, mass_cap, w, iso, tip_min);
    if (sc == 0 && threadIdx.x == 0) row_in[w] = valid ? 1 : 0;
    if (!valid) return;                                  // a row outside the grid: flagged, no value written

#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp)
        s_seed[kp][wave][lane] = walk_seed<NFP>((b9_ctab)(tab + (size_t)(w * NPOPS + kp) * L.total), L, (iso[kp].n - 1) * K, Q, wave, so, sw);
    __syncthreads();

#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        const b9_ctab t_wp = (b9_ctab)(tab + (size_t)(w * NPOPS + kp) * L.total);
        double tmax = walk_start(s_seed[kp], lane);
        double ref = tmax, s0 = 0.0;
        walk_nodes<NFP>(t_wp, L, (iso[kp].n - 1) * K, Q, wave, dead, cut2, tmax, so, sw, [&](bool live, double x, int, int, b9_ctab) {
            if (live) lpd_term(-0.5 * x, ref, s0);
        });
        s_state[kp][wave][0][lane] = ref;
        s_state[kp][wave][1][lane] = s0;
    }
    __syncthreads();
    if (wave != 0 || dead) return;

    // ---- wave 0: the four shares merged in wave order, the star finished
    const double c0m = st.mg_c0m[slot];
    double ll[NPOPS];
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        const WaveMerge m = wave_merge(s_state[kp], lane);
        ll[kp] = (m.S0 > 0.0) ? c0m + (m.r + log(m.S0)) : NEG_INF;
    }
    scratch[(size_t)w * st.n + orig] = finish_star<NPOPS>(ll, par, st.mg_la[slot]).v;
}

// ------------------------------------------------------------------------------------------
// k_star_lpd_wd: the WD-stage stars (b9_chain_walk.hip.h) with a per-lane online log-sum-exp pair, merged by the wave's shuffle
// tree (a fixed order).
// ------------------------------------------------------------------------------------------
template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_lpd_wd(DevStars st, double m_wd_up, const IsoHdr *__restrict__ hdr, const double *__restrict__ params,
                                                     int K, const double *__restrict__ wtab, double *__restrict__ scratch)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k_wd = blockIdx.x * 4 + wave, w = blockIdx.y, n_wp = gridDim.y * NPOPS;
    if (k_wd >= st.n_wd) return;
    const WdStar<NFP> ws = wd_star<NFP, NPOPS>(st, hdr, params, k_wd, w);
    if (!ws.valid) return;                               // (k_star_lpd has flagged the row)
    const double c0m = st.c0m[ws.slot];
    double ll[NPOPS];
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        const WdSteps<NFP> sp = wd_steps<NFP>(ws, m_wd_up, hdr, K, wtab, w * NPOPS + kp, n_wp);
        Lse acc; acc.mx = NEG_INF; acc.sm = 0.0;
        if (sp.on) {
            for (int j = 1 + lane; j <= sp.steps; j += 64) {
                const double *__restrict__ const r = sp.rows + (size_t)(j - 1) * NFP;
                double chi2 = 0.0;
#pragma unroll
                for (int f = 0; f < NFP; ++f) { const double d = r[f] - ws.obs[f]; chi2 = fma(ws.wgt[f] * d, d, chi2); }
                if (isfinite(chi2)) lse_add(acc, (sp.lpm[j - 1] - 0.5 * chi2) + sp.log_w);
            }
        }
        acc = lse_wave(acc);
        ll[kp] = (acc.mx == NEG_INF) ? NEG_INF : c0m + (acc.mx + log(acc.sm));
    }
    if (lane == 0) scratch[(size_t)w * st.n + ws.orig] = finish_star<NPOPS>(ll, ws.par, st.la[ws.slot]).v;
}

// ------------------------------------------------------------------------------------------
// k_pw_accumulate: one lane per star: the chunk's rows in ascending order through the recurrence of DESIGN.md section 2 on the
// star's eight words, held in registers.  A lane's row values are independent loads, all issued before the dependent chain
// (B9_PW_MAX_ROWS of them, the loops unrolled so that v[] stays in registers).  Contractions only where the statement writes an
// fma; one exp, the library's.
// ------------------------------------------------------------------------------------------
// (B9_PW_MAX_ROWS: b9_launch.h)

// the online log-sum-exp half of the recurrence: (mx, s) takes the value x; k = 0 is handled by the caller
__device__ __forceinline__ void pw_lse(double x, double &mx, double &s)
{
#pragma clang fp contract(off)
    if (x > mx) { s = __builtin_fma(s, exp(mx - x), 1.0); mx = x; }
    else s = s + exp(x - mx);
}

__global__ __launch_bounds__(256) void k_pw_accumulate(const double *__restrict__ scratch, const int *__restrict__ row_in, int n_rows, int n_stars,
                                                       double *__restrict__ acc)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_stars) return;
    double v[B9_PW_MAX_ROWS];
#pragma unroll
    for (int r = 0; r < B9_PW_MAX_ROWS; ++r) v[r] = (r < n_rows && row_in[r]) ? scratch[(size_t)r * n_stars + i] : 0.0;
    double *__restrict__ const a = acc + (size_t)i * B9_PW_N;
    double rows = a[B9_PW_ROWS], ninf = a[B9_PW_NINF], vmax = a[B9_PW_VMAX], spos = a[B9_PW_SPOS], rmax = a[B9_PW_RMAX], sneg = a[B9_PW_SNEG],
           mean = a[B9_PW_MEAN], m2 = a[B9_PW_M2];
#pragma unroll
    for (int r = 0; r < B9_PW_MAX_ROWS; ++r) {
        if (r >= n_rows || !row_in[r]) continue;
        const double x = v[r], k = rows - ninf;          // k: the finite rows taken so far
        rows = rows + 1.0;
        if (x == NEG_INF) { ninf = ninf + 1.0; continue; }
        if (k == 0.0) {
            vmax = x; spos = 1.0; rmax = -x; sneg = 1.0; mean = x; m2 = 0.0;
        } else {
            pw_lse(x, vmax, spos);
            pw_lse(-x, rmax, sneg);
            const double d = x - mean;
            mean = mean + d / (k + 1.0);
            m2 = __builtin_fma(d, x - mean, m2);
        }
    }
    a[B9_PW_ROWS] = rows; a[B9_PW_NINF] = ninf; a[B9_PW_VMAX] = vmax; a[B9_PW_SPOS] = spos; a[B9_PW_RMAX] = rmax; a[B9_PW_SNEG] = sneg;
    a[B9_PW_MEAN] = mean; a[B9_PW_M2] = m2;
}

// ------------------------------------------------------------------------------------------
// k_pw_tail: one lane per star, one wave per workgroup: the tail_len largest values of r = -v among the star's finite rows,
// descending, padded with -inf.  The device copy is [tail_len][n_stars]: a wave's lanes touch neighbouring words at every depth.
// The wave's 64 lists are worked in LDS, [tail_len][64] (dynamic, 128 KB at tail_len = 256: opted in through with_lds; a lane's
// words lie 64 apart, so a wave's accesses at one depth are conflict-free, and the lists are indexed in memory, never as a
// register array): read in coalesced, written back coalesced.  A new value is first tested against the star's smallest kept
// one, held in a register; only a larger one is inserted, by a walk from the bottom that moves the smaller entries down one
// place.  (The same walk on the global copy, every step a dependent round trip to memory: 0.27 ms a chunk of 32 rows at 20k
// stars and tail_len 49 against 0.57 ms for k_star_lpd; docs/LABNOTES.md section 24.)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_pw_tail(const double *__restrict__ scratch, const int *__restrict__ row_in, int n_rows, int n_stars,
                                                int tail_len, double *__restrict__ tail)
{
    extern __shared__ __attribute__((aligned(16))) double pw_lists[];            // [tail_len][64]
    const int lane = threadIdx.x, i = blockIdx.x * 64 + lane;
    const bool on = i < n_stars;
    double v[B9_PW_MAX_ROWS];
#pragma unroll
    for (int r = 0; r < B9_PW_MAX_ROWS; ++r) v[r] = (on && r < n_rows && row_in[r]) ? scratch[(size_t)r * n_stars + i] : NEG_INF;
    double *const t = pw_lists + lane;
    for (int j = 0; j < tail_len; ++j) t[j * 64] = on ? tail[(size_t)j * n_stars + i] : NEG_INF;
    double low = t[(tail_len - 1) * 64];
#pragma unroll
    for (int r = 0; r < B9_PW_MAX_ROWS; ++r) {
        const double x = -v[r];                          // (+inf for a row that does not take part)
        if (!(x < __builtin_inf()) || !(x > low)) continue;
        int j = tail_len - 1;
        while (j > 0) {
            const double up = t[(j - 1) * 64];
            if (!(up < x)) break;
            t[j * 64] = up;
            --j;
        }
        t[j * 64] = x;
        low = t[(tail_len - 1) * 64];
    }
    if (on)
        for (int j = 0; j < tail_len; ++j) tail[(size_t)j * n_stars + i] = t[j * 64];
}

// k_pw_transpose: out[c][r] = in[r][c] for in [n_r][n_c]: the tail between the caller's [n_stars][tail_len] and the device's
// [tail_len][n_stars].  One lane per word of `out` (coalesced stores).
__global__ __launch_bounds__(256) void k_pw_transpose(const double *__restrict__ in, int n_r, int n_c, double *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n_r * n_c) return;
    const int c = (int)(i / n_r), r = (int)(i - (long long)c * n_r);
    out[i] = in[(size_t)r * n_c + c];
}

// k_pw_fill: n words set to x (the tail's -inf start)
__global__ __launch_bounds__(256) void k_pw_fill(double *__restrict__ p, long long n, double x)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = x;
}

// ------------------------------------------------------------------------------------------
// k_pw_rows: one WAVE per row: the row's values summed over the stars in ascending (the caller's) order, one plain add each.
// k_hist_rows' one lane per row walks its row alone -- 64 loads in flight, every one a line of its own to the lane: 0.67 ms per
// chunk at 50k stars, the latency of 780 batches (docs/LABNOTES.md section 24).  Here the wave reads the row coalesced, lane l
// the words s + l + 64 u of a batch of 64 B9_PW_ROWS_UNROLL stars, and the adds stay ONE chain in star order: every word goes
// through a scalar register pair (v_readlane) into the same accumulator.  -inf propagates through the adds; a row outside the
// grid gives -inf from its flag.
// ------------------------------------------------------------------------------------------
#define B9_PW_ROWS_UNROLL 8

__device__ __forceinline__ double pw_lane(double v, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

__global__ __launch_bounds__(64) void k_pw_rows(const double *__restrict__ scratch, const int *__restrict__ row_in, int n_stars,
                                                double *__restrict__ rows)
{
    const int r = blockIdx.x, lane = threadIdx.x;
    if (!row_in[r]) { if (lane == 0) rows[r] = NEG_INF; return; }
    const double *__restrict__ const x = scratch + (size_t)r * n_stars;
    double a = 0.0;
    int s = 0;
    for (; s + 64 * B9_PW_ROWS_UNROLL <= n_stars; s += 64 * B9_PW_ROWS_UNROLL) {
        double v[B9_PW_ROWS_UNROLL];
#pragma unroll
        for (int u = 0; u < B9_PW_ROWS_UNROLL; ++u) v[u] = x[s + 64 * u + lane];
#pragma unroll
        for (int u = 0; u < B9_PW_ROWS_UNROLL; ++u) {
#pragma unroll
            for (int l = 0; l < 64; ++l) a = a + pw_lane(v[u], l);
        }
    }
    for (; s < n_stars; s += 64) {                       // the last, partial batch: 64 stars at a time, the very last ones counted
        const int m = min(64, n_stars - s);
        const double v = lane < m ? x[s + lane] : 0.0;
        for (int l = 0; l < m; ++l) a = a + pw_lane(v, l);
    }
    if (lane == 0) rows[r] = a;
}
