// b9_phot_resid.hip.h -- b9_phot_resid (the photResiduals counterpart): k_resid_stage (the call's pivots in the mg_* order),
// k_star_resid (MS/RGB-stage stars, one LANE per star), k_star_resid_wd (WD-stage stars, one WAVE per star) and k_resid_rows (a
// row's sums over the stars).  Part of the single translation unit b9_kernels.hip (included there, after b9_mass_hist.hip.h);
// gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------
// Exact posterior-predictive residuals over a chain ("Posterior-predictive residuals").  The grid, the node
// terms t_(k, n), the weights w = exp(t - logsumexp t) and the membership p are b9_star_moments'; where that call keeps the
// moments of the node's masses, these kernels keep the moments of the node's MAGNITUDES about a per-star pivot c_f (the caller's
// obs_f where sigma_f > 0, else 0):  d_f = pred_f - c_f, one rounded subtraction of the node table's row word, and
//     x = {1, p, p sum w d_0, p sum w d_0^2, ..., p sum w d_(nf-1), p sum w d_(nf-1)^2}          (2 + 2 nf columns)
// per (row, star) in a scratch [row][star][2 + 2 nf] in the caller's star order; k_chain_accumulate adds the rows to the per-star
// accumulators in ascending row order and k_resid_rows sums a row over the stars in ascending star order, one plain add each:
// the same bits for any chunking.  No random numbers, no atomics.
//
// k_star_resid: grid (64-star chunk of the mg_* copy, row) x 256, the walk and the pruning of b9_chain_walk.hip.h.  Per population
// a lane keeps an online log-sum-exp reference, S0 and 2 NFP weighted sums in registers (lse_step: the rare jump of the
// reference rescales all of them).  Which terms enter, and how the reference moves, depends on the terms alone.
//
// LDS.  A population's four wave states are [4][2 + 2 NFP][64] doubles: 68 KB at 16 filters, so two populations' states do not
// fit a static block.  Of the two possible forms (a population at a time through one reused block; filters tiled across
// gridDim.z as k_star_hist tiles bins) this file takes the FIRST: the populations are worked one after the other, each merged
// by wave 0 in wave order 0..3 out of the one block before the next overwrites it; a population before the last parks its
// normalised sums in the output (a lane reads back only what it wrote itself).  Tiling the filters would evaluate every term's
// exp once per tile.  All LDS is dynamic ([seeds][states]: 72 KB at 16 filters, 40 KB at 8, 24 KB at 4 with two populations).
// It never bounds the occupancy: the registers do (docs/LABNOTES.md section 23: 256 VGPRs + 27 AGPRs at 16 filters, one
// workgroup per CU; 146 at 8 filters, three).  A column [c][64] is a bank per lane pair: conflict-free.
// ------------------------------------------------------------------------------------------

// k_resid_stage: the pivots [n][nf] in the caller's order (host-formed: obs where sigma > 0, else 0) into the mg_* copy's order
// and layout [mg_pad / 64][NFP][64]; empty slots and padded filters 0.  One lane per (slot, filter).
template <int NFP>
__global__ __launch_bounds__(256) void k_resid_stage(DevStars st, int nf, const double *__restrict__ piv_in, double *__restrict__ piv_mg)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= st.mg_pad * NFP) return;
    const int slot = i / NFP, f = i - slot * NFP, orig = st.mg_perm[slot];
    piv_mg[B9_SIDX(NFP, f, slot)] = (orig >= 0 && f < nf) ? piv_in[(size_t)orig * nf + f] : 0.0;
}

// one more term t = -X / 2 of a node whose row (NFP magnitudes) is wave-uniform.
// s: {S0, then per filter the sums weighted by d and d^2}
template <int NFP>
__device__ __forceinline__ void resid_term(double t, b9_ctab row, const double (&piv)[NFP], double &ref, double (&s)[1 + 2 * NFP])
{
    const double e = lse_step(t, ref, [&](double scale) {
#pragma unroll
        for (int c = 0; c < 1 + 2 * NFP; ++c) s[c] *= scale;
    });
    s[0] += e;
#pragma unroll
    for (int f = 0; f < NFP; ++f) {
        const double d = row[f] - piv[f], ed = e * d;
        s[1 + 2 * f] += ed;
        s[2 + 2 * f] = fma(ed, d, s[2 + 2 * f]);
    }
}

template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_resid(DevStars st, int nf, const double *__restrict__ piv_mg, const IsoHdr *__restrict__ hdr,
                                                    const double *__restrict__ iso_data, long long iso_stride, int mass_cap,
                                                    const double *__restrict__ params, int K, int Q, const double *__restrict__ tab, MargLayout L,
                                                    double cut2, double *__restrict__ scratch)
{
    constexpr int NS = 1 + 2 * NFP;                       // a lane's sums; a state is the reference and these
    extern __shared__ __attribute__((aligned(16))) double s_lds[];
    double (*const s_seed)[4][64] = reinterpret_cast<double (*)[4][64]>(s_lds);                          // [NPOPS][wave][lane]
    double (*const s_state)[1 + NS][64] = reinterpret_cast<double (*)[1 + NS][64]>(s_lds + NPOPS * 4 * 64);   // [wave][word][lane]
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int sc = blockIdx.x, w = blockIdx.y, ncol = 2 + 2 * nf;
    const int slot = sc * 64 + lane, orig = st.mg_perm[slot];
    const bool dead = orig < 0;
    double so[NFP], sw[NFP], piv[NFP];
#pragma unroll
    for (int f = 0; f < NFP; ++f) {
        so[f] = st.mg_so[B9_SIDX(NFP, f, slot)]; sw[f] = st.mg_sw[B9_SIDX(NFP, f, slot)]; piv[f] = piv_mg[B9_SIDX(NFP, f, slot)];
    }
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

#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp)
        s_seed[kp][wave][lane] = walk_seed<NFP>((b9_ctab)(tab + (size_t)(w * NPOPS + kp) * L.total), L, (iso[kp].n - 1) * K, Q, wave, so, sw);
    __syncthreads();

    double lg[NPOPS];
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        const b9_ctab t_wp = (b9_ctab)(tab + (size_t)(w * NPOPS + kp) * L.total);
        double tmax = walk_start(s_seed[kp], lane);
        double ref = tmax, s[NS];
#pragma unroll
        for (int c = 0; c < NS; ++c) s[c] = 0.0;
        walk_nodes<NFP>(t_wp, L, (iso[kp].n - 1) * K, Q, wave, dead, cut2, tmax, so, sw, [&](bool live, double x, int, int, b9_ctab row) {
            if (live) resid_term<NFP>(-0.5 * x, row, piv, ref, s);
        });
        s_state[wave][0][lane] = ref;
#pragma unroll
        for (int c = 0; c < NS; ++c) s_state[wave][1 + c][lane] = s[c];
        __syncthreads();

        // ---- wave 0: the four shares merged in wave order.  A population before the last parks its normalised sums in the
        // output's columns 2.. (a lane reads back only what it wrote itself); the last one mixes them with star_finish's weights
        if (wave == 0 && !dead) {
            const WaveMerge mg = wave_merge(s_state, lane);
            lg[kp] = (mg.S0 > 0.0) ? mg.r + log(mg.S0) : NEG_INF;
            double p = 0.0, wk[NPOPS];
            bool any = false;
            if (kp == NPOPS - 1) any = star_finish<NPOPS>(lg, st.mg_c0m[slot], st.mg_la[slot], par, p, wk);
            for (int c = 0; c < 2 * nf; ++c) {
                const double mn = (mg.S0 > 0.0) ? wave_sum(mg, &s_state[0][2 + c][lane], (1 + NS) * 64) / mg.S0 : 0.0;
                if (kp < NPOPS - 1) { out[2 + c] = mn; continue; }
                double m = wk[NPOPS - 1] * mn;
                if (NPOPS == 2) m = wk[0] * out[2 + c] + m;
                out[2 + c] = any ? p * m : 0.0;
            }
            if (kp == NPOPS - 1) { out[0] = any ? 1.0 : 0.0; out[1] = any ? p : 0.0; }
        }
        if (kp + 1 < NPOPS) __syncthreads();             // the block is the next population's
    }
}

// ------------------------------------------------------------------------------------------
// k_star_resid_wd: the WD-stage stars (b9_chain_walk.hip.h).  Per lane an online log-sum-exp with S0 and the 2 NFP weighted sums;
// the lanes' states are merged by the wave's shuffle tree (a fixed order).  The pivot is the slot-order copy's obs word: the
// caller's bits where sigma > 0, 0 for an unused filter.
// ------------------------------------------------------------------------------------------
template <int NFP, int NPOPS>
__global__ __launch_bounds__(256) void k_star_resid_wd(DevStars st, int nf, double m_wd_up, const IsoHdr *__restrict__ hdr,
                                                       const double *__restrict__ params, int K, const double *__restrict__ wtab,
                                                       double *__restrict__ scratch)
{
    constexpr int NS = 1 + 2 * NFP;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int k_wd = blockIdx.x * 4 + wave, w = blockIdx.y, n_wp = gridDim.y * NPOPS, ncol = 2 + 2 * nf;
    if (k_wd >= st.n_wd) return;
    const WdStar<NFP> ws = wd_star<NFP, NPOPS>(st, hdr, params, k_wd, w);
    double *__restrict__ const out = scratch + ((size_t)w * st.n + ws.orig) * ncol;
    if (!ws.valid) {
        for (int c = lane; c < ncol; c += 64) out[c] = 0.0;
        return;
    }
    // (lane 0 finishes the star; a population before the last parks its normalised sums in the output, as k_star_resid does)
    double lg[NPOPS], s[NS];
#pragma unroll
    for (int kp = 0; kp < NPOPS; ++kp) {
        const WdSteps<NFP> sp = wd_steps<NFP>(ws, m_wd_up, hdr, K, wtab, w * NPOPS + kp, n_wp);
        double mx = NEG_INF;
#pragma unroll
        for (int c = 0; c < NS; ++c) s[c] = 0.0;
        if (sp.on) {
            for (int j = 1 + lane; j <= sp.steps; j += 64) {
                const double *__restrict__ const r = sp.rows + (size_t)(j - 1) * NFP;
                double d[NFP], chi2 = 0.0;
#pragma unroll
                for (int f = 0; f < NFP; ++f) { d[f] = r[f] - ws.obs[f]; chi2 = fma(ws.wgt[f] * d[f], d[f], chi2); }
                if (isfinite(chi2)) {
                    const double term = (sp.lpm[j - 1] - 0.5 * chi2) + sp.log_w;
                    if (term == NEG_INF) continue;
                    double b[NS];
                    b[0] = 1.0;
#pragma unroll
                    for (int f = 0; f < NFP; ++f) { b[1 + 2 * f] = d[f]; b[2 + 2 * f] = d[f] * d[f]; }
                    lser_merge<NS>(mx, s, term, b);
                }
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            double b[NS];
            const double bmx = __shfl_down(mx, o, 64);
#pragma unroll
            for (int c = 0; c < NS; ++c) b[c] = __shfl_down(s[c], o, 64);
            lser_merge<NS>(mx, s, bmx, b);
        }
        const bool has = mx != NEG_INF && s[0] > 0.0;
        lg[kp] = has ? mx + log(s[0]) : NEG_INF;
#pragma unroll
        for (int c = 0; c < 2 * NFP; ++c) s[1 + c] = has ? s[1 + c] / s[0] : 0.0;
        if (kp < NPOPS - 1 && lane == 0) {
#pragma unroll
            for (int c = 0; c < 2 * NFP; ++c)
                if (c < 2 * nf) out[2 + c] = s[1 + c];
        }
    }
    if (lane != 0) return;
    double p, wk[NPOPS];
    const bool any = star_finish<NPOPS>(lg, st.c0m[ws.slot], st.la[ws.slot], ws.par, p, wk);
#pragma unroll
    for (int c = 0; c < 2 * NFP; ++c)
        if (c < 2 * nf) {
            double m = wk[NPOPS - 1] * s[1 + c];
            if (NPOPS == 2) m = wk[0] * out[2 + c] + m;
            out[2 + c] = any ? p * m : 0.0;
        }
    out[0] = any ? 1.0 : 0.0; out[1] = any ? p : 0.0;
}

// k_resid_rows: a row's sums over the stars in ascending (the caller's) order, one plain add each, formed from the scratch values
// x and s = 1 / sigma (isig [n_stars][nf], the caller's order, 0 = filter unused: the star is left out of that filter's sums):
//     N += p,  R += -(x[2 + 2f] s),  C += (x[3 + 2f] s) s,  W += (p s) s,  D += -((x[2 + 2f] s) s);   column 0 += p (every star).
// One workgroup per row; one OWNER lane per output column (5 nf + 1 of them: a (filter, sum) pair each, and column 0), so a
// column is one chain of n_stars adds in star order.  A row's increments [n_stars][2 + 2 nf] and the 1 / sigma table are both
// contiguous in star order: all 256 lanes stream them through LDS in tiles of B9_RESID_TILE stars with coalesced loads, the next
// tile's words in registers while the owners add from the current one (two LDS buffers, one barrier a tile).  The literal form
// -- one lane per (row, filter) walking global memory with 16 stars' loads in flight -- has four waves a chunk and waits for
// memory 1250 times a row: 26 ms of a 36 ms call at 20k stars, this form 14 ms of 24.5 (docs/LABNOTES.md section 23).  rows: [n_rows][1 + 5 nf].
#define B9_RESID_TILE 128
#define B9_RESID_AHEAD 16
#define B9_RESID_TILE_LOADS ((B9_RESID_TILE * (2 + 3 * B9_MAX_FILT) + 255) / 256)      // words of a tile per lane, at most
__global__ __launch_bounds__(256) void k_resid_rows(const double *__restrict__ scratch, const double *__restrict__ isig, int n_stars, int nf,
                                                    double *__restrict__ rows)
{
    extern __shared__ __attribute__((aligned(16))) double s_tile[];       // two buffers of {x [TILE][ncol], s [TILE][nf]}
    const int tid = threadIdx.x, r = blockIdx.x, ncol = 2 + 2 * nf, tile_words = B9_RESID_TILE * (ncol + nf);
    const double *__restrict__ const x = scratch + (size_t)r * n_stars * ncol;
    // the owner's column: o = 5 f + q (q: N, R, C, W, D) or 5 nf (column 0)
    const int n_owner = 5 * nf + 1;
    const bool owner = tid < n_owner, total = tid == 5 * nf;
    const int f = total ? 0 : tid / 5, q = tid - 5 * f;
    const int word = (total || q == 0 || q == 3) ? 1 : (q == 1 || q == 4) ? 2 + 2 * f : 3 + 2 * f;
    const bool plain = total || q == 0, twice = q >= 2, neg = q == 1 || q == 4;
    double acc = 0.0, v[B9_RESID_TILE_LOADS];
    // (branch-free per lane: one unconditional load from a clamped address, so the tile's loads are all in flight together;
    // left as per-lane branches the compiler waits for each load before it issues the next: 1.44 ms a dispatch instead of 1.20)
    auto fetch = [&](int s0) {                          // tile [s0, s0 + tn) -> registers: the x words, then the s words
        const int tn = min(B9_RESID_TILE, n_stars - s0), nx = tn * ncol, ns = tn * nf;
        const double *__restrict__ const xb = x + (size_t)s0 * ncol, *__restrict__ const sb = isig + (size_t)s0 * nf;
#pragma unroll
        for (int k = 0; k < B9_RESID_TILE_LOADS; ++k) {
            if (k * 256 < nx + ns) {                    // (wave-uniform)
                const int w = tid + k * 256;
                const double *ptr = w < nx ? xb + w : sb + min(w - nx, ns - 1);
                v[k] = *ptr;
            }
        }
    };
    auto stash = [&](int s0, double *buf) {             // registers -> LDS: x at 0, s at TILE * ncol
        const int tn = min(B9_RESID_TILE, n_stars - s0), nx = tn * ncol, ns = tn * nf;
#pragma unroll
        for (int k = 0; k < B9_RESID_TILE_LOADS; ++k) {
            const int w = tid + k * 256;
            if (k * 256 < nx + ns && w < nx + ns) buf[w < nx ? w : B9_RESID_TILE * ncol + (w - nx)] = v[k];
        }
    };
    if (n_stars > 0) { fetch(0); stash(0, s_tile); }
    __syncthreads();
    for (int s0 = 0, t = 0; s0 < n_stars; s0 += B9_RESID_TILE, ++t) {
        const double *cur = s_tile + (size_t)(t & 1) * tile_words;
        double *nxt = s_tile + (size_t)((t + 1) & 1) * tile_words;
        const bool more = s0 + B9_RESID_TILE < n_stars;
        if (more) fetch(s0 + B9_RESID_TILE);
        if (owner) {
            const int tn = min(B9_RESID_TILE, n_stars - s0);
            const double *xw = cur + word, *sw = cur + B9_RESID_TILE * ncol + f;
            auto add = [&](double p, double s) {         // one star, in order: the only chain is acc
                const double a = p * s, b = a * s;
                double val = plain ? p : (twice ? b : a);
                val = neg ? -val : val;
                acc = s > 0.0 ? acc + val : acc;
            };
            // B9_RESID_AHEAD stars' LDS words are read before the adds that consume them, so the chain does not wait for an LDS
            // round trip per star (measured: not what bounds the kernel -- docs/LABNOTES.md section 23)
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
        if (more) stash(s0 + B9_RESID_TILE, nxt);
        __syncthreads();
    }
    if (owner) rows[(size_t)r * n_owner + (total ? 0 : 1 + tid)] = acc;
}
