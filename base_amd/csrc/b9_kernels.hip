// b9_kernels.hip -- hand-written gfx950 kernels of the BASE-9 per-step log-posterior path.
//
//   k_derive_iso   SURVEY 8a rows a3, a8  one workgroup per (walker, population, slice of EEPs): grid
//                                     brackets by wave ballot, EEP-range intersection, EEP-wise
//                                     tri-linear interpolation (one value per thread).  In the
//                                     device-resident sampler it first FINISHES the previous step
//                                     (fixed-order sum of partials + prior + Metropolis accept,
//                                     recomputed identically by every workgroup of the walker) and
//                                     draws the new proposal (Philox4x32-10 + Box-Muller)
//   k_star_like    rows a4-a7, a9      given-mass mode, the dominant kernel.  HOT workgroups: one
//                                     LANE per star -- 8-ary search in the LDS-staged mass column,
//                                     magnitude rows from L2, binary flux combination, Gaussian
//                                     chi^2, population mixture, product-form field-star mixture,
//                                     one partial per wave.  HEAVY workgroups (first in the grid):
//                                     the stars above the AGB tip (IFMR -> WD cooling -> WD
//                                     atmosphere, or NS/BH) through the general per-star code
//   k_star_marg    row a6 (marg.)      marginalised mode: ONE WAVEFRONT PER STAR integrating over
//                                     primary mass and mass ratio, rigorous pruning, online
//                                     log-sum-exp, wavefront-shuffle merge
//   k_mcmc_step    rows a4-a9, 8f-1    the fused sampler step, ONE launch per MCMC step (given-mass mode):
//                                     accept/reject of step t-1 (redundantly per wave), k_star_like's
//                                     roles on step t's proposal, and both candidate isochrone sets
//                                     of step t+1 on extra workgroups
//   k_finalize     row a8              fixed-order sum of the partials + cluster prior (+ the accept
//                                     of a two-launch sampler block's last step)
//   k_predict_mags rows a4-a7, a9      b9_predict_mags: the forward model alone (no observations) --
//                                     one lane per system, predicted apparent magnitudes + stage
//   k_wd_node_table / k_wd_sample      b9_sample_wd_mass: the WD chain once per node of the call's own grid with its
//                                     derived values kept, then one lane per WD-stage star against the table
//   k_chain_accumulate               the four reductions over a saved chain below: their shared node walk, star finish and WD
//                                     steps (b9_chain_walk.hip.h), and the per-star accumulation of a chunk's rows
//   k_wd_node_table_status / k_wd_moments   b9_wd_moments: exact per-WD posterior moments of the ZAMS mass and the five derived
//                                     values over b9_sample_wd_mass's grid (one lane per WD-stage star), summed over the rows
//   k_star_moments / _wd              b9_star_moments: exact per-star posterior moments over the marginalisation
//                                     grid (one lane per star, four waves sharing the node table), summed over the rows
//   k_star_hist / _wd / k_hist_rows   b9_mass_hist: exact binned mass posteriors over the same grid (a
//                                     per-wave LDS histogram per lane, bins worked in tiles), summed over the rows and the stars
//   k_star_ratio / _wd                b9_ratio_hist: the joint table (primary-mass bin x mass-ratio node) of the same weights
//                                     (k_star_hist's frame, a tile holds whole mass bins), summed over the rows and the stars
//   k_star_bins / _wd                b9_star_bins: the same bins on every star's OWN edges with the two open ends kept (the
//                                     bin is per lane, the edges staged in LDS), summed over the rows
//   k_wd_bins                        b9_wd_bins: b9_wd_moments' node weights binned on every (WD-stage star, quantity)'s OWN
//                                     edges, one selected quantity per blockIdx.z, summed over the rows
//   k_band_points / k_band_wd_points / k_band_accumulate   b9_cmd_band: the MS/RGB loci and WD sequences a saved chain's rows imply
//                                     (one lane per point into a chunk's value table), reduced over the rows one lane per line
//   k_star_loo / _wd / k_loo_rows       b9_filter_loo: exact leave-one-filter-out predictions and densities (b9_filter_loo.hip.h)
//   k_star_off / _wd / k_offset_stage / k_off_rows   b9_star_offset: exact per-star reddening / distance offsets (b9_star_offset.hip.h)
//   k_star_resid / _wd / k_resid_stage / k_resid_rows   b9_phot_resid: exact posterior-predictive magnitude
//                                     moments per filter over the same grid, summed over the rows and, standardised, the stars
//   k_star_lpd / _wd / k_pw_accumulate / k_pw_tail / k_pw_rows   b9_pointwise: every star's marginal log-likelihood per row over
//                                     the same grid, reduced over the rows (online log-sum-exps, Welford, largest -v) and the stars
//   k_infl_accumulate / k_infl_groups   b9_star_influence: the same values as leave-one-star-out weights of the caller's per-row
//                                     quantities (one lane per star, quantities tiled), and summed over the stars of each group
//
// The kernels live in the *.hip.h files included below (one translation unit); this file holds
// k_finalize and the host-callable launch wrappers.
//
// The reference source is not mounted (/root/reference/README.md:4), so none of this can
// cite a reference file:line; DESIGN.md "Math" is the normative restatement and
// oracle/b9_oracle.c the CPU checker.  Floating-point contract: built with
// -ffp-contract=off; every interpolation is an explicit fma(t, b - a, a), which makes the
// derived isochrone bit-identical to the oracle's.
//
// No MFMA anywhere: there is no dense contraction on this path (BASELINE.json north_star).
// Diagnostic-only macros (never defined in the shipped library): B9_STAMPS (per-phase s_memtime
// stamps), B9_ABL_* (ablation builds used for the attribution in docs/LABNOTES.md section 8).
#include "b9_device.h"
#include "b9_launch.h"
#include "b9_devbuf.h"
#include <algorithm>
#include <cstring>
#include "../../include/base9_hip.h"

#include "b9_diag.hip.h"
#include "b9_common.hip.h"
#include "b9_derive.hip.h"
#include "b9_star.hip.h"
#include "b9_star_like.hip.h"
#include "b9_mcmc_step.hip.h"
#define B9_TREE_KD B9_TREE_KD_SMALL
namespace tree_kd3 {
#include "b9_mcmc_tree.hip.h"
}
#undef B9_TREE_KD
#undef B9_TREE_KV
#define B9_TREE_KD B9_TREE_KD_LARGE
namespace tree_kd5 {
#include "b9_mcmc_tree.hip.h"
}
#undef B9_TREE_KD
#include "b9_star_marg.hip.h"
#include "b9_marg_step.hip.h"
#include "b9_predict.hip.h"
#include "b9_chain_walk.hip.h"
#include "b9_wd_sample.hip.h"
#include "b9_star_moments.hip.h"
#include "b9_wd_moments.hip.h"
#include "b9_mass_hist.hip.h"
#include "b9_ratio_hist.hip.h"
#include "b9_star_bins.hip.h"
#include "b9_wd_bins.hip.h"
#include "b9_phot_resid.hip.h"
#include "b9_filter_loo.hip.h"
#include "b9_star_offset.hip.h"
#include "b9_pointwise.hip.h"
#include "b9_star_influence.hip.h"
#include "b9_cmd_band.hip.h"

// ------------------------------------------------------------------------------------------
// k_finalize: one workgroup per walker: fixed-order sum of the partials + prior -> logpost[w]
// (SURVEY 8a row a8); -inf for a walker outside the grid; with mc.enabled also the accept/reject
// of the block's last step.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_finalize(const IsoHdr *__restrict__ hdr, const double *__restrict__ partial,
                                                   int n_partial, long long partial_stride, int n_pops,
                                                   const double *__restrict__ params, DevPriors pr,
                                                   double *__restrict__ logpost, double *__restrict__ perstar,
                                                   int n_stars, McmcDev mc, unsigned long long *__restrict__ done_flag, unsigned long long done_seq)
{
    __shared__ double s_red[4], s_cur[B9_NPARAM], s_lp;
    const int w = blockIdx.x, tid = threadIdx.x;
    const double *row = params + (size_t)w * B9_NPARAM;
    bool in_support;
    const double lp = finish_logpost(hdr, partial + (size_t)w * partial_stride, n_partial, row, pr, n_pops, w, s_red, &in_support);
    if (tid == 0) {
        logpost[w] = lp;
        // b9_logpost's completion word (mapped host memory, behind the value it announces): the host polls it instead of
        // waiting for the stream's completion signal
        if (done_flag) { __threadfence_system(); __hip_atomic_store(done_flag + w, done_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
    }
    // a walker inside the grid whose prior is -inf still has per-star values from the star kernel;
    // the oracle reports -inf for them as well
    if (perstar && !in_support)
        for (int i = tid; i < n_stars; i += 256) perstar[(size_t)w * n_stars + i] = NEG_INF;
    if (mc.enabled) metropolis_accept(mc, w, mc.step, mc.row, row, lp, true, s_cur, &s_lp);
}

// ------------------------------------------------------------------------------------------
// launch wrappers
// ------------------------------------------------------------------------------------------
#include <type_traits>

// Opt a kernel in to `lds` bytes of dynamic LDS: above 64 KB a launch needs the attribute, above the CU's 160 KB nothing helps.
template <class K>
static hipError_t lds_opt_in(K *kern, size_t lds)
{
    if (lds > B9_LDS_PER_CU) return hipErrorInvalidValue;
    if (lds <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

// a kernel, its dynamic LDS, and what opting in to that said: derived once for an occupancy query and for the launch
template <class K> struct LdsKernel { K *kern; size_t lds; hipError_t err; };
template <class K> static LdsKernel<K> with_lds(K *kern, size_t lds) { return {kern, lds, lds_opt_in(kern, lds)}; }

// Runtime (pk.nfp, n_pops) -> the instantiated <NFP, NPOPS> of {4, 8, 16} x {1, 2}: f gets them as integral constants.
template <int N> using Int = std::integral_constant<int, N>;
template <class F>
static hipError_t dispatch_nfp(int nfp, F &&f)
{
    switch (nfp) {
    case 4:  return f(Int<4>{});
    case 8:  return f(Int<8>{});
    case 16: return f(Int<16>{});
    default: return hipErrorInvalidValue;
    }
}
template <class F>
static hipError_t dispatch(int nfp, int n_pops, F &&f)
{
    return dispatch_nfp(nfp, [&](auto nfp_c) { return n_pops == 2 ? f(nfp_c, Int<2>{}) : f(nfp_c, Int<1>{}); });
}

hipError_t b9k_derive_iso(const DevPack &pk, const B9IsoSet &set, int n_walkers, const McmcDev &mc, const DevPriors &pr, const B9Prev &prev,
                          hipStream_t stream)
{
    const int gy = (set.mass_cap * (pk.nfp + 1) + 255) / 256;
    hipLaunchKernelGGL(k_derive_iso, dim3(n_walkers * set.n_pops, gy), dim3(256), 0, stream,
                       pk, set.params, set.n_pops, set.hdr, set.iso, set.iso_stride, set.mass_cap, mc, pr,
                       prev.partial.ptr, prev.partial.n, prev.partial.stride, prev.set.hdr, prev.set.params);
    return hipGetLastError();
}

hipError_t b9k_derive_iso_rows(const DevPack &pk, const double *host_rows, const B9IsoSet &set, int n_walkers, hipStream_t stream)
{
    if (n_walkers < 1 || n_walkers > 8) return hipErrorInvalidValue;
    HostRows rows{};
    std::memcpy(rows.v, host_rows, sizeof(double) * B9_NPARAM * n_walkers);
    const int gy = (set.mass_cap * (pk.nfp + 1) + 255) / 256;
    hipLaunchKernelGGL(k_derive_iso_rows, dim3(n_walkers * set.n_pops, gy), dim3(256), 0, stream,
                       pk, rows, set.params, set.n_pops, set.hdr, set.iso, set.iso_stride, set.mass_cap);
    return hipGetLastError();
}

// LDS of the heavy-star role: the WD axes (the cooling tracks' concatenated age axes only while they fit
// B9_WC_AGE_LDS_MAX doubles; longer ones are searched in L2) + per (candidate, population) the four AGB-tip columns
// and the mass column + each candidate's parameter row
static size_t heavy_lds_doubles(const DevPack &pk, int n_pops, int n_cand, int mass_cap)
{
    // [8 words of reduction scratch][the packed axes, DevPack::heavy_const][AGB tips: the whole table, or the corner columns]
    // [mass columns][parameter rows][find_bracket's over-read]
    const size_t n_tips = (size_t)pk.n_feh * pk.n_y * pk.n_age;
    const size_t tips = n_tips <= B9_TIPS_LDS_MAX ? n_tips : (size_t)4 * n_pops * n_cand * pk.n_age;
    return 8 + (size_t)pk.hc_len + tips + (size_t)n_pops * n_cand * mass_cap + (size_t)n_cand * B9_NPARAM + 8;
}

// dynamic LDS, bytes, of the kernels that evaluate ONE candidate per walker (k_star_like, k_mcmc_tree): the hot role's mass
// columns (+ 8: find_bracket's last stage may read up to 6 entries past a column's end, masked out) or the heavy role's axes
static size_t one_candidate_lds(const DevPack &pk, int n_pops, int mass_cap)
{
    return sizeof(double) * std::max((size_t)n_pops * mass_cap + 8, heavy_lds_doubles(pk, n_pops, 1, mass_cap));
}

hipError_t b9k_star_like(const DevPack &pk, const DevStars &st, const B9IsoSet &set, int n_walkers, const B9Partial &partial, double *perstar,
                         const B9Groups &gr, int heavy_parts, hipStream_t stream)
{
    return dispatch(pk.nfp, set.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        const auto k = with_lds(k_star_like<NFP, NPOPS>, one_candidate_lds(pk, NPOPS, set.mass_cap));
        if (k.err != hipSuccess) return k.err;
        const int hot = 8 * ((gr.n_blocks * NPOPS + 7) / 8) * n_walkers;     // padded so every XCD sees whole walker sets (two populations: a workgroup per half tile)
        const int heavy = (n_walkers * heavy_parts + 7) / 8 * 8;     // heavy-star workgroups lead the grid
        hipLaunchKernelGGL(k.kern, dim3(heavy + hot), dim3(256), k.lds, stream, pk, st, set.hdr, set.iso,
                           set.iso_stride, set.mass_cap, set.params, n_walkers, partial.ptr, partial.stride, gr.n_groups, gr.group_tiles,
                           gr.groups_per_block, gr.n_blocks, perstar, heavy, heavy_parts);
        return hipGetLastError();
    });
}

hipError_t b9k_finalize(const B9IsoSet &set, const B9Partial &partial, const DevPriors &pr, int n_walkers, double *d_logpost, double *perstar,
                        int n_stars, const McmcDev &mc, hipStream_t stream, unsigned long long *done_flag, unsigned long long done_seq)
{
    hipLaunchKernelGGL(k_finalize, dim3(n_walkers), dim3(256), 0, stream, set.hdr, partial.ptr, partial.n, partial.stride,
                       set.n_pops, set.params, pr, d_logpost, perstar, n_stars, mc, done_flag, done_seq);
    return hipGetLastError();
}

size_t b9k_predict_lds(int nfp, int mass_cap, int n_pops) { return sizeof(double) * (size_t)n_pops * mass_cap * (nfp + 1); }

hipError_t b9k_predict_mags(const DevPack &pk, const B9IsoSet &set, long long n, const double *mass1, const double *mass_ratio, const int *wd_type,
                            const int *pop, double *out_mags, int *out_stage, int n_wgs, hipStream_t stream)
{
    return dispatch_nfp(pk.nfp, [&](auto nfp_c) {
        constexpr int NFP = decltype(nfp_c)::value;
        const auto k = with_lds(k_predict_mags<NFP>, b9k_predict_lds(NFP, set.mass_cap, set.n_pops));
        if (k.err != hipSuccess) return k.err;
        const long long need = (n + 255) / 256;
        hipLaunchKernelGGL(k.kern, dim3((unsigned)std::max(1ll, std::min<long long>(need, n_wgs))), dim3(256), k.lds, stream, pk, set.hdr, set.iso,
                           set.iso_stride, set.mass_cap, set.n_pops, set.params, n, mass1, mass_ratio, wd_type, pop, out_mags, out_stage);
        return hipGetLastError();
    });
}

// acc [n_words] += the n_rows rows of scratch [n_rows][n_words], ascending: the last launch of every reduction over a chunk of rows
static void launch_chain_accumulate(const double *scratch, int n_rows, long long n_words, double *acc, hipStream_t stream)
{
    hipLaunchKernelGGL(k_chain_accumulate, dim3((unsigned)((n_words + 255) / 256)), dim3(256), 0, stream, scratch, n_rows, n_words, acc);
}

// ---- the WD-grid calls (b9_sample_wd_mass, b9_wd_moments, b9_wd_bins): the node table of a chunk of rows, then the call's star kernel ----
long long b9k_wd_grid_table_doubles(int nfp, long long n_nodes, bool status)       // per (row, population)
{
    return n_nodes * (status ? B9_WDM_NODE_DOUBLES(nfp) : B9_WDS_NODE_DOUBLES(nfp));
}

// The chunk's node table (STATUS: with every node's status behind it) behind the guard the three calls share.  Returns
// n_wp = n_rows * NPOPS, or 0: invalid arguments, nothing launched.
template <int NFP, int NPOPS, bool STATUS>
static int launch_wd_grid_table(const DevPack &pk, const DevStars &st, const B9WdGrid &g, int n_rows, hipStream_t stream)
{
    if (!g.tab || n_rows < 1 || g.n_nodes < 1 || st.n_wd < 1 || n_rows * NPOPS > 65535) return 0;
    const int n_wp = n_rows * NPOPS;
    hipLaunchKernelGGL(STATUS ? k_wd_node_table_status<NFP> : k_wd_node_table<NFP>, dim3((g.n_nodes + 63) / 64, n_wp), dim3(128), 0, stream, pk, g.set.hdr, g.set.iso,
                       g.set.iso_stride, g.set.mass_cap, NPOPS, g.set.params, g.n_nodes, g.tab, n_wp);
    return n_wp;
}

hipError_t b9k_wd_sample(const DevPack &pk, const DevStars &st, const B9WdGrid &g, int n_rows, const B9WdSample &smp, hipStream_t stream)
{
    return dispatch(pk.nfp, g.set.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        const int n_wp = launch_wd_grid_table<NFP, NPOPS, false>(pk, st, g, n_rows, stream);
        if (!n_wp) return hipErrorInvalidValue;
        WdSampleOut out{};
        out.zams = smp.zams; out.member = smp.member; out.pop = smp.pop; out.wd_rank = g.rank;
        out.der[0] = smp.wd_mass; out.der[1] = smp.prec_log_age; out.der[2] = smp.log_cool_age; out.der[3] = smp.log_teff; out.der[4] = smp.logg;
        out.k0 = smp.k0; out.k1 = smp.k1; out.row0 = smp.row0;
        hipLaunchKernelGGL((k_wd_sample<NFP, NPOPS>), dim3((st.n_wd + 63) / 64, n_rows), dim3(64), 0, stream, pk, st, g.set.hdr, g.set.params, g.n_nodes,
                           g.tab, n_wp, out);
        return hipGetLastError();
    });
}

hipError_t b9k_wd_moments(const DevPack &pk, const DevStars &st, const B9WdGrid &g, int n_rows, hipStream_t stream)
{
    return dispatch(pk.nfp, g.set.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        if (!g.rank || !g.scratch || !g.acc) return hipErrorInvalidValue;
        const int n_wp = launch_wd_grid_table<NFP, NPOPS, true>(pk, st, g, n_rows, stream);
        if (!n_wp) return hipErrorInvalidValue;
        hipLaunchKernelGGL((k_wd_moments<NFP, NPOPS>), dim3((st.n_wd + 63) / 64, n_rows), dim3(64), 0, stream, pk, st, g.set.hdr, g.set.params, g.n_nodes,
                           g.tab, n_wp, g.rank, g.scratch);
        launch_chain_accumulate(g.scratch, n_rows, (long long)st.n_wd * B9_WDM_N, g.acc, stream);
        return hipGetLastError();
    });
}

hipError_t b9k_wd_bins(const DevPack &pk, const DevStars &st, const B9WdGrid &g, int n_rows, int quantity_mask, int n_bins, hipStream_t stream)
{
    return dispatch(pk.nfp, g.set.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        const int n_sel = __builtin_popcount((unsigned)quantity_mask);
        if (!g.rank || !g.edges || !g.scratch || !g.acc || n_bins < 1 || n_bins > B9_WBIN_MAX_BINS || quantity_mask < 1 || quantity_mask >= (1 << B9_WQ_N))
            return hipErrorInvalidValue;
        const int n_wp = launch_wd_grid_table<NFP, NPOPS, true>(pk, st, g, n_rows, stream);
        if (!n_wp) return hipErrorInvalidValue;
        const auto k = with_lds(k_wd_bins<NFP, NPOPS>, sizeof(double) * 64 * ((size_t)(n_bins + 1) + (size_t)(n_bins + 2)));
        if (k.err != hipSuccess) return k.err;
        hipLaunchKernelGGL(k.kern, dim3((st.n_wd + 63) / 64, n_rows, n_sel), dim3(64), k.lds, stream, pk, st, g.set.hdr, g.set.params, g.n_nodes,
                           g.tab, n_wp, g.rank, quantity_mask, n_sel, g.edges, n_bins, g.scratch);
        launch_chain_accumulate(g.scratch, n_rows, (long long)st.n_wd * n_sel * (n_bins + 3), g.acc, stream);
        return hipGetLastError();
    });
}

// ---- b9_cmd_band: the chunk's WD node table (b9_wd_moments' kernel, as it is), the points' values, the accumulation over the rows ----
hipError_t b9k_cmd_band(const DevPack &pk, const B9Band &b, int n_rows, hipStream_t stream)
{
    return dispatch_nfp(pk.nfp, [&](auto nfp_c) {
        constexpr int NFP = decltype(nfp_c)::value;
        const B9IsoSet &s = b.set;
        const B9BandSpec &sp = b.spec;
        const int n_wp = n_rows * s.n_pops, n_ms = sp.n_ratio * sp.n_eep, n_wd = sp.n_types * sp.n_wd_nodes;
        if (!b.values || !b.pivot || (!b.mom && !b.bins) || n_rows < 1 || n_wp > 65535 || sp.n_lines < 1 || (n_wd > 0 && !b.wd_tab) ||
            (b.bins && (!b.edges_t || b.n_bins < 1 || b.n_bins > B9_BAND_MAX_BINS)))
            return hipErrorInvalidValue;
        if (n_ms > 0)
            hipLaunchKernelGGL(k_band_points<NFP>, dim3((n_ms + 255) / 256, n_wp), dim3(256), 0, stream, pk, s.hdr, s.iso, s.iso_stride, s.mass_cap, s.n_pops,
                               s.params, sp, b.values);
        if (n_wd > 0) {
            hipLaunchKernelGGL(k_wd_node_table_status<NFP>, dim3((sp.n_wd_nodes + 63) / 64, n_wp), dim3(128), 0, stream, pk, s.hdr, s.iso, s.iso_stride,
                               s.mass_cap, s.n_pops, s.params, sp.n_wd_nodes, b.wd_tab, n_wp);
            hipLaunchKernelGGL(k_band_wd_points<NFP>, dim3((n_wd + 255) / 256, n_wp), dim3(256), 0, stream, pk, s.hdr, s.n_pops, b.wd_tab, n_wp, sp, b.values);
        }
        const size_t lds = b.bins ? sizeof(double) * 64 * (size_t)(2 * b.n_bins + 4) : 0;
        hipLaunchKernelGGL(k_band_accumulate, dim3((unsigned)((sp.n_lines + 63) / 64)), dim3(64), lds, stream, b.values, n_rows, sp.n_lines, b.pivot, b.mom,
                           b.bins, b.edges_t, b.n_bins);
        return hipGetLastError();
    });
}

// doubles of one (walker, population)'s node table (MargLayout, b9_device.h)
long long b9k_marg_table_doubles(int nfp, int mass_cap, int K, int Q) { return marg_layout(nfp, mass_cap, K, Q).total; }
// Does a catalogue of n_star_chunks x n_pops split its star chunks' windows over several workgroups (DevStars::mg_piece)?  Below 512
// chunk-populations (32k stars of one population) -- a function of the CATALOGUE, never of the walkers on the GPU: it decides how a
// star's sum rounds.  How many workgroups each chunk gets is the catalogue plan's business (b9_capi_margplan.cpp).  Measured in round 4
// with a uniform split, ms per b9_logpost call at 4 x 4, one workgroup per chunk -> split: 10k stars x 1 walker 0.18 -> 0.07, 200 stars
// 0.14 -> 0.06, 20k x 8 walkers 0.21 -> 0.19; 30k x 2 populations x 8 walkers would lose (0.27 -> 0.37: 938 chunk-populations, unsplit).
int b9k_marg_split(int n_star_chunks, int n_pops) { return n_star_chunks * n_pops < 512 ? 1 : 0; }
long long b9k_marg_shares_doubles(int n_pieces, int n_pops) { return (long long)std::max(1, n_pieces) * n_pops * 128; }      // per walker
long long b9k_marg_wd_table_doubles(int nfp, int K) { return (long long)8 * K * (2 * nfp + 1); }       // per (walker, population)

// Does a launch of `wgs` star workgroups leave the chip nearly empty (at most five waves per SIMD on average; n_cu: the compute
// units of the context's device, as every other plan counts them)?  Then its waves are latency-bound on the row loop: the SPARSE
// tile setting (star_marg_body, TILE = 2: same bits, speed only -- tests/test_gpu_placement.py crosses the two).
static bool marg_sparse(long long wgs, int n_cu)
{
    return wgs * 4 <= (long long)5 * std::max(1, n_cu) * 4;
}

// The node tables of n_walkers x n_pops derived isochrones: one workgroup per (walker-population, 64-node chunk).  Returns what
// the LDS opt-in said; the caller collects the launch's own error.
template <int NFP>
static hipError_t launch_marg_table(const DevPack &pk, const B9IsoSet &s, int n_walkers, const B9Marg &mg, hipStream_t stream)
{
    const MargLayout L = marg_layout(NFP, s.mass_cap, mg.K, mg.Q);
    const auto k = with_lds(k_marg_table<NFP>, sizeof(double) * ((size_t)s.mass_cap + 8 + 8 * NFP));
    if (k.err != hipSuccess) return k.err;
    hipLaunchKernelGGL(k.kern, dim3(n_walkers * s.n_pops, L.n_chunks), dim3(256), k.lds, stream, pk, s.hdr, s.iso,
                       s.iso_stride, s.mass_cap, s.n_pops, s.params, mg.K, mg.Q, mg.tab, L);
    return hipSuccess;
}
// ... and the WD-stage stars' node table (2 x 8 K WD chains per walker and population)
template <int NFP>
static void launch_marg_wd_table(const DevPack &pk, const B9IsoSet &s, int n_walkers, const B9Marg &mg, hipStream_t stream)
{
    hipLaunchKernelGGL((k_marg_wd_table<NFP>), dim3(n_walkers * s.n_pops, (8 * mg.K + 63) / 64), dim3(128), 0, stream, pk, s.hdr, s.iso, s.iso_stride,
                       s.mass_cap, s.n_pops, s.params, mg.K, mg.wd_tab, n_walkers * s.n_pops);
}
// the pruning width the star kernels take
static double marg_cut2(const B9Marg &mg) { return mg.prune ? 2.0 * B9_MARG_CUT : __builtin_inf(); }

// What the five reductions over a saved chain launch first, behind the guard they share (the tables, the scratch, 1 .. 65535
// rows): the node table of a chunk of rows (k_marg_table, its layout L) into the call's own buffer, with WD-stage stars
// k_marg_wd_table too, and the pruning width cut2 the star kernels take.  err: nothing of the call's own may be launched.
struct ChainTables { hipError_t err; MargLayout L; double cut2; };
template <int NFP>
static ChainTables chain_tables(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, hipStream_t stream)
{
    ChainTables t{hipErrorInvalidValue, marg_layout(NFP, c.set.mass_cap, c.mg.K, c.mg.Q), marg_cut2(c.mg)};
    if (!c.mg.tab || !c.scratch || n_rows < 1 || n_rows > 65535 || (st.n_wd > 0 && !c.mg.wd_tab)) return t;
    t.err = launch_marg_table<NFP>(pk, c.set, n_rows, c.mg, stream);
    if (t.err == hipSuccess && st.n_wd > 0) launch_marg_wd_table<NFP>(pk, c.set, n_rows, c.mg, stream);
    return t;
}

// ---- b9_star_moments: the node tables of a chunk of rows into the call's own buffers, the stars' increments, the accumulation -----
hipError_t b9k_star_moments(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, hipStream_t stream)
{
    return dispatch(pk.nfp, c.set.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        const B9IsoSet &s = c.set;
        if (!c.acc) return hipErrorInvalidValue;
        const ChainTables t = chain_tables<NFP>(pk, st, c, n_rows, stream);
        if (t.err != hipSuccess) return t.err;
        hipLaunchKernelGGL((k_star_moments<NFP, NPOPS>), dim3(st.mg_pad / 64, n_rows), dim3(256), 0, stream, st, s.hdr, s.iso, s.iso_stride, s.mass_cap,
                           s.params, c.mg.K, c.mg.Q, c.mg.tab, t.L, t.cut2, c.scratch);
        if (st.n_wd > 0)
            hipLaunchKernelGGL((k_star_moments_wd<NFP, NPOPS>), dim3((st.n_wd + 3) / 4, n_rows), dim3(256), 0, stream, st, pk.m_wd_up, s.hdr, s.params, c.mg.K,
                               c.mg.wd_tab, c.scratch);
        launch_chain_accumulate(c.scratch, n_rows, (long long)st.n * B9_MOM_N, c.acc, stream);
        return hipGetLastError();
    });
}

// ---- b9_mass_hist: the node tables of a chunk of rows, the stars' binned increments, the accumulation, the rows' sums -----------
hipError_t b9k_mass_hist(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, int quantity, const double *edges, int n_bins,
                         hipStream_t stream)
{
    return dispatch(pk.nfp, c.set.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        const B9IsoSet &s = c.set;
        if (!edges || n_bins < 1 || n_bins > B9_HIST_MAX_BINS) return hipErrorInvalidValue;
        HistEdges ed{};
        for (int b = 0; b <= n_bins; ++b) ed.e[b] = edges[b];
        ed.n_bins = n_bins; ed.quantity = quantity;
        const ChainTables t = chain_tables<NFP>(pk, st, c, n_rows, stream);
        if (t.err != hipSuccess) return t.err;
        // a tile of bins: one histogram [bins][64] per wave
        const int tb = std::min(n_bins, B9_HIST_TILE), n_tiles = (n_bins + B9_HIST_TILE - 1) / B9_HIST_TILE;
        const auto k = with_lds(k_star_hist<NFP, NPOPS>, sizeof(double) * 64 * (NPOPS * 4 + 4 * 2 + 4 * (size_t)tb));   // seeds, states, histograms
        if (k.err != hipSuccess) return k.err;
        hipLaunchKernelGGL(k.kern, dim3(st.mg_pad / 64, n_rows, n_tiles), dim3(256), k.lds, stream, st, s.hdr, s.iso, s.iso_stride, s.mass_cap,
                           s.params, c.mg.K, c.mg.Q, c.mg.tab, t.L, t.cut2, ed, tb, c.scratch);
        if (st.n_wd > 0)
            hipLaunchKernelGGL((k_star_hist_wd<NFP, NPOPS>), dim3((st.n_wd + 3) / 4, n_rows), dim3(256), 0, stream, st, pk.m_wd_up, s.hdr, s.params, c.mg.K,
                               c.mg.wd_tab, ed, c.scratch);
        const int ncol = n_bins + 1;
        if (c.acc) launch_chain_accumulate(c.scratch, n_rows, (long long)st.n * ncol, c.acc, stream);
        if (c.rows)
            hipLaunchKernelGGL(k_hist_rows, dim3((unsigned)((n_rows * ncol + 255) / 256)), dim3(256), 0, stream, c.scratch, n_rows, st.n, ncol, c.rows);
        return hipGetLastError();
    });
}

// ---- b9_ratio_hist: the node tables of a chunk of rows, the stars' (mass bin, ratio node) increments, the accumulation, the rows' sums
hipError_t b9k_ratio_hist(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, const double *mass_edges, int n_mbins, hipStream_t stream)
{
    return dispatch(pk.nfp, c.set.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        const B9IsoSet &s = c.set;
        const int Q = c.mg.Q;
        if (!mass_edges || n_mbins < 1 || n_mbins > B9_RH_MAX_MBINS || Q < 1 || Q > B9_RH_MAX_Q || n_mbins * Q > B9_RH_MAX_CELLS) return hipErrorInvalidValue;
        HistEdges ed{};
        for (int b = 0; b <= n_mbins; ++b) ed.e[b] = mass_edges[b];
        ed.n_bins = n_mbins; ed.quantity = B9_HQ_PRIMARY;
        const ChainTables t = chain_tables<NFP>(pk, st, c, n_rows, stream);
        if (t.err != hipSuccess) return t.err;
        // a tile of whole mass bins: one histogram [mass bins of the tile x Q][64] per wave
        const int mpt = std::max(1, B9_HIST_TILE / Q), tc = std::min(n_mbins, mpt) * Q, n_tiles = (n_mbins + mpt - 1) / mpt;
        const auto k = with_lds(k_star_ratio<NFP, NPOPS>, sizeof(double) * 64 * (NPOPS * 4 + 4 * 2 + 4 * (size_t)tc));      // seeds, states, histograms
        if (k.err != hipSuccess) return k.err;
        hipLaunchKernelGGL(k.kern, dim3(st.mg_pad / 64, n_rows, n_tiles), dim3(256), k.lds, stream, st, s.hdr, s.iso, s.iso_stride, s.mass_cap,
                           s.params, c.mg.K, Q, c.mg.tab, t.L, t.cut2, ed, mpt, tc, c.scratch);
        if (st.n_wd > 0)
            hipLaunchKernelGGL((k_star_ratio_wd<NFP, NPOPS>), dim3((st.n_wd + 3) / 4, n_rows), dim3(256), 0, stream, st, pk.m_wd_up, s.hdr, s.params, c.mg.K,
                               Q, c.mg.wd_tab, ed, c.scratch);
        const int ncol = n_mbins * Q + 1;
        if (c.acc) launch_chain_accumulate(c.scratch, n_rows, (long long)st.n * ncol, c.acc, stream);
        if (c.rows)
            hipLaunchKernelGGL(k_hist_rows, dim3((unsigned)((n_rows * ncol + 255) / 256)), dim3(256), 0, stream, c.scratch, n_rows, st.n, ncol, c.rows);
        return hipGetLastError();
    });
}

// ---- b9_star_bins: the node tables of a chunk of rows, the stars' increments on their own edges, the accumulation -----------------
hipError_t b9k_star_bins(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, int quantity, const double *edges, int n_bins,
                         hipStream_t stream)
{
    return dispatch(pk.nfp, c.set.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        const B9IsoSet &s = c.set;
        if (!c.acc || !edges || n_bins < 1 || n_bins > B9_SBIN_MAX_BINS) return hipErrorInvalidValue;
        const ChainTables t = chain_tables<NFP>(pk, st, c, n_rows, stream);
        if (t.err != hipSuccess) return t.err;
        // seeds, states, the 64 stars' edges, one histogram [n_bins + 2][64] per wave
        const auto k = with_lds(k_star_bins<NFP, NPOPS>, sizeof(double) * 64 * (NPOPS * 4 + 4 * 2 + (size_t)(n_bins + 1) + 4 * (size_t)(n_bins + 2)));
        if (k.err != hipSuccess) return k.err;
        hipLaunchKernelGGL(k.kern, dim3(st.mg_pad / 64, n_rows), dim3(256), k.lds, stream, st, s.hdr, s.iso, s.iso_stride, s.mass_cap,
                           s.params, c.mg.K, c.mg.Q, c.mg.tab, t.L, t.cut2, edges, n_bins, quantity, c.scratch);
        if (st.n_wd > 0)
            hipLaunchKernelGGL((k_star_bins_wd<NFP, NPOPS>), dim3((st.n_wd + 3) / 4, n_rows), dim3(256), 0, stream, st, pk.m_wd_up, s.hdr, s.params, c.mg.K,
                               c.mg.wd_tab, edges, n_bins, quantity, c.scratch);
        launch_chain_accumulate(c.scratch, n_rows, (long long)st.n * (n_bins + 3), c.acc, stream);
        return hipGetLastError();
    });
}

// ---- b9_phot_resid: the node tables of a chunk of rows, the stars' residual increments, the accumulation, the rows' sums ----------
hipError_t b9k_resid_stage(const DevPack &pk, const DevStars &st, const double *piv_in, double *piv_mg, hipStream_t stream)
{
    return dispatch_nfp(pk.nfp, [&](auto nfp_c) {
        constexpr int NFP = decltype(nfp_c)::value;
        if (!piv_in || !piv_mg) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_resid_stage<NFP>, dim3((unsigned)((st.mg_pad * NFP + 255) / 256)), dim3(256), 0, stream, st, pk.nf, piv_in, piv_mg);
        return hipGetLastError();
    });
}

hipError_t b9k_phot_resid(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, const double *piv_mg, const double *isig, hipStream_t stream)
{
    return dispatch(pk.nfp, c.set.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        const B9IsoSet &s = c.set;
        if (!piv_mg || (c.rows && !isig)) return hipErrorInvalidValue;
        const int nf = pk.nf;
        const ChainTables t = chain_tables<NFP>(pk, st, c, n_rows, stream);
        if (t.err != hipSuccess) return t.err;
        const auto k = with_lds(k_star_resid<NFP, NPOPS>, sizeof(double) * 64 * (NPOPS * 4 + 4 * (2 + 2 * (size_t)NFP)));      // seeds, one population's states
        if (k.err != hipSuccess) return k.err;
        hipLaunchKernelGGL(k.kern, dim3(st.mg_pad / 64, n_rows), dim3(256), k.lds, stream, st, nf, piv_mg, s.hdr, s.iso, s.iso_stride, s.mass_cap,
                           s.params, c.mg.K, c.mg.Q, c.mg.tab, t.L, t.cut2, c.scratch);
        if (st.n_wd > 0)
            hipLaunchKernelGGL((k_star_resid_wd<NFP, NPOPS>), dim3((st.n_wd + 3) / 4, n_rows), dim3(256), 0, stream, st, nf, pk.m_wd_up, s.hdr, s.params, c.mg.K,
                               c.mg.wd_tab, c.scratch);
        if (c.acc) launch_chain_accumulate(c.scratch, n_rows, (long long)st.n * (2 + 2 * nf), c.acc, stream);
        if (c.rows) {
            const auto kr = with_lds(k_resid_rows, sizeof(double) * 2 * B9_RESID_TILE * (2 + 3 * (size_t)nf));      // two tiles of {x, 1 / sigma}
            if (kr.err != hipSuccess) return kr.err;
            hipLaunchKernelGGL(kr.kern, dim3(n_rows), dim3(256), kr.lds, stream, c.scratch, isig, st.n, nf, c.rows);
        }
        return hipGetLastError();
    });
}

// ---- b9_filter_loo: the node tables of a chunk of rows, the stars' leave-one-filter-out increments, the accumulation, the rows' sums
hipError_t b9k_filter_loo(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, const double *piv_mg, const double *lsn_mg, const double *lsn,
                          const double *isig, hipStream_t stream)
{
    return dispatch(pk.nfp, c.set.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value, LT = LooTile<NFP>::LT;
        const B9IsoSet &s = c.set;
        if (!piv_mg || !lsn_mg || !lsn || (c.rows && !isig)) return hipErrorInvalidValue;
        const int nf = pk.nf;
        const ChainTables t = chain_tables<NFP>(pk, st, c, n_rows, stream);
        if (t.err != hipSuccess) return t.err;
        const auto k = with_lds(k_star_loo<NFP, NPOPS>, sizeof(double) * 64 * (NPOPS * 4 + 4 * (2 + 4 * (size_t)LT)));      // seeds, one population's states
        if (k.err != hipSuccess) return k.err;
        hipLaunchKernelGGL(k.kern, dim3(st.mg_pad / 64, n_rows, NFP / LT), dim3(256), k.lds, stream, st, nf, piv_mg, lsn_mg, s.hdr, s.iso, s.iso_stride,
                           s.mass_cap, s.params, c.mg.K, c.mg.Q, c.mg.tab, t.L, t.cut2, c.scratch);
        if (st.n_wd > 0)
            hipLaunchKernelGGL((k_star_loo_wd<NFP, NPOPS>), dim3((st.n_wd + 3) / 4, n_rows), dim3(256), 0, stream, st, nf, pk.m_wd_up, s.hdr, s.params, c.mg.K,
                               c.mg.wd_tab, lsn, c.scratch);
        if (c.acc) launch_chain_accumulate(c.scratch, n_rows, (long long)st.n * (2 + 3 * nf), c.acc, stream);
        if (c.rows) {
            const auto kr = with_lds(k_loo_rows, sizeof(double) * 2 * B9_LOO_TILE * (2 + 4 * (size_t)nf));      // two tiles of {x, 1 / sigma}
            if (kr.err != hipSuccess) return kr.err;
            hipLaunchKernelGGL(kr.kern, dim3(n_rows), dim3(256), kr.lds, stream, c.scratch, isig, st.n, nf, c.rows);
        }
        return hipGetLastError();
    });
}

// ---- b9_star_offset: the call's directions staged; then the node tables of a chunk of rows, the stars' offset increments, the
// accumulation, the rows' sums
static OffDirs off_dirs(const DevPack &pk, const B9Offset &o)
{
    OffDirs d{};
    for (int j = 0; j < o.n_dir; ++j) {
        for (int f = 0; f < pk.nf; ++f) d.k[j][f] = o.k[(size_t)j * pk.nf + f];
        d.tau2[j] = o.tau[j] * o.tau[j];
        d.itau2[j] = 1.0 / d.tau2[j];
    }
    return d;
}
static bool off_ok(const DevPack &pk, const B9Offset &o)
{
    return o.n_dir >= 1 && o.n_dir <= B9_OFF_MAX_DIR && pk.nf <= B9_MAX_FILT && o.k && o.tau && o.c_in && o.c_mg && o.cv && o.ob;
}

hipError_t b9k_offset_stage(const DevPack &pk, const DevStars &st, const B9Offset &o, hipStream_t stream)
{
    return dispatch_nfp(pk.nfp, [&](auto nfp_c) {
        constexpr int NFP = decltype(nfp_c)::value;
        if (!off_ok(pk, o)) return hipErrorInvalidValue;
        const long long lanes = std::max((long long)st.mg_pad * NFP * o.n_dir, (long long)st.n * o.n_dir);
        hipLaunchKernelGGL(k_offset_stage<NFP>, dim3((unsigned)((lanes + 255) / 256), 2), dim3(256), 0, stream, st, pk.nf, o.n_dir, off_dirs(pk, o), o.c_in, o.c_mg,
                           o.cv, o.ob);
        return hipGetLastError();
    });
}

template <int NFP, int NPOPS, int DT>
static hipError_t launch_star_off(const DevStars &st, const B9Chain &c, const ChainTables &t, int n_rows, const B9Offset &o, hipStream_t stream)
{
    const B9IsoSet &s = c.set;
    const auto k = with_lds(k_star_off<NFP, NPOPS, DT>, sizeof(double) * 64 * (NPOPS * 4 + 4 * (2 + 4 * (size_t)DT)));      // seeds, one population's states
    if (k.err != hipSuccess) return k.err;
    hipLaunchKernelGGL(k.kern, dim3(st.mg_pad / 64, n_rows, (o.n_dir + DT - 1) / DT), dim3(256), k.lds, stream, st, o.n_dir, o.c_mg, o.cv, o.ob, s.hdr, s.iso,
                       s.iso_stride, s.mass_cap, s.params, c.mg.K, c.mg.Q, c.mg.tab, t.L, t.cut2, c.scratch);
    return hipGetLastError();
}

hipError_t b9k_star_offset(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, const B9Offset &o, hipStream_t stream)
{
    return dispatch(pk.nfp, c.set.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value, DT_MAX = OffTile<NFP>::DT_MAX;
        if (!off_ok(pk, o)) return hipErrorInvalidValue;
        const int D = o.n_dir;
        const ChainTables t = chain_tables<NFP>(pk, st, c, n_rows, stream);
        if (t.err != hipSuccess) return t.err;
        hipError_t err;
        if (D == 1) err = launch_star_off<NFP, NPOPS, 1>(st, c, t, n_rows, o, stream);
        else if (D == 2 || DT_MAX == 2) err = launch_star_off<NFP, NPOPS, 2>(st, c, t, n_rows, o, stream);
        else err = launch_star_off<NFP, NPOPS, DT_MAX>(st, c, t, n_rows, o, stream);
        if (err != hipSuccess) return err;
        if (st.n_wd > 0)
            hipLaunchKernelGGL((k_star_off_wd<NFP, NPOPS>), dim3((st.n_wd + 3) / 4, n_rows), dim3(256), 0, stream, st, D, off_dirs(pk, o), pk.m_wd_up, c.set.hdr, c.set.params,
                               c.mg.K, c.mg.wd_tab, c.scratch);
        if (c.acc) launch_chain_accumulate(c.scratch, n_rows, (long long)st.n * (2 + 3 * D), c.acc, stream);
        if (c.rows) {
            const auto kr = with_lds(k_off_rows, sizeof(double) * 2 * B9_OFF_TILE * (2 + 5 * (size_t)D));      // two tiles of {x, C, V}
            if (kr.err != hipSuccess) return kr.err;
            hipLaunchKernelGGL(kr.kern, dim3(n_rows), dim3(256), kr.lds, stream, c.scratch, o.cv, st.n, D, c.rows);
        }
        return hipGetLastError();
    });
}

// ---- b9_pointwise: the node tables of a chunk of rows, every star's v, the per-star state, the tails, the rows' sums ---------------
hipError_t b9k_pw_tail_load(const double *tail_io, int n_stars, int tail_len, double *tail, hipStream_t stream)
{
    if (!tail || n_stars < 1 || tail_len < 1) return hipErrorInvalidValue;
    const long long n = (long long)n_stars * tail_len;
    if (tail_io) hipLaunchKernelGGL(k_pw_transpose, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, tail_io, n_stars, tail_len, tail);
    else hipLaunchKernelGGL(k_pw_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, tail, n, (double)NEG_INF);
    return hipGetLastError();
}

hipError_t b9k_pw_tail_store(const double *tail, int n_stars, int tail_len, double *tail_io, hipStream_t stream)
{
    if (!tail || !tail_io || n_stars < 1 || tail_len < 1) return hipErrorInvalidValue;
    const long long n = (long long)n_stars * tail_len;
    hipLaunchKernelGGL(k_pw_transpose, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, tail, tail_len, n_stars, tail_io);
    return hipGetLastError();
}

// the value half, shared with b9k_star_influence: scratch [n_rows][st.n] and row_in [n_rows]
template <int NFP, int NPOPS>
static hipError_t launch_pw_values(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, int *row_in, hipStream_t stream)
{
    const B9IsoSet &s = c.set;
    const ChainTables t = chain_tables<NFP>(pk, st, c, n_rows, stream);
    if (t.err != hipSuccess) return t.err;
    hipLaunchKernelGGL((k_star_lpd<NFP, NPOPS>), dim3(st.mg_pad / 64, n_rows), dim3(256), 0, stream, st, s.hdr, s.iso, s.iso_stride, s.mass_cap,
                       s.params, c.mg.K, c.mg.Q, c.mg.tab, t.L, t.cut2, c.scratch, row_in);
    if (st.n_wd > 0)
        hipLaunchKernelGGL((k_star_lpd_wd<NFP, NPOPS>), dim3((st.n_wd + 3) / 4, n_rows), dim3(256), 0, stream, st, pk.m_wd_up, s.hdr, s.params, c.mg.K,
                           c.mg.wd_tab, c.scratch);
    return hipSuccess;
}
// ... and the tails
static hipError_t launch_pw_tail(const DevStars &st, const B9Chain &c, int n_rows, const int *row_in, double *tail, int tail_len, hipStream_t stream)
{
    const auto kt = with_lds(k_pw_tail, sizeof(double) * 64 * (size_t)tail_len);          // the wave's 64 lists
    if (kt.err != hipSuccess) return kt.err;
    hipLaunchKernelGGL(kt.kern, dim3((unsigned)((st.n + 63) / 64)), dim3(64), kt.lds, stream, c.scratch, row_in, n_rows, st.n, tail_len, tail);
    return hipSuccess;
}

hipError_t b9k_pointwise(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, int *row_in, double *tail, int tail_len, hipStream_t stream)
{
    return dispatch(pk.nfp, c.set.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        if (!row_in || n_rows > B9_PW_MAX_ROWS || (tail && (!c.acc || tail_len < 1 || tail_len > B9_PW_MAX_TAIL))) return hipErrorInvalidValue;
        if (const hipError_t e = launch_pw_values<NFP, NPOPS>(pk, st, c, n_rows, row_in, stream)) return e;
        const unsigned star_wgs = (unsigned)((st.n + 255) / 256);
        if (c.acc)
            hipLaunchKernelGGL(k_pw_accumulate, dim3(star_wgs), dim3(256), 0, stream, c.scratch, row_in, n_rows, st.n, c.acc);
        if (tail)
            if (const hipError_t e = launch_pw_tail(st, c, n_rows, row_in, tail, tail_len, stream)) return e;
        if (c.rows)
            hipLaunchKernelGGL(k_pw_rows, dim3((unsigned)n_rows), dim3(64), 0, stream, c.scratch, row_in, st.n, c.rows);
        return hipGetLastError();
    });
}

// ---- b9_star_influence: b9_pointwise's values of a chunk of rows, then the per-star influence state, the tails, the groups' sums
template <int QT>
static void launch_infl_accumulate(const DevStars &st, const B9Chain &c, int n_rows, const int *row_in, const B9Influence &f, hipStream_t stream)
{
    // one launch per tile, in stream order: every tile reads the head as the chunk found it, the last one stores the new head
    const int tiles = (f.n_q + QT - 1) / QT;
    for (int t = 0; t < tiles; ++t)
        hipLaunchKernelGGL(k_infl_accumulate<QT>, dim3((unsigned)((st.n + 255) / 256)), dim3(256), 0, stream, c.scratch, row_in, n_rows, st.n, f.q, f.n_q, t,
                           t == tiles - 1 ? 1 : 0, c.acc);
}
template <int NG>
static void launch_infl_groups(const DevStars &st, const B9Chain &c, int n_rows, const int *row_in, const B9Influence &f, hipStream_t stream)
{
    hipLaunchKernelGGL(k_infl_groups<NG>, dim3((unsigned)n_rows), dim3(64), 0, stream, c.scratch, row_in, st.n, f.group, f.n_groups, c.rows);
}

hipError_t b9k_star_influence(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, int *row_in, double *tail, int tail_len, const B9Influence &f,
                              hipStream_t stream)
{
    return dispatch(pk.nfp, c.set.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        if (!row_in || n_rows > B9_PW_MAX_ROWS || (tail && (!c.acc || tail_len < 1 || tail_len > B9_PW_MAX_TAIL))) return hipErrorInvalidValue;
        if (c.acc && (!f.q || f.n_q < 1 || f.n_q > B9_INF_MAX_Q)) return hipErrorInvalidValue;
        if (c.rows && (!f.group || f.n_groups < 1 || f.n_groups > B9_INF_MAX_GROUPS)) return hipErrorInvalidValue;
        if (const hipError_t e = launch_pw_values<NFP, NPOPS>(pk, st, c, n_rows, row_in, stream)) return e;
        if (c.acc) {
            // quantities per instance: every tile is a launch and recomputes the head, so as few tiles as the registers carry
            if (f.n_q == 1) launch_infl_accumulate<1>(st, c, n_rows, row_in, f, stream);
            else if (f.n_q == 2) launch_infl_accumulate<2>(st, c, n_rows, row_in, f, stream);
            else launch_infl_accumulate<4>(st, c, n_rows, row_in, f, stream);
        }
        if (tail)
            if (const hipError_t e = launch_pw_tail(st, c, n_rows, row_in, tail, tail_len, stream)) return e;
        if (c.rows) {
            if (f.n_groups == 1) launch_infl_groups<1>(st, c, n_rows, row_in, f, stream);
            else if (f.n_groups == 2) launch_infl_groups<2>(st, c, n_rows, row_in, f, stream);
            else if (f.n_groups <= 4) launch_infl_groups<4>(st, c, n_rows, row_in, f, stream);
            else launch_infl_groups<8>(st, c, n_rows, row_in, f, stream);
        }
        return hipGetLastError();
    });
}

// The marginalised star grid: one workgroup (four waves sharing the node table's sub-chunks) per (64-star chunk or piece, walker),
// dispatched in DevStars::marg_order.
// XCD placement (k_star_marg's head): two walker groups x four star-chunk groups.  Each XCD's L2 fetches its group's node
// tables and its share of the stars once: 8 x (tables / wsplit) + wsplit x (star copy) bytes in all -- 50k stars x 8
// walkers, 4 x 4 grid: 42.5 MB per launch at wsplit 1, 35.2 at 2, 41.3 at 4 (rocprofv3 FETCH_SIZE; the launch time is the
// same for all three: 164 us -- the kernel is VALU-bound, the placement only decides how much crosses the fabric)
struct MargGrid { int wsplit, csplit, per_xcd; };      // walker groups, star-chunk groups, star workgroups per XCD
static MargGrid marg_star_grid(const DevStars &st, int n_walkers, bool split)
{
    MargGrid g;
    g.wsplit = n_walkers % 2 == 0 ? 2 : 1;
    g.csplit = 8 / g.wsplit;
    g.per_xcd = (((split ? st.mg_n_pieces : st.mg_pad / 64) + g.csplit - 1) / g.csplit) * (n_walkers / g.wsplit);
    return g;
}

// smp == nullptr: the plain marginal likelihood; else every star also draws one (mass, ratio[, population]) node
hipError_t b9k_star_marg(const DevPack &pk, const DevStars &st, const B9IsoSet &set, int n_walkers, const B9Partial &partial, double *perstar,
                         const B9Marg &mg, const B9MargSample *smp, int n_cu, hipStream_t stream)
{
    return dispatch(pk.nfp, set.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        const auto launch = [&](auto sample_c) {
            constexpr bool SAMPLE = decltype(sample_c)::value;
            MargSample ms{};
            if (SAMPLE) { ms.mass = smp->mass; ms.ratio = smp->ratio; ms.member = smp->member; ms.pop = smp->pop; ms.k0 = smp->k0; ms.k1 = smp->k1; ms.row0 = smp->row0; }
            if (!mg.tab) return hipErrorInvalidValue;
            const MargLayout L = marg_layout(NFP, set.mass_cap, mg.K, mg.Q);
            const hipError_t e = launch_marg_table<NFP>(pk, set, n_walkers, mg, stream);      // the call's node table
            if (e != hipSuccess) return e;
            // SPLIT: a small catalogue's launch lasts as long as its heaviest star chunk (giants: 100 us where the median chunk takes
            // 40) while most of the chip idles, so several workgroups share a chunk's window (DevStars::mg_piece; k_marg_merge).  A
            // function of the CATALOGUE only -- it decides how a star's sum rounds, and a walker's chain must not depend on how many
            // walkers share the GPU.  The sampleMass draws keep one workgroup per chunk.
            const bool split = !SAMPLE && st.mg_n_pieces > 0;
            if (split && !mg.shares) return hipErrorInvalidValue;
            const MargGrid g = marg_star_grid(st, n_walkers, split);
            const double cut2 = marg_cut2(mg);
            // rows through LDS tiles or through scalar registers (star_marg_body, TILE): measured per instance -- 8 (4) filters x one
            // population, unsplit, is the one shape the scalar path still wins in this kernel (2.20 against 2.17e9 star-evals/s)
            const bool sparse = !SAMPLE && split && marg_sparse((long long)st.mg_n_pieces * n_walkers, n_cu);
            const bool tiled = !SAMPLE && (split || NPOPS == 2 || NFP >= 16);
            const auto kern = sparse ? k_star_marg<NFP, NPOPS, SAMPLE, !SAMPLE, false, SAMPLE ? 0 : 2>
                            : split  ? k_star_marg<NFP, NPOPS, SAMPLE, !SAMPLE, false, SAMPLE ? 0 : 1>
                            : tiled  ? k_star_marg<NFP, NPOPS, SAMPLE, false, false, SAMPLE ? 0 : 1>
                                     : k_star_marg<NFP, NPOPS, SAMPLE, false>;
            const size_t tile_lds = tiled ? sizeof(double) * 4 * B9_TILE_DOUBLES(NFP) : 0;
            hipLaunchKernelGGL(kern, dim3(8 * g.per_xcd), dim3(256), tile_lds, stream, pk, st, set.hdr, set.iso, set.iso_stride,
                               set.mass_cap, set.params, partial.ptr, partial.stride, perstar, mg.K, mg.Q, ms, mg.tab, L, n_walkers, cut2, g.wsplit, mg.shares);
            if (split)
                hipLaunchKernelGGL((k_marg_merge<NPOPS>), dim3(st.mg_pad / 64, n_walkers), dim3(64), 0, stream, st, set.hdr, set.params, partial.ptr, partial.stride,
                                   perstar, mg.shares);
            if (st.n_wd > 0) {        // the catalogue's WD-stage stars: their node table, then a wave per star
                if (!mg.wd_tab) return hipErrorInvalidValue;
                launch_marg_wd_table<NFP>(pk, set, n_walkers, mg, stream);
                hipLaunchKernelGGL((k_star_marg_wd<NFP, NPOPS, SAMPLE>), dim3((st.n_wd + 3) / 4, n_walkers), dim3(256), 0, stream, pk, st, set.hdr,
                                   set.iso, set.iso_stride, set.mass_cap, set.params, partial.ptr, partial.stride, perstar, mg.K, ms, mg.wd_tab);
            }
            return hipGetLastError();
        };
        return smp ? launch(std::true_type{}) : launch(std::false_type{});
    });
}

// The catalogue plan's counting pass: the unsplit star kernel on ONE row (the reference row), every wave leaving the number of
// (16 nodes x one mass ratio) units it evaluated in cost[star chunk][4].
hipError_t b9k_star_marg_cost(const DevPack &pk, const DevStars &st, const B9IsoSet &set, const B9Partial &partial, const B9Marg &mg, unsigned *cost,
                              hipStream_t stream)
{
    return dispatch(pk.nfp, set.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        MargSample ms{};
        ms.cost = cost;
        const MargLayout L = marg_layout(NFP, set.mass_cap, mg.K, mg.Q);
        const int n_chunks = st.mg_pad / 64;
        hipLaunchKernelGGL((k_star_marg<NFP, NPOPS, false, false, true>), dim3(8 * ((n_chunks + 7) / 8)), dim3(256), 0, stream, pk, st, set.hdr, (const double *)nullptr, 0ll,
                           set.mass_cap, set.params, partial.ptr, partial.stride, (double *)nullptr, mg.K, mg.Q, ms, mg.tab, L, 1, marg_cut2(mg), 1, (double *)nullptr);
        return hipGetLastError();
    });
}

// ---- the marginalised mode's fused sampler step (k_marg_step) -----------------------------------------------------------
// The node tables of a set of derived isochrones WITHOUT the star launch: the prologue of a fused block (its first
// proposal comes from k_derive_iso; every later one is built inside k_marg_step).
hipError_t b9k_marg_tables(const DevPack &pk, const B9IsoSet &set, int n_walkers, const B9Marg &mg, hipStream_t stream)
{
    return dispatch_nfp(pk.nfp, [&](auto nfp_c) {
        constexpr int NFP = decltype(nfp_c)::value;
        const hipError_t e = launch_marg_table<NFP>(pk, set, n_walkers, mg, stream);
        if (e != hipSuccess) return e;
        if (mg.wd_tab) launch_marg_wd_table<NFP>(pk, set, n_walkers, mg, stream);
        return hipGetLastError();
    });
}

// Dynamic LDS of k_marg_step (its table builders' tiles; every workgroup of the launch gets it): the fused step runs only while it
// leaves the star role its workgroups per CU (B9_MSTEP_LDS_MAX: 160 KB / 7 less the kernel's static arrays, with 8 filters)
size_t b9k_marg_step_lds(int nfp, int mass_cap) { return sizeof(double) * B9_MSTEP_LDS_DOUBLES(nfp, mass_cap); }

hipError_t b9k_marg_step(const DevPack &pk, const DevStars &st, const StepDev &sd, const DevPriors &pr, const B9Marg &mg, int n_cu, hipStream_t stream)
{
    return dispatch(pk.nfp, sd.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        const int W = sd.n_walkers, K = mg.K;
        const bool split = st.mg_n_pieces > 0;
        const MargGrid g = marg_star_grid(st, W, split);
        const long long wd_doubles = b9k_marg_wd_table_doubles(NFP, K);
        MargStep mx{};
        mx.K = K; mx.Q = mg.Q; mx.L = marg_layout(NFP, sd.mass_cap, K, mg.Q);
        mx.n_chunks_cap = mx.L.n_chunks;
        mx.n_wd_blocks = st.n_wd > 0 ? (8 * K + 127) / 128 : 0;
        mx.wsplit = g.wsplit;
        if (split && !mg.shares) return hipErrorInvalidValue;
        if (st.n_wd > 0 && !mg.wd_tab) return hipErrorInvalidValue;
        mx.cut2 = marg_cut2(mg);
        mx.tab = mg.tab; mx.wd_tab = mg.wd_tab; mx.wd_stride = (long long)W * NPOPS * wd_doubles; mx.shares = mg.shares;      // (wd_stride: one candidate's WD tables)
        const int front = (W + W * 2 * NPOPS * (mx.n_chunks_cap + mx.n_wd_blocks) + 7) / 8 * 8;
        const int stars = 8 * g.per_xcd;
        const int wd = st.n_wd > 0 ? ((st.n_wd + 3) / 4) * W : 0;
        const size_t lds = b9k_marg_step_lds(NFP, sd.mass_cap);
        if (lds > B9_MSTEP_LDS_MAX(NFP)) return hipErrorInvalidValue;
        // this parity's two candidates, as the star roles read them (see MargStepSel)
        const b9i::CandAt c0 = b9i::cand_at(sd.set, 0, W, NPOPS);
        const IsoHdr *hdr_rd = sd.cand_hdr + c0.wp;
        const double *par_rd = sd.cand_par + c0.row * B9_NPARAM, *tab_rd = mg.tab + c0.wp * mx.L.total, *wd_rd = mg.wd_tab ? mg.wd_tab + c0.wp * wd_doubles : nullptr;
        static_assert(B9_MSTEP_LDS_DOUBLES(NFP, 2) >= 4 * B9_TILE_DOUBLES(NFP), "the star role's row tiles borrow the builders' dynamic LDS");
        const auto kern = !split ? k_marg_step<NFP, NPOPS, false>
                        : marg_sparse((long long)st.mg_n_pieces * W, n_cu) ? k_marg_step<NFP, NPOPS, true, 2> : k_marg_step<NFP, NPOPS, true>;
        hipLaunchKernelGGL(kern, dim3(front + stars + wd), dim3(256), lds, stream, pk, st, sd, pr, mx, front, stars, hdr_rd, par_rd, tab_rd, wd_rd);
        if (split) hipLaunchKernelGGL((k_marg_step_merge<NPOPS>), dim3(st.mg_pad / 64, W), dim3(64), 0, stream, st, sd, mx);
        return hipGetLastError();
    });
}

// ---- the fused sampler step (k_mcmc_step) ------------------------------------------------------------------------
// k_mcmc_step's instance and its dynamic LDS: the hot role's mass columns of both candidates (+ 8: find_bracket's masked
// over-read), or the heavy role's axes, whichever is larger
static size_t mcmc_step_lds(const DevPack &pk, int n_pops, int mass_cap)
{
    return sizeof(double) * std::max((size_t)2 * n_pops * mass_cap + 8, heavy_lds_doubles(pk, n_pops, 2, mass_cap));
}

template <int NFP, int NPOPS>
static auto mcmc_step_kernel(const DevPack &pk, int mass_cap)
{
    return with_lds(k_mcmc_step<NFP, NPOPS>, mcmc_step_lds(pk, NPOPS, mass_cap));
}

// Workgroups of the fused step that one CU holds at once for the loaded pack (registers, LDS, wave slots of THIS
// instantiation): the launch plan sizes its single occupancy round from it instead of assuming a machine.
hipError_t b9k_mcmc_step_occupancy(const DevPack &pk, int n_pops, int mass_cap, int *blocks_per_cu)
{
    return dispatch(pk.nfp, n_pops, [&](auto nfp_c, auto npops_c) {
        const auto k = mcmc_step_kernel<decltype(nfp_c)::value, decltype(npops_c)::value>(pk, mass_cap);
        if (k.err != hipSuccess) return k.err;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, reinterpret_cast<const void *>(k.kern), 256, k.lds);
    });
}

void b9k_mcmc_step_desc(StepBlockDev *desc, const DevPack &pk, const DevStars &st, const StepDev &sd, const DevPriors &pr,
                        const B9Groups &gr, int heavy_parts, int derive_parts, int derive_order)
{
    std::memset(desc, 0, sizeof *desc);         // (padding too: the image is copied whole)
    desc->pk = pk; desc->st = st; desc->pr = pr; desc->sd = sd;
    desc->sd.set = desc->sd.has_prev = desc->sd.derive_next = desc->sd.row = 0; desc->sd.step = 0;      // the launch's own words
    desc->sd.rows = nullptr; desc->sd.host_state = nullptr; desc->sd.host_rows = nullptr;               // k_mcmc_finish's own
    const int W = sd.n_walkers, NPOPS = sd.n_pops;
    const int derive_first = derive_order >= 0 ? (derive_order == 1 ? 2 : 1) : 0;
    const int n_derive = W * 2 * NPOPS * derive_parts;
    StepGridDev &g = desc->grid;
    g.group_tiles = gr.group_tiles; g.n_groups = gr.n_groups; g.groups_per_block = gr.groups_per_block; g.n_blocks = gr.n_blocks;
    g.front_blocks = (W * heavy_parts + W + (derive_first ? n_derive : 0) + 7) / 8 * 8;     // heavy, writers, (derivation), pad
    g.hot_blocks = 8 * ((gr.n_blocks * NPOPS + 7) / 8) * W;
    g.heavy_parts = heavy_parts; g.derive_parts = derive_parts; g.derive_first = derive_first;
}

hipError_t b9k_mcmc_step(const StepBlockDev &desc, const StepBlockDev *d_desc, const StepDev &sd, hipStream_t stream)
{
    return dispatch(desc.pk.nfp, desc.sd.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        const auto k = mcmc_step_kernel<NFP, NPOPS>(desc.pk, desc.sd.mass_cap);
        if (k.err != hipSuccess) return k.err;
        const StepGridDev &g = desc.grid;
        const int back = (!g.derive_first && sd.derive_next) ? desc.sd.n_walkers * 2 * NPOPS * g.derive_parts : 0;
        // (the kernel's first parameter is a reference into the constant address space: the argument list holds the descriptor's
        //  device address, handed over here as the pointer it is)
        int set = sd.set, has_prev = sd.has_prev, derive_next = sd.derive_next, row = sd.row;
        unsigned long long step = sd.step;
        void *args[] = {&d_desc, &set, &has_prev, &derive_next, &row, &step};
        return hipLaunchKernel(reinterpret_cast<const void *>(k.kern), dim3(g.front_blocks + g.hot_blocks + back), dim3(256), args, k.lds, stream);
    });
}

// ---- tree-speculative step (k_mcmc_tree) -------------------------------------------------------------------------
// which of the two builds of b9_mcmc_tree.hip.h a catalogue of n_groups canonical groups uses
static bool tree_large(int n_groups) { return n_groups > 16 * B9_TREE_KD_SMALL; }

template <int NFP, int NPOPS>
static auto mcmc_tree_kernel(const DevPack &pk, int mass_cap, int n_groups)
{
    return with_lds(tree_large(n_groups) ? tree_kd5::k_mcmc_tree<NFP, NPOPS> : tree_kd3::k_mcmc_tree<NFP, NPOPS>, one_candidate_lds(pk, NPOPS, mass_cap));
}

// LDS of the launch that carries a given-mass block's heavy role -- the fused step, the tree launch's build for a catalogue of
// n_groups canonical groups, or the two-launch form's k_star_like: the dynamic request and, where that alone passes 64 KB, the
// kernel's static LDS beside it (no launch).
hipError_t b9k_step_lds(const DevPack &pk, int n_pops, int mass_cap, B9StepKind kind, int n_groups, size_t *dynamic_bytes, size_t *static_bytes)
{
    *dynamic_bytes = kind == B9_STEP_FUSED ? mcmc_step_lds(pk, n_pops, mass_cap) : one_candidate_lds(pk, n_pops, mass_cap);
    *static_bytes = 0;
    if (*dynamic_bytes <= 64 * 1024) return hipSuccess;
    return dispatch(pk.nfp, n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        const void *kern = kind == B9_STEP_FUSED ? reinterpret_cast<const void *>(k_mcmc_step<NFP, NPOPS>)
                         : kind == B9_STEP_STAR_LIKE ? reinterpret_cast<const void *>(k_star_like<NFP, NPOPS>)
                         : tree_large(n_groups) ? reinterpret_cast<const void *>(tree_kd5::k_mcmc_tree<NFP, NPOPS>)
                                                : reinterpret_cast<const void *>(tree_kd3::k_mcmc_tree<NFP, NPOPS>);
        hipFuncAttributes attr;
        const hipError_t e = hipFuncGetAttributes(&attr, kern);
        if (e == hipSuccess) *static_bytes = attr.sharedSizeBytes;
        return e;
    });
}

hipError_t b9k_mcmc_tree_occupancy(const DevPack &pk, int n_pops, int mass_cap, int n_groups, int *blocks_per_cu)
{
    return dispatch(pk.nfp, n_pops, [&](auto nfp_c, auto npops_c) {
        const auto k = mcmc_tree_kernel<decltype(nfp_c)::value, decltype(npops_c)::value>(pk, mass_cap, n_groups);
        if (k.err != hipSuccess) return k.err;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, reinterpret_cast<const void *>(k.kern), 256, k.lds);
    });
}

hipError_t b9k_mcmc_tree(const DevPack &pk, const DevStars &st, const TreeDev &td, const DevPriors &pr, int group_tiles,
                         int derive_parts, hipStream_t stream)
{
    return dispatch(pk.nfp, td.n_pops, [&](auto nfp_c, auto npops_c) {
        constexpr int NFP = decltype(nfp_c)::value, NPOPS = decltype(npops_c)::value;
        const auto k = mcmc_tree_kernel<NFP, NPOPS>(pk, td.mass_cap, td.n_groups);
        if (k.err != hipSuccess) return k.err;
        const int W = td.n_walkers, NN = (1 << td.depth) - 1, NO = td.derive_mode == 2 ? 1 : (1 << td.depth);
        const int writers = W;                                   // (prologue: the step-table workgroups)
        const int n_derive = td.derive_mode == 0 ? 0 : W * NO * NN * NPOPS * derive_parts;
        const int heavy = td.levels > 0 ? W * NN * td.heavy_parts : 0;
        const int front = (writers + n_derive + heavy + 7) / 8 * 8;
        const int hot = td.levels > 0 ? 8 * ((td.n_groups * NPOPS + 7) / 8) * W * NN : 0;
        hipLaunchKernelGGL(k.kern, dim3(front + hot), dim3(256), k.lds, stream, pk, st, td, pr, group_tiles, front, derive_parts);
        return hipGetLastError();
    });
}

hipError_t b9k_tree_finish(const TreeDev &td, const DevPriors &pr, hipStream_t stream)
{
    hipLaunchKernelGGL(tree_large(td.n_groups) ? tree_kd5::k_tree_finish : tree_kd3::k_tree_finish, dim3(td.n_walkers), dim3(256), 0, stream, td, pr);
    return hipGetLastError();
}

hipError_t b9k_tree_begin(const double *host_up, double *dev, int up_words, const double *prev_final, double *state, int n_walkers, hipStream_t stream)
{
    hipLaunchKernelGGL(tree_kd3::k_tree_begin, dim3(1), dim3(256), 0, stream, host_up, dev, up_words, prev_final, state, n_walkers);
    return hipGetLastError();
}

hipError_t b9k_mcmc_begin(const double *host_up, double *dev, int up_words, const double *prev_final, double *cur0, double *lp0,
                          double *state0, int n_walkers, hipStream_t stream)
{
    hipLaunchKernelGGL(k_mcmc_begin, dim3(1), dim3(256), 0, stream, host_up, dev, up_words, prev_final, cur0, lp0, state0, n_walkers);
    return hipGetLastError();
}

hipError_t b9k_mcmc_finish(const DevPack &pk, const StepDev &sd, const DevPriors &pr, hipStream_t stream)
{
    hipLaunchKernelGGL(k_mcmc_finish, dim3(sd.n_walkers), dim3(256), 0, stream, pk, sd, pr);
    return hipGetLastError();
}

hipError_t b9k_chain_rows(const StepDev &sd, const double *cur_fin, const double *lp_fin, hipStream_t stream)
{
    hipLaunchKernelGGL(k_chain_rows, dim3(sd.n_walkers), dim3(256), 0, stream, sd, cur_fin, lp_fin);
    return hipGetLastError();
}

// An empty kernel: bracketing it with HIP events measures what an event bracket adds to a kernel's
// own duration (dispatch boundary + event processing); b9_calibrate_timing subtracts nothing by
// itself, it only reports the figure.
__global__ void k_noop(int *p) { if (p && threadIdx.x == 1024) *p = 0; }
// keeps the queue busy for ~`ticks` s_memrealtime ticks (100 MHz) so that work enqueued behind it
// executes back to back (bounded spin; one wave)
__global__ void k_spin(unsigned long long ticks, int *p)
{
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    int guard = 0;
    while (__builtin_amdgcn_s_memrealtime() - t0 < ticks && guard < (1 << 24)) ++guard;
    if (p && guard < 0) *p = guard;
}
hipError_t b9k_spin(double microseconds, hipStream_t stream)
{
    hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, stream, (unsigned long long)(microseconds * 100.0), (int *)nullptr);
    return hipGetLastError();
}
hipError_t b9k_noop(hipStream_t stream)
{
    hipLaunchKernelGGL(k_noop, dim3(1), dim3(64), 0, stream, (int *)nullptr);
    return hipGetLastError();
}

// (shader-cycle counter, 100 MHz reference counter) stamped per COMPUTE UNIT by whichever of the launch's workgroups landed
// there: two such stamps bracket a stretch of stream work, and delta(s_memtime) / delta(s_memrealtime) x 100 MHz of one CU
// is the clock its shader engine actually ran at over it (MI355X_MICROARCH.md: the in-kernel clock, not pp_dpm_sclk).
// The cycle counters of different CUs are offset against each other by arbitrary amounts (measured: tens of millions of
// cycles), so a difference is only ever formed between two stamps of the SAME CU.  out[cu slot] = {t, tr}.
__global__ void k_clock_stamp(unsigned long long *out)
{
    if (threadIdx.x != 0) return;
    unsigned xcc, hw;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    unsigned long long t, tr;
    asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(t), "=s"(tr) :: "memory");
    const unsigned slot = ((xcc & 7u) << 8) | ((hw >> 8) & 0xFFu);      // HW_ID[15:8] = shader engine, shader array, CU
    // several workgroups land on one CU: the FIRST to claim the (zeroed) slot writes both words, so a pair is one workgroup's
    if (atomicCAS(out + 2 * slot, 0ull, t) == 0ull) out[2 * slot + 1] = tr;
}
hipError_t b9k_clock_stamp(unsigned long long *d_out, hipStream_t stream)
{
    hipLaunchKernelGGL(k_clock_stamp, dim3(2048), dim3(64), 0, stream, d_out);
    return hipGetLastError();
}
