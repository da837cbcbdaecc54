// b9_capi_eval.cpp -- one log-posterior evaluation through the C ABI: derive -> stars -> finalize (b9_logpost,
// b9_logpost_device), the per-star mass draws (b9_sample_mass), the isochrone dump (b9_derive_isochrone) and the forward
// model alone (b9_predict_mags); the reductions over a saved chain through chain_reduce -- the per-star posterior moments
// (b9_star_moments), the binned mass posteriors (b9_mass_hist), the per-star bins (b9_star_bins), the posterior-predictive
// residuals (b9_phot_resid), the leave-one-filter-out predictions (b9_filter_loo), the per-star offsets (b9_star_offset), the pointwise predictive densities
// (b9_pointwise) and the star influence (b9_star_influence) --; and the three calls on a WD mass grid of the
// caller's own size through wd_grid_reduce -- the WD-stage stars' posterior draws (b9_sample_wd_mass), their exact posterior
// moments (b9_wd_moments) and their per-line bins (b9_wd_bins); and the loci a saved chain implies in the CMD (b9_cmd_band: a pack,
// no stars, its own driver and arena).  Every launch wrapper takes its derived isochrone set as one
// view (B9IsoSet, b9_launch.h): buffer_set hands out the context's, b9_predict_mags and the two drivers build theirs where they
// carve their buffers.  A driver fills what its call works on once (ChainDev : B9Chain, WdGridDev : B9WdGrid) and a body hands
// it to its wrapper whole, with the chunk's row count and the call's own few arguments.
#include "b9_ctx.h"
#include <algorithm>
#include <cmath>
#include <atomic>
#include <functional>
#include <string>
#include <vector>

using namespace b9i;

namespace b9i {

// ping-pong work-buffer set (0 / 1) of the context's populations: the sets lie cap_walkers rows of cap_pops populations apart
B9IsoSet buffer_set(const b9_ctx *ctx, int set)
{
    const B9IsoSet all{ctx->work.params.get(), ctx->work.hdr.get(), ctx->work.iso.get(), ctx->work.iso_stride, ctx->work.mass_cap, ctx->work.cap_pops};
    B9IsoSet s = all.at((size_t)set * ctx->work.cap_walkers);
    s.n_pops = ctx->opt.n_pops;
    return s;
}

// the context's marginalisation grid and node tables (ensure_marg_table)
B9Marg marg_tables(const b9_ctx *ctx)
{
    return B9Marg{marg_grid(ctx).K, marg_grid(ctx).Q, ctx->marg_prune, ctx->d_marg_tab.get(), ctx->d_marg_wd_tab.get(), ctx->d_marg_shares.get()};
}

// number of partial sums one walker gets from the star kernel under the current plan / mode
// (marginalised mode: one per 64-star chunk -- the star kernel sums a chunk's values in a fixed order -- and one per four WD-stage stars)
int partial_count(const b9_ctx *ctx, const B9Groups &plan)
{
    return ctx->opt.mode == B9_MODE_MARGINALISED ? ctx->st.mg_pad / 64 + (ctx->st.n_wd + 3) / 4 : plan.n_groups * 4 + ctx->heavy_parts;
}

// doubles between two walkers' partial rows (room for either mode's row)
long long partial_stride(const b9_ctx *ctx) { return (long long)ctx->st.n_pad + ctx->st.n_pad / 64; }

// the context's partial sums under the current plan / mode (after ensure_capacity)
B9Partial partials(const b9_ctx *ctx, const B9Groups &plan) { return B9Partial{ctx->d_partial.get(), partial_count(ctx, plan), partial_stride(ctx)}; }

// The star-likelihood launch (given-mass: hot + heavy workgroups; marginalised: one wave per star)
// on buffer set `set`, bracketed by timing events when sampled.
int launch_stars(b9_ctx *ctx, const B9IsoSet &bf, int32_t n_walkers, double *d_perstar, const B9Groups &plan,
                        hipStream_t stream)
{
    TimingBracket tb;
    int rc = bracket_before(ctx, stream, tb);
    if (rc) return rc;
    if (ctx->opt.mode == B9_MODE_MARGINALISED) {
        rc = ensure_marg_table(ctx, n_walkers, bf.n_pops, marg_grid(ctx).K, marg_grid(ctx).Q);
        if (rc) return rc;
        HIPCHK(ctx, b9k_star_marg(ctx->pk, ctx->st, bf, n_walkers, partials(ctx, plan), d_perstar, marg_tables(ctx), nullptr, ctx->n_cu, stream));
    } else {
        HIPCHK(ctx, b9k_star_like(ctx->pk, ctx->st, bf, n_walkers, partials(ctx, plan), d_perstar, plan, ctx->heavy_parts, stream));
    }
    return bracket_after(ctx, stream, tb, true);
}

}  // namespace b9i

namespace {

// One log-posterior evaluation of rows that are already in buffer set 0's parameter rows (or in
// d_params when that is a caller's device pointer): derive -> stars -> finalize.
int launch_logpost(b9_ctx *ctx, double *d_params, int32_t n_walkers, double *d_logpost,
                          double *d_perstar, hipStream_t stream, const double *host_rows = nullptr,
                          unsigned long long *done_flag = nullptr, unsigned long long done_seq = 0)
{
    const int n_pops = ctx->opt.n_pops;
    // (the buffers first: the canonical tile groups key on mass_cap, which ensure_capacity brings up to the loaded pack -- a
    //  plan made before it would follow whatever pack the context held before, or none)
    int rc = ensure_capacity(ctx, n_walkers, n_pops, (size_t)partial_stride(ctx) * n_walkers, false);
    if (rc) return rc;
    const B9Groups plan = make_plan(ctx, n_walkers, n_pops);
    B9IsoSet bf = buffer_set(ctx, 0);
    bf.params = d_params;
    const McmcDev off{};
    if (host_rows)      // <= 8 rows travel in the kernel arguments: no upload
        HIPCHK(ctx, b9k_derive_iso_rows(ctx->pk, host_rows, bf, n_walkers, stream));
    else
        HIPCHK(ctx, b9k_derive_iso(ctx->pk, bf, n_walkers, off, ctx->pr, no_prev(), stream));
    rc = launch_stars(ctx, bf, n_walkers, d_perstar, plan, stream);
    if (rc) return rc;
    HIPCHK(ctx, b9k_finalize(bf, partials(ctx, plan), ctx->pr, n_walkers, d_logpost, d_perstar, ctx->st.n, off, stream, done_flag, done_seq));
    return B9_OK;
}

}  // namespace

extern "C" {

int b9_logpost_device(b9_ctx *ctx, const double *d_params, int32_t n_walkers, double *d_logpost,
                      double *d_perstar, void *stream_v)
{
    if (!ctx || !d_params || !d_logpost || n_walkers < 1) return B9_ERR_INVALID;
    if (block_outstanding(ctx)) return fail(ctx, B9_ERR_STATE, kBlockOutstanding);
    int rc = check_ready(ctx);
    if (rc) return rc;
    hipStream_t stream = stream_v ? static_cast<hipStream_t>(stream_v) : ctx->stream;
    return launch_logpost(ctx, const_cast<double *>(d_params), n_walkers, d_logpost, d_perstar, stream);
}

int b9_logpost(b9_ctx *ctx, const double *params, int32_t n_walkers, double *out_logpost, double *out_perstar)
{
    if (!ctx || !params || !out_logpost || n_walkers < 1) return B9_ERR_INVALID;
    if (block_outstanding(ctx)) return fail(ctx, B9_ERR_STATE, kBlockOutstanding);
    int rc = check_ready(ctx);
    if (rc) return rc;
    rc = ensure_capacity(ctx, n_walkers, ctx->opt.n_pops, (size_t)partial_stride(ctx) * n_walkers, out_perstar != nullptr);
    if (rc) return rc;
    // The per-step call of a host-driven sampler (the reference's logPostStep) is latency: for up
    // to 8 rows the parameters ride in the first launch's kernel arguments and the log-posteriors are written by
    // k_finalize straight into pinned host memory mapped into the device -- no copy command in the stream at all.
    {
        const Reserved r = ctx->h_lp.reserve(16);
        if (r.err) return alloc_failed(ctx, named(r, "ctx->h_lp"));
        if (r.fresh) std::memset(ctx->h_lp.get(), 0, sizeof(double) * 16);
    }
    const bool small = n_walkers <= 8;
    // ... and the host does not wait for the stream's completion signal either (a wake-up of several microseconds): the
    // last launch stores a per-call sequence number behind every log-posterior and the host polls those words
    volatile unsigned long long *const h_done = reinterpret_cast<volatile unsigned long long *>(ctx->h_lp.get() + 8);
    const bool polled = small && !out_perstar;
    const unsigned long long seq = ++ctx->lp_seq;
    if (small) {
        rc = launch_logpost(ctx, ctx->work.params.get(), n_walkers, ctx->h_lp.dev(), out_perstar ? ctx->d_perstar.get() : nullptr, ctx->stream, params,
                            polled ? reinterpret_cast<unsigned long long *>(ctx->h_lp.dev() + 8) : nullptr, seq);
        if (rc) return rc;
    } else {
        HIPCHK(ctx, hipMemcpyAsync(ctx->work.params.get(), params, sizeof(double) * B9_NPARAM * n_walkers, hipMemcpyHostToDevice, ctx->stream));
        rc = b9_logpost_device(ctx, ctx->work.params.get(), n_walkers, ctx->work.logpost.get(), out_perstar ? ctx->d_perstar.get() : nullptr, ctx->stream);
        if (rc) return rc;
        HIPCHK(ctx, hipMemcpyAsync(out_logpost, ctx->work.logpost.get(), sizeof(double) * n_walkers, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (out_perstar)
        HIPCHK(ctx, hipMemcpyAsync(out_perstar, ctx->d_perstar.get(), sizeof(double) * (size_t)n_walkers * ctx->st.n,
                                   hipMemcpyDeviceToHost, ctx->stream));
    if (polled) {
        // (bounded: a launch that failed never stores its words -- after ~2 ms the stream's own wait takes over and reports)
        bool done = false;
        for (long spin = 0; spin < 2000000 && !done; ++spin) {
            done = true;
            for (int w = 0; w < n_walkers; ++w) done = done && h_done[w] == seq;
            if (!done) __builtin_ia32_pause();
        }
        if (!done) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        std::atomic_thread_fence(std::memory_order_acquire);
    } else {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (small) std::memcpy(out_logpost, ctx->h_lp.get(), sizeof(double) * n_walkers);
    return B9_OK;
}

int b9_sample_mass(b9_ctx *ctx, const double *params, int32_t n_rows, uint64_t seed, int64_t row0,
                   double *out_mass, double *out_ratio, double *out_member, int32_t *out_pop)
{
    if (!ctx || !params || n_rows < 1 || !out_mass || !out_ratio || !out_member) return B9_ERR_INVALID;
    if (block_outstanding(ctx)) return fail(ctx, B9_ERR_STATE, kBlockOutstanding);
    int rc = check_ready(ctx);
    if (rc) return rc;
    const int n_pops = ctx->opt.n_pops, n = ctx->st.n;
    const int K = marg_grid(ctx).K, Q = marg_grid(ctx).Q;
    const int chunk = std::min<int>(n_rows, 32);
    rc = ensure_capacity(ctx, chunk, n_pops, (size_t)partial_stride(ctx) * chunk, false);
    if (rc) return rc;
    rc = ensure_marg_table(ctx, chunk, n_pops, K, Q);
    if (rc) return rc;
    // (allocated per call and released at return: at 50k stars the draws of a chunk are ~45 MB)
    const size_t per = (size_t)chunk * n;
    DeviceBuf<double> out;
    DeviceBuf<int> pop;
    RESERVE(ctx, out, per * 3);
    if (out_pop) RESERVE(ctx, pop, per);
    double *const d_out = out.get();
    int *const d_pop = pop.get();
    hipStream_t s = ctx->stream;
    const B9IsoSet bf = buffer_set(ctx, 0);
    const B9Partial part{ctx->d_partial.get(), 0, partial_stride(ctx)};
    const McmcDev off{};
    for (int r0 = 0; r0 < n_rows; r0 += chunk) {
        const int m = std::min(chunk, n_rows - r0);
        HIPCHK(ctx, hipMemcpyAsync(bf.params, params + (size_t)r0 * B9_NPARAM, sizeof(double) * B9_NPARAM * m, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemsetAsync(d_out, 0, sizeof(double) * per * 3, s));     // rows outside the grid write nothing
        if (d_pop) HIPCHK(ctx, hipMemsetAsync(d_pop, 0, sizeof(int) * per, s));
        HIPCHK(ctx, b9k_derive_iso(ctx->pk, bf, m, off, ctx->pr, no_prev(), s));
        B9MargSample smp{d_out, d_out + per, d_out + 2 * per, d_pop, 0, 0, (long long)(row0 + r0)};
        split_seed(seed, &smp.k0, &smp.k1);
        // the kernel indexes its outputs [row][n_stars] with the launch's own row count: rows are contiguous for any m
        HIPCHK(ctx, b9k_star_marg(ctx->pk, ctx->st, bf, m, part, nullptr, marg_tables(ctx), &smp, ctx->n_cu, s));
        const size_t cnt = (size_t)m * n, o = (size_t)r0 * n;
        HIPCHK(ctx, hipMemcpyAsync(out_mass + o, d_out, sizeof(double) * cnt, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(out_ratio + o, d_out + per, sizeof(double) * cnt, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipMemcpyAsync(out_member + o, d_out + 2 * per, sizeof(double) * cnt, hipMemcpyDeviceToHost, s));
        if (d_pop) HIPCHK(ctx, hipMemcpyAsync(out_pop + o, d_pop, sizeof(int) * cnt, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
    }
    return B9_OK;
}

int b9_derive_isochrone(b9_ctx *ctx, const double *param_row, int32_t pop, int32_t cap, double *out_mass,
                        double *out_mags, int32_t *out_first_eep, int32_t *out_n, double *out_agb_tip)
{
    if (!ctx || !param_row || !out_mass || !out_mags || !out_first_eep || !out_n || !out_agb_tip) return B9_ERR_INVALID;
    if (!ctx->have_pack) return fail(ctx, B9_ERR_STATE, "load the pack first");
    if (block_outstanding(ctx)) return fail(ctx, B9_ERR_STATE, kBlockOutstanding);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = ensure_capacity(ctx, 1, 1, 1, false);
    if (rc) return rc;
    double row[B9_NPARAM];
    std::memcpy(row, param_row, sizeof row);
    if (pop) row[B9_P_Y] = row[B9_P_Y2];
    HIPCHK(ctx, hipMemcpyAsync(ctx->work.params.get(), row, sizeof row, hipMemcpyHostToDevice, ctx->stream));
    B9IsoSet one = buffer_set(ctx, 0);
    one.n_pops = 1;
    HIPCHK(ctx, b9k_derive_iso(ctx->pk, one, 1, McmcDev{}, ctx->pr, no_prev(), ctx->stream));
    IsoHdr h;
    HIPCHK(ctx, hipMemcpyAsync(&h, ctx->work.hdr.get(), sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *out_n = 0; *out_first_eep = 0; *out_agb_tip = 0.0;
    if (!h.valid) return B9_OK;
    if (h.n > cap) return fail(ctx, B9_ERR_CAPACITY, "isochrone longer than the caller's buffers");
    const int nf = ctx->pk.nf, nfp = ctx->pk.nfp;
    std::vector<double> buf((size_t)h.n * nfp);
    HIPCHK(ctx, hipMemcpy(out_mass, ctx->work.iso.get(), sizeof(double) * h.n, hipMemcpyDeviceToHost));
    HIPCHK(ctx, hipMemcpy(buf.data(), ctx->work.iso.get() + ctx->work.mass_cap, sizeof(double) * buf.size(), hipMemcpyDeviceToHost));
    for (int e = 0; e < h.n; ++e) std::memcpy(&out_mags[(size_t)e * nf], &buf[(size_t)e * nfp], sizeof(double) * nf);
    *out_n = h.n; *out_first_eep = h.first_eep; *out_agb_tip = h.agb_tip;
    return B9_OK;
}

int b9_predict_mags(b9_ctx *ctx, const double *param_row, int64_t n, const double *mass1, const double *mass_ratio,
                    const int32_t *wd_type, const int32_t *pop, double *out_mags, int32_t *out_stage)
{
    if (!ctx || !param_row || n < 0 || (n > 0 && (!mass1 || !mass_ratio || !out_mags))) return B9_ERR_INVALID;
    if (!ctx->have_pack) return fail(ctx, B9_ERR_STATE, "load the pack first");
    if (block_outstanding(ctx)) return fail(ctx, B9_ERR_STATE, kBlockOutstanding);
    int n_pops = 1;
    for (int64_t i = 0; i < n; ++i) {
        if (!std::isfinite(mass1[i]) || !std::isfinite(mass_ratio[i]) || mass_ratio[i] < 0.0)
            return fail(ctx, B9_ERR_INVALID, "b9_predict_mags: system " + std::to_string(i) + " has a non-finite mass or a negative mass ratio");
        if (pop && (pop[i] < 0 || pop[i] > 1)) return fail(ctx, B9_ERR_INVALID, "b9_predict_mags: a population is 0 or 1");
        if (pop && pop[i] == 1) n_pops = 2;        // the second isochrone is derived only when some system needs it
    }
    if (n == 0) return B9_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const DevPack &pk = ctx->pk;
    const int nf = pk.nf;
    B9IsoSet set{nullptr, nullptr, nullptr, 0, pack_mass_cap(pk.max_eep), n_pops};
    set.iso_stride = pack_iso_stride(set.mass_cap, pk.nfp);
    if (b9k_predict_lds(pk.nfp, set.mass_cap, n_pops) > B9_LDS_PER_CU)
        return fail(ctx, B9_ERR_CAPACITY, "b9_predict_mags: the derived isochrones do not fit the kernel's LDS");
    RESERVE(ctx, ctx->d_pred_hdr, 2);
    RESERVE(ctx, ctx->d_pred_par, B9_NPARAM);
    RESERVE(ctx, ctx->d_pred_iso, (size_t)(2 * set.iso_stride));
    set.params = ctx->d_pred_par.get(); set.hdr = ctx->d_pred_hdr.get(); set.iso = ctx->d_pred_iso.get();
    // systems in chunks of at most 2^20 (every system's result depends on that system alone, so the chunking is invisible)
    const int64_t chunk = std::min<int64_t>(n, (int64_t)1 << 20);
    const PredArena a = pred_arena((size_t)chunk, nf);
    RESERVE(ctx, ctx->d_pred_io, a.bytes);
    char *io = ctx->d_pred_io.get();
    double *d_m1 = part<double>(io, a.o_m1), *d_q = part<double>(io, a.o_q), *d_mags = part<double>(io, a.o_mags);
    int *d_wd = part<int>(io, a.o_wd), *d_pop = part<int>(io, a.o_pop), *d_stage = part<int>(io, a.o_stage);
    hipStream_t s = ctx->stream;
    HIPCHK(ctx, b9k_derive_iso_rows(pk, param_row, set, 1, s));
    for (int64_t i0 = 0; i0 < n; i0 += chunk) {
        const int64_t m = std::min(chunk, n - i0);
        HIPCHK(ctx, hipMemcpyAsync(d_m1, mass1 + i0, sizeof(double) * m, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(d_q, mass_ratio + i0, sizeof(double) * m, hipMemcpyHostToDevice, s));
        if (wd_type) HIPCHK(ctx, hipMemcpyAsync(d_wd, wd_type + i0, sizeof(int) * m, hipMemcpyHostToDevice, s));
        if (pop) HIPCHK(ctx, hipMemcpyAsync(d_pop, pop + i0, sizeof(int) * m, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, b9k_predict_mags(pk, set, m, d_m1, d_q, wd_type ? d_wd : nullptr, pop ? d_pop : nullptr, d_mags, d_stage, 4 * ctx->n_cu, s));
        HIPCHK(ctx, hipMemcpyAsync(out_mags + (size_t)i0 * nf, d_mags, sizeof(double) * m * nf, hipMemcpyDeviceToHost, s));
        if (out_stage) HIPCHK(ctx, hipMemcpyAsync(out_stage + i0, d_stage, sizeof(int) * m, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));      // (the host arrays of the next chunk reuse the same device buffers)
    }
    return B9_OK;
}

// ---- b9_cmd_band: the loci a saved chain's rows imply, reduced over the rows line by line; a pack, no stars ------------------
#define B9_BAND_TABLE_BYTES ((size_t)64 << 20)
#define B9_BAND_MAX_ROWS 256

int b9_cmd_band(b9_ctx *ctx, const double *params, int32_t n_rows, const b9_band_spec *spec, int32_t flags, const double *pivot, double *mom,
                const double *edges, int32_t n_bins, double *bins)
{
    if (!ctx || !params || !spec || n_rows < 1 || (!mom && !bins)) return B9_ERR_INVALID;
    if (!ctx->have_pack) return fail(ctx, B9_ERR_STATE, "load the pack first");
    if (block_outstanding(ctx)) return fail(ctx, B9_ERR_STATE, kBlockOutstanding);
    const DevPack &pk = ctx->pk;
    const int nf = pk.nf;
    if (spec->n_eep < 0 || spec->n_ratio < 0 || spec->n_ratio > B9_BAND_MAX_RATIOS || (spec->n_ratio > 0 && !spec->ratio))
        return fail(ctx, B9_ERR_INVALID, "b9_cmd_band: n_eep must not be negative and n_ratio must lie in 0 .. B9_BAND_MAX_RATIOS");
    for (int s = 0; s < spec->n_ratio; ++s)
        if (!std::isfinite(spec->ratio[s]) || spec->ratio[s] < 0.0 || spec->ratio[s] > 1.0) return fail(ctx, B9_ERR_INVALID, "b9_cmd_band: a mass ratio lies in [0, 1]");
    if (spec->n_eep > 0 && spec->n_ratio == 0) return fail(ctx, B9_ERR_INVALID, "b9_cmd_band: MS/RGB points need a mass ratio");
    if (spec->n_wd_nodes < 0 || (spec->n_wd_nodes > 0 && (spec->wd_types < 1 || spec->wd_types > 3)))
        return fail(ctx, B9_ERR_INVALID, "b9_cmd_band: n_wd_nodes must not be negative and wd_types selects DA (1), DB (2) or both (3)");
    if (spec->n_colour < 0 || spec->n_colour > B9_BAND_MAX_COLOURS || (spec->n_colour > 0 && !spec->colour))
        return fail(ctx, B9_ERR_INVALID, "b9_cmd_band: n_colour must lie in 0 .. B9_BAND_MAX_COLOURS");
    for (int c = 0; c < 2 * spec->n_colour; ++c)
        if (spec->colour[c] < 0 || spec->colour[c] >= nf || spec->colour[c | 1] == spec->colour[c & ~1])
            return fail(ctx, B9_ERR_INVALID, "b9_cmd_band: a colour takes two different filters of the pack");
    B9Band b{};
    B9BandSpec &sp = b.spec;
    B9IsoSet &set = b.set;
    set.n_pops = ctx->opt.n_pops == 2 ? 2 : 1;
    sp.eep0 = spec->eep0; sp.n_eep = spec->n_eep; sp.n_ratio = spec->n_ratio; sp.n_wd_nodes = spec->n_wd_nodes; sp.n_colour = spec->n_colour;
    for (int s = 0; s < sp.n_ratio; ++s) sp.ratio[s] = spec->ratio[s];
    for (int c = 0; c < sp.n_colour; ++c) { sp.colour[c][0] = spec->colour[2 * c]; sp.colour[c][1] = spec->colour[2 * c + 1]; }
    if (sp.n_wd_nodes > 0)
        for (int t = 0; t < 2; ++t) if (spec->wd_types >> t & 1) sp.type_id[sp.n_types++] = t;
    const size_t P = (size_t)sp.n_ratio * sp.n_eep + (size_t)sp.n_types * sp.n_wd_nodes, C = 1 + (size_t)nf + sp.n_colour;
    const size_t n_lines = (size_t)set.n_pops * P * C;
    if (P == 0) return fail(ctx, B9_ERR_INVALID, "b9_cmd_band: the spec has no lines");
    if (P > (size_t)1 << 28) return fail(ctx, B9_ERR_CAPACITY, "b9_cmd_band: too many points");
    sp.P = (int)P; sp.C = (int)C; sp.n_lines = (long long)n_lines;
    const size_t ne = (size_t)n_bins + 1, nbc = (size_t)n_bins + 3;
    if (bins) {
        if (!edges) return fail(ctx, B9_ERR_INVALID, "b9_cmd_band: bins need edges");
        if (n_bins < 1 || n_bins > B9_BAND_MAX_BINS) return fail(ctx, B9_ERR_INVALID, "b9_cmd_band: n_bins must lie in 1 .. B9_BAND_MAX_BINS");
        for (size_t l = 0; l < n_lines; ++l)
            for (size_t e = 0; e < ne; ++e)
                if (!std::isfinite(edges[l * ne + e]) || (e > 0 && !(edges[l * ne + e] > edges[l * ne + e - 1])))
                    return fail(ctx, B9_ERR_INVALID, "b9_cmd_band: line " + std::to_string(l) + ": the edges must be finite and strictly ascending");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    set.mass_cap = pack_mass_cap(pk.max_eep); set.iso_stride = pack_iso_stride(set.mass_cap, pk.nfp);
    // rows of a chunk: at most B9_BAND_MAX_ROWS, and as few as keep the value table and the WD node table within 64 MiB each
    const size_t tab_row = sp.n_types ? (size_t)set.n_pops * (size_t)b9k_wd_grid_table_doubles(pk.nfp, sp.n_wd_nodes, true) : 0;
    if (std::max(tab_row, n_lines) > ((size_t)8 << 30) / sizeof(double)) return fail(ctx, B9_ERR_CAPACITY, "b9_cmd_band: one row's tables would exceed 8 GiB");
    // ... and so does the lines' own state: pivot, moments, bin words, edges
    if (n_lines > ((size_t)8 << 30) / sizeof(double) / (1 + B9_BAND_NMOM + (bins ? nbc + ne : 0)))
        return fail(ctx, B9_ERR_CAPACITY, "b9_cmd_band: the lines' pivots, moments, bins and edges would exceed 8 GiB");
    size_t chunk = std::min<size_t>({(size_t)n_rows, (size_t)B9_BAND_MAX_ROWS, B9_BAND_TABLE_BYTES / (n_lines * sizeof(double))});
    if (tab_row) chunk = std::min(chunk, B9_BAND_TABLE_BYTES / (tab_row * sizeof(double)));
    chunk = std::max<size_t>(1, chunk);
    const BandArena a = band_arena(chunk, set.n_pops, set.iso_stride, tab_row, n_lines, mom ? B9_BAND_NMOM : 0, bins ? nbc : 0, bins ? ne : 0, sizeof(IsoHdr));
    RESERVE(ctx, ctx->d_band, a.bytes);
    char *base = ctx->d_band.get();
    set.params = part<double>(base, a.o_par); set.hdr = part<IsoHdr>(base, a.o_hdr); set.iso = part<double>(base, a.o_iso);
    b.wd_tab = tab_row ? part<double>(base, a.o_tab) : nullptr; b.values = part<double>(base, a.o_values); b.pivot = part<double>(base, a.o_pivot);
    b.mom = mom ? part<double>(base, a.o_mom) : nullptr; b.bins = bins ? part<double>(base, a.o_bins) : nullptr;
    b.edges_t = bins ? part<double>(base, a.o_edges) : nullptr; b.n_bins = bins ? n_bins : 0;
    // the uploads' sources (they live until the wait below): the starting state when the call does not continue, the edges [b][line]
    const bool cont = (flags & B9_BAND_CONTINUE) != 0;
    std::vector<double> mom0, edges_t;
    hipStream_t s = ctx->stream;
    const auto enqueue = [&]() -> int {
        if (pivot) HIPCHK(ctx, hipMemcpyAsync(b.pivot, pivot, sizeof(double) * n_lines, hipMemcpyHostToDevice, s));
        else HIPCHK(ctx, hipMemsetAsync(b.pivot, 0, sizeof(double) * n_lines, s));
        if (mom) {
            if (!cont) {
                mom0.assign(n_lines * B9_BAND_NMOM, 0.0);
                for (size_t l = 0; l < n_lines; ++l) { mom0[l * B9_BAND_NMOM + B9_BAND_MIN] = INFINITY; mom0[l * B9_BAND_NMOM + B9_BAND_MAX] = -INFINITY; }
            }
            HIPCHK(ctx, hipMemcpyAsync(b.mom, cont ? mom : mom0.data(), sizeof(double) * n_lines * B9_BAND_NMOM, hipMemcpyHostToDevice, s));
        }
        if (bins) {
            if (cont) HIPCHK(ctx, hipMemcpyAsync(b.bins, bins, sizeof(double) * n_lines * nbc, hipMemcpyHostToDevice, s));
            else HIPCHK(ctx, hipMemsetAsync(b.bins, 0, sizeof(double) * n_lines * nbc, s));
            edges_t.resize(n_lines * ne);
            for (size_t l = 0; l < n_lines; ++l)
                for (size_t e = 0; e < ne; ++e) edges_t[e * n_lines + l] = edges[l * ne + e];
            HIPCHK(ctx, hipMemcpyAsync(b.edges_t, edges_t.data(), sizeof(double) * n_lines * ne, hipMemcpyHostToDevice, s));
        }
        const McmcDev off{};
        for (int r0 = 0; r0 < n_rows; r0 += (int)chunk) {
            const int m = std::min((int)chunk, n_rows - r0);
            HIPCHK(ctx, hipMemcpyAsync(set.params, params + (size_t)r0 * B9_NPARAM, sizeof(double) * B9_NPARAM * m, hipMemcpyHostToDevice, s));
            HIPCHK(ctx, b9k_derive_iso(pk, set, m, off, ctx->pr, no_prev(), s));
            HIPCHK(ctx, b9k_cmd_band(pk, b, m, s));
        }
        // (the outputs leave only after everything has succeeded so far: a failed launch leaves them untouched)
        if (mom) HIPCHK(ctx, hipMemcpyAsync(mom, b.mom, sizeof(double) * n_lines * B9_BAND_NMOM, hipMemcpyDeviceToHost, s));
        if (bins) HIPCHK(ctx, hipMemcpyAsync(bins, b.bins, sizeof(double) * n_lines * nbc, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));
        return B9_OK;
    };
    // (a failure part-way: nothing may still be reading mom0 / edges_t when they go out of scope; the call's error stays in ctx->err)
    const int rc = enqueue();
    if (rc) (void)hipStreamSynchronize(s);
    return rc;
}

int b9_n_wd_stars(const b9_ctx *ctx)
{
    if (!ctx) return B9_ERR_INVALID;
    if (!ctx->have_stars) return B9_ERR_STATE;
    return ctx->n_wd_stage;
}

}  // extern "C"

namespace {

// ---- the reductions over a saved chain: b9_star_moments, b9_mass_hist, b9_star_bins, b9_phot_resid, b9_filter_loo, b9_star_offset, b9_pointwise,
// b9_star_influence
// What one of them is to the driver below.  Rows are worked in chunks of at most max_rows, and of as few rows as keep the chunk's
// increments [rows][n_stars][n_col] within scratch_bytes.
struct ChainCall {
    const char *name;
    size_t n_col, n_acc, n_rowcol;       // increments per (row, star); accumulator words per star; words of a row's sums
    size_t max_rows, scratch_bytes;
    bool cont;                           // the call's CONTINUE flag: acc comes in
    double *acc, *rows;                  // host: the per-star accumulators [n_stars][n_acc], the per-row sums [n_rows][n_rowcol] (null: not asked for)
    size_t extra_bytes[kChainExtras];    // the call's own parts of the arena
};
// ... and what the call's hooks see: the arena's parts as the launch wrappers take them (B9Chain: acc / rows null when the caller
// did not ask for them; mg.wd_tab without WD-stage stars) and the call's own
struct ChainDev : B9Chain {
    char *extra[kChainExtras];
};
using ChainHook = std::function<int(const ChainDev &)>;
using ChainBody = std::function<hipError_t(const ChainDev &, int /* rows of the chunk */)>;

// The shared checks of the context's state, behind each call's own argument validation.
int chain_ready(b9_ctx *ctx)
{
    if (block_outstanding(ctx)) return fail(ctx, B9_ERR_STATE, kBlockOutstanding);
    if (!ctx->have_pack || !ctx->have_stars) return fail(ctx, B9_ERR_STATE, "load the pack and the stars first");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->stars_dirty) { const int rc = build_stars(ctx); if (rc) return rc; }
    return B9_OK;
}

// The chunked driver (after chain_ready): sizes, one arena in ctx->d_chain, the accumulators in (or cleared), `begin`, then per
// chunk the parameter rows, their isochrones, `body` -- which writes every (row, star) of the chunk, so nothing is cleared -- and
// the chunk's row sums out; at last the accumulators out, `end`, and the wait.  An empty catalogue has all-zero row sums.
int chain_reduce(b9_ctx *ctx, const ChainCall &c, const double *params, int n_rows, const ChainBody &body, const ChainHook &begin = nullptr,
                 const ChainHook &end = nullptr)
{
    const int n = ctx->st.n;
    if (n == 0) {
        if (c.rows) std::fill(c.rows, c.rows + (size_t)n_rows * c.n_rowcol, 0.0);
        return B9_OK;
    }
    const DevPack &pk = ctx->pk;
    ChainDev d{};
    B9IsoSet &set = d.set;
    B9Marg &mg = d.mg;
    set.n_pops = ctx->opt.n_pops == 2 ? 2 : 1; mg.K = marg_grid(ctx).K; mg.Q = marg_grid(ctx).Q; mg.prune = ctx->marg_prune;
    set.mass_cap = pack_mass_cap(pk.max_eep); set.iso_stride = pack_iso_stride(set.mass_cap, pk.nfp);
    const size_t tab_row = (size_t)set.n_pops * (size_t)b9k_marg_table_doubles(pk.nfp, set.mass_cap, mg.K, mg.Q);
    const size_t wd_row = ctx->st.n_wd > 0 ? (size_t)set.n_pops * (size_t)b9k_marg_wd_table_doubles(pk.nfp, mg.K) : 0;
    const size_t chunk = mom_chunk_rows((size_t)n_rows, (size_t)n, c.n_col, c.max_rows, c.scratch_bytes);
    if (chunk * (tab_row + wd_row) > ((size_t)8 << 30) / sizeof(double))
        return fail(ctx, B9_ERR_CAPACITY, std::string(c.name) + ": marginalisation grid too fine: the node tables would exceed 8 GiB");
    const ChainArena a = chain_arena(chunk, set.n_pops, set.iso_stride, tab_row, wd_row, (size_t)n, c.n_col, c.n_acc, c.rows ? c.n_rowcol : 0, sizeof(IsoHdr),
                                     c.extra_bytes);
    RESERVE(ctx, ctx->d_chain, a.bytes);
    char *base = ctx->d_chain.get();
    set.params = part<double>(base, a.o_par); set.hdr = part<IsoHdr>(base, a.o_hdr); set.iso = part<double>(base, a.o_iso); mg.tab = part<double>(base, a.o_tab);
    mg.wd_tab = wd_row ? part<double>(base, a.o_wd) : nullptr; d.scratch = part<double>(base, a.o_scratch);
    d.acc = c.acc ? part<double>(base, a.o_acc) : nullptr; d.rows = c.rows ? part<double>(base, a.o_rows) : nullptr;
    for (int k = 0; k < kChainExtras; ++k) d.extra[k] = base + a.o_extra[k];
    const size_t acc_bytes = sizeof(double) * (size_t)n * c.n_acc;
    hipStream_t s = ctx->stream;
    if (d.acc) {
        if (c.cont) HIPCHK(ctx, hipMemcpyAsync(d.acc, c.acc, acc_bytes, hipMemcpyHostToDevice, s));
        else HIPCHK(ctx, hipMemsetAsync(d.acc, 0, acc_bytes, s));
    }
    if (begin) { const int rc = begin(d); if (rc) return rc; }
    const McmcDev off{};
    for (int r0 = 0; r0 < n_rows; r0 += (int)chunk) {
        const int m = std::min((int)chunk, n_rows - r0);
        HIPCHK(ctx, hipMemcpyAsync(set.params, params + (size_t)r0 * B9_NPARAM, sizeof(double) * B9_NPARAM * m, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, b9k_derive_iso(pk, set, m, off, ctx->pr, no_prev(), s));
        HIPCHK(ctx, body(d, m));
        if (d.rows) HIPCHK(ctx, hipMemcpyAsync(c.rows + (size_t)r0 * c.n_rowcol, d.rows, sizeof(double) * m * c.n_rowcol, hipMemcpyDeviceToHost, s));
    }
    if (d.acc) HIPCHK(ctx, hipMemcpyAsync(c.acc, d.acc, acc_bytes, hipMemcpyDeviceToHost, s));
    if (end) { const int rc = end(d); if (rc) return rc; }
    HIPCHK(ctx, hipStreamSynchronize(s));
    return B9_OK;
}

// ---- the calls on a WD mass grid of the caller's own size: b9_sample_wd_mass, b9_wd_moments, b9_wd_bins ----------------------
// Rows are worked in chunks: at most B9_WDS_MAX_ROWS rows, and as few as keep the chunk's node table within B9_WDS_TABLE_BYTES
// and its words [rows][n_lines][n_col] within the call's scratch_bytes (one row, whatever its size, when that alone is larger).
#define B9_WDS_TABLE_BYTES ((size_t)64 << 20)
#define B9_WDS_MAX_ROWS 256
#define B9_WBIN_SCRATCH_BYTES ((size_t)64 << 20)

// What one of them is to the driver below; a line is a WD-stage star, or for the bins a (WD-stage star, selected quantity).
struct WdGridCall {
    const char *name;
    bool status;                         // the node table keeps every node's status
    size_t lines_per_wd, n_col, n_acc;   // lines per WD-stage star; words per (row, line); accumulator words per line (0: acc null)
    size_t scratch_bytes;                // 0: the table alone limits the chunk
    bool pop;                            // the draws' populations, an int per (row, WD-stage star)
    size_t n_edges;                      // edges per line
    bool cont;                           // the call's CONTINUE flag: acc comes in
    double *acc;                         // host: the accumulators [n_lines][n_acc]
};
// ... and what the call's hooks see: the arena's parts as the launch wrappers take them (B9WdGrid: acc / edges null when the call
// has none) and the driver's own
struct WdGridDev : B9WdGrid {
    int *pop;                            // the draws' populations (null when the call has none)
    int n_wd;
    size_t per;                          // (row, WD-stage star) pairs of a whole chunk
};
using WdGridHook = std::function<int(const WdGridDev &)>;
using WdGridChunk = std::function<int(const WdGridDev &, int /* first row */, int /* rows */)>;
using WdGridBody = std::function<hipError_t(const WdGridDev &, int /* first row */, int /* rows */)>;

// The chunked driver (after chain_ready): sizes, one arena in ctx->d_wds, every star's column up, the accumulators in (or cleared),
// `begin`, then per chunk the parameter rows, their isochrones, `body` and `after`; at last the accumulators out and the wait: a
// chunk's buffers are reused in stream order.  A catalogue without WD-stage stars: nothing is allocated or launched.
int wd_grid_reduce(b9_ctx *ctx, const WdGridCall &c, const double *params, int n_rows, int n_nodes, const WdGridBody &body, const WdGridHook &begin = nullptr,
                   const WdGridChunk &after = nullptr)
{
    const int n = ctx->st.n;
    if (ctx->st.n_wd == 0) return B9_OK;
    const DevPack &pk = ctx->pk;
    WdGridDev d{};
    B9IsoSet &set = d.set;
    d.n_wd = ctx->st.n_wd; d.n_nodes = n_nodes; set.n_pops = ctx->opt.n_pops == 2 ? 2 : 1;
    set.mass_cap = pack_mass_cap(pk.max_eep); set.iso_stride = pack_iso_stride(set.mass_cap, pk.nfp);
    const size_t n_lines = (size_t)d.n_wd * c.lines_per_wd;
    const size_t tab_row = (size_t)set.n_pops * (size_t)b9k_wd_grid_table_doubles(pk.nfp, n_nodes, c.status);       // doubles per row
    if (tab_row > ((size_t)8 << 30) / sizeof(double)) return fail(ctx, B9_ERR_CAPACITY, std::string(c.name) + ": one row's node table would exceed 8 GiB");
    size_t chunk = std::min<size_t>({(size_t)n_rows, (size_t)B9_WDS_MAX_ROWS, B9_WDS_TABLE_BYTES / (tab_row * sizeof(double))});
    if (c.scratch_bytes) chunk = std::min(chunk, c.scratch_bytes / (n_lines * c.n_col * sizeof(double)));
    chunk = std::max<size_t>(1, chunk);
    d.per = chunk * d.n_wd;
    const WdGridArena a = wd_grid_arena(chunk, set.n_pops, set.iso_stride, tab_row, n_lines, (size_t)n, c.n_col, c.n_acc, c.pop ? (size_t)d.n_wd : 0, c.n_edges,
                                        sizeof(IsoHdr));
    RESERVE(ctx, ctx->d_wds, a.bytes);
    char *base = ctx->d_wds.get();
    set.params = part<double>(base, a.o_par); set.hdr = part<IsoHdr>(base, a.o_hdr); set.iso = part<double>(base, a.o_iso); d.tab = part<double>(base, a.o_tab);
    d.scratch = part<double>(base, a.o_scratch); d.acc = c.acc ? part<double>(base, a.o_acc) : nullptr;
    d.pop = c.pop ? part<int>(base, a.o_pop) : nullptr; d.rank = part<int>(base, a.o_rank);
    d.edges = c.n_edges ? part<double>(base, a.o_edges) : nullptr;
    std::vector<int> rank(n);            // wd_rank[star]: the WD-stage stars before it (an upload's source: it lives until the wait below)
    for (int i = 0, k = 0; i < n; ++i) { rank[i] = k; k += ctx->hs.stage[i] == B9_STAGE_WD; }
    hipStream_t s = ctx->stream;
    const size_t acc_bytes = sizeof(double) * n_lines * c.n_acc;
    HIPCHK(ctx, hipMemcpyAsync(d.rank, rank.data(), sizeof(int) * n, hipMemcpyHostToDevice, s));
    if (begin) { const int rc = begin(d); if (rc) return rc; }
    if (d.acc) {
        if (c.cont) HIPCHK(ctx, hipMemcpyAsync(d.acc, c.acc, acc_bytes, hipMemcpyHostToDevice, s));
        else HIPCHK(ctx, hipMemsetAsync(d.acc, 0, acc_bytes, s));
    }
    const McmcDev off{};
    for (int r0 = 0; r0 < n_rows; r0 += (int)chunk) {
        const int m = std::min((int)chunk, n_rows - r0);
        HIPCHK(ctx, hipMemcpyAsync(set.params, params + (size_t)r0 * B9_NPARAM, sizeof(double) * B9_NPARAM * m, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, b9k_derive_iso(pk, set, m, off, ctx->pr, no_prev(), s));
        HIPCHK(ctx, body(d, r0, m));
        if (after) { const int rc = after(d, r0, m); if (rc) return rc; }
    }
    if (d.acc) HIPCHK(ctx, hipMemcpyAsync(c.acc, d.acc, acc_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipStreamSynchronize(s));
    return B9_OK;
}

}  // namespace

#define B9_MOM_SCRATCH_BYTES ((size_t)64 << 20)
#define B9_MOM_MAX_ROWS 32
#define B9_HIST_SCRATCH_BYTES ((size_t)64 << 20)
#define B9_HIST_MAX_ROWS 32
#define B9_SBIN_SCRATCH_BYTES ((size_t)64 << 20)
#define B9_SBIN_MAX_ROWS 32
#define B9_RESID_SCRATCH_BYTES ((size_t)64 << 20)
#define B9_RESID_MAX_ROWS 32
#define B9_LOO_SCRATCH_BYTES ((size_t)64 << 20)
#define B9_LOO_MAX_ROWS 32
#define B9_OFF_SCRATCH_BYTES ((size_t)64 << 20)
#define B9_OFF_MAX_ROWS 32
// (B9_PW_MAX_ROWS: b9_launch.h -- the reducers hold a chunk's rows in registers; 32 rows up to 65536 stars)
#define B9_PW_SCRATCH_BYTES ((size_t)16 << 20)

extern "C" {

int b9_star_moments(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t flags, double *acc)
{
    if (!ctx || !params || !acc || n_rows < 1) return B9_ERR_INVALID;
    if (const int rc = chain_ready(ctx)) return rc;
    const ChainCall c{"b9_star_moments", B9_MOM_N, B9_MOM_N, 0, B9_MOM_MAX_ROWS, B9_MOM_SCRATCH_BYTES, (flags & B9_MOM_CONTINUE) != 0, acc, nullptr, {}};
    return chain_reduce(ctx, c, params, n_rows, [&](const ChainDev &d, int m) {
        return b9k_star_moments(ctx->pk, ctx->st, d, m, ctx->stream);
    });
}

int b9_mass_hist(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t quantity, const double *edges, int32_t n_bins, int32_t flags,
                 double *star_hist, double *row_hist)
{
    if (!ctx || !params || !edges || n_rows < 1 || (!star_hist && !row_hist)) return B9_ERR_INVALID;
    if (quantity != B9_HQ_PRIMARY && quantity != B9_HQ_SECONDARY && quantity != B9_HQ_SYSTEM) return fail(ctx, B9_ERR_INVALID, "b9_mass_hist: unknown quantity");
    if (n_bins < 1 || n_bins > B9_HIST_MAX_BINS) return fail(ctx, B9_ERR_INVALID, "b9_mass_hist: n_bins must lie in 1 .. B9_HIST_MAX_BINS");
    for (int b = 0; b <= n_bins; ++b)
        if (!std::isfinite(edges[b]) || (b > 0 && !(edges[b] > edges[b - 1])))
            return fail(ctx, B9_ERR_INVALID, "b9_mass_hist: the edges must be finite and strictly ascending");
    if (const int rc = chain_ready(ctx)) return rc;
    const size_t ncol = (size_t)n_bins + 1;
    const ChainCall c{"b9_mass_hist", ncol, ncol, ncol, B9_HIST_MAX_ROWS, B9_HIST_SCRATCH_BYTES, (flags & B9_HIST_CONTINUE) != 0, star_hist, row_hist, {}};
    return chain_reduce(ctx, c, params, n_rows, [&](const ChainDev &d, int m) {
        return b9k_mass_hist(ctx->pk, ctx->st, d, m, quantity, edges, n_bins, ctx->stream);
    });
}

int b9_ratio_hist(b9_ctx *ctx, const double *params, int32_t n_rows, const double *mass_edges, int32_t n_mbins, int32_t flags,
                  double *star_cells, double *row_cells)
{
    if (!ctx || !params || !mass_edges || n_rows < 1 || (!star_cells && !row_cells)) return B9_ERR_INVALID;
    if (n_mbins < 1 || n_mbins > B9_RH_MAX_MBINS) return fail(ctx, B9_ERR_INVALID, "b9_ratio_hist: n_mbins must lie in 1 .. B9_RH_MAX_MBINS");
    const int Q = marg_grid(ctx).Q;
    if (Q < 1 || Q > B9_RH_MAX_Q) return fail(ctx, B9_ERR_INVALID, "b9_ratio_hist: marg_n_q must lie in 1 .. 64");
    if ((size_t)n_mbins * (size_t)Q > B9_RH_MAX_CELLS) return fail(ctx, B9_ERR_INVALID, "b9_ratio_hist: n_mbins * marg_n_q must not exceed B9_RH_MAX_CELLS");
    for (int b = 0; b <= n_mbins; ++b)
        if (!std::isfinite(mass_edges[b]) || (b > 0 && !(mass_edges[b] > mass_edges[b - 1])))
            return fail(ctx, B9_ERR_INVALID, "b9_ratio_hist: the mass edges must be finite and strictly ascending");
    if (const int rc = chain_ready(ctx)) return rc;
    const size_t ncol = (size_t)n_mbins * Q + 1;
    const ChainCall c{"b9_ratio_hist", ncol, ncol, ncol, B9_HIST_MAX_ROWS, B9_HIST_SCRATCH_BYTES, (flags & B9_RH_CONTINUE) != 0, star_cells, row_cells, {}};
    return chain_reduce(ctx, c, params, n_rows, [&](const ChainDev &d, int m) {
        return b9k_ratio_hist(ctx->pk, ctx->st, d, m, mass_edges, n_mbins, ctx->stream);
    });
}

int b9_star_bins(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t quantity, const double *edges, int32_t n_bins, int32_t flags, double *acc)
{
    if (!ctx || !params || !edges || !acc || n_rows < 1) return B9_ERR_INVALID;
    if (quantity != B9_HQ_PRIMARY && quantity != B9_HQ_SECONDARY && quantity != B9_HQ_SYSTEM) return fail(ctx, B9_ERR_INVALID, "b9_star_bins: unknown quantity");
    if (n_bins < 1 || n_bins > B9_SBIN_MAX_BINS) return fail(ctx, B9_ERR_INVALID, "b9_star_bins: n_bins must lie in 1 .. B9_SBIN_MAX_BINS");
    if (!ctx->have_stars) return fail(ctx, B9_ERR_STATE, "load the pack and the stars first");
    const size_t n = (size_t)ctx->hs.n, ne = (size_t)n_bins + 1, ncol = (size_t)n_bins + 3;
    for (size_t i = 0; i < n; ++i)
        for (size_t b = 0; b < ne; ++b)
            if (!std::isfinite(edges[i * ne + b]) || (b > 0 && !(edges[i * ne + b] > edges[i * ne + b - 1])))
                return fail(ctx, B9_ERR_INVALID, "b9_star_bins: star " + std::to_string(i) + ": the edges must be finite and strictly ascending");
    if (const int rc = chain_ready(ctx)) return rc;
    // the call's part: every star's edges, the caller's star order (the upload's source is the caller's array: it lives until the wait)
    const ChainCall c{"b9_star_bins", ncol, ncol, 0, B9_SBIN_MAX_ROWS, B9_SBIN_SCRATCH_BYTES, (flags & B9_SBIN_CONTINUE) != 0, acc, nullptr, {8 * n * ne, 0, 0}};
    auto d_edges = [](const ChainDev &d) { return reinterpret_cast<double *>(d.extra[0]); };
    return chain_reduce(ctx, c, params, n_rows, [&](const ChainDev &d, int m) {
        return b9k_star_bins(ctx->pk, ctx->st, d, m, quantity, d_edges(d), n_bins, ctx->stream);
    }, [&](const ChainDev &d) {
        HIPCHK(ctx, hipMemcpyAsync(d_edges(d), edges, sizeof(double) * n * ne, hipMemcpyHostToDevice, ctx->stream));
        return (int)B9_OK;
    });
}

int b9_phot_resid(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t flags, double *star_resid, double *row_resid)
{
    if (!ctx || !params || n_rows < 1 || (!star_resid && !row_resid)) return B9_ERR_INVALID;
    if (const int rc = chain_ready(ctx)) return rc;
    const DevPack &pk = ctx->pk;
    const size_t n = (size_t)ctx->st.n, nf = (size_t)pk.nf, ncol = 2 + 2 * nf;
    // the call's parts: the pivots in the caller's order [n][nf] and in the mg_* copy's [mg_pad][nfp], and 1 / sigma [n][nf]
    const ChainCall c{"b9_phot_resid", ncol, ncol, 1 + 5 * nf, B9_RESID_MAX_ROWS, B9_RESID_SCRATCH_BYTES, (flags & B9_RESID_CONTINUE) != 0, star_resid, row_resid,
                      {8 * n * nf, 8 * (size_t)ctx->st.mg_pad * pk.nfp, 8 * n * nf}};
    auto piv_mg = [](const ChainDev &d) { return reinterpret_cast<double *>(d.extra[1]); };
    auto isig = [](const ChainDev &d) { return reinterpret_cast<double *>(d.extra[2]); };
    std::vector<double> piv, is;         // (the uploads' sources: they live until the driver has waited for the stream)
    return chain_reduce(ctx, c, params, n_rows, [&](const ChainDev &d, int m) {
        return b9k_phot_resid(pk, ctx->st, d, m, piv_mg(d), isig(d), ctx->stream);
    }, [&](const ChainDev &d) {
        // the pivots (the caller's obs bits where sigma > 0, else 0) and 1 / sigma (0: filter unused), the caller's star order
        const HostStars &h = ctx->hs;
        piv.resize(n * nf); is.resize(n * nf);
        for (size_t k = 0; k < piv.size(); ++k) {
            const bool used = h.sigma[k] > 0.0;
            piv[k] = used ? h.obs[k] : 0.0;
            is[k] = used ? 1.0 / h.sigma[k] : 0.0;
        }
        HIPCHK(ctx, hipMemcpyAsync(d.extra[0], piv.data(), sizeof(double) * piv.size(), hipMemcpyHostToDevice, ctx->stream));
        if (d.rows) HIPCHK(ctx, hipMemcpyAsync(isig(d), is.data(), sizeof(double) * is.size(), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, b9k_resid_stage(pk, ctx->st, reinterpret_cast<double *>(d.extra[0]), piv_mg(d), ctx->stream));
        return (int)B9_OK;
    });
}

int b9_filter_loo(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t flags, double *star_loo, double *row_loo)
{
    if (!ctx || !params || n_rows < 1 || (!star_loo && !row_loo)) return B9_ERR_INVALID;
    if (const int rc = chain_ready(ctx)) return rc;
    const DevPack &pk = ctx->pk;
    const size_t n = (size_t)ctx->st.n, nf = (size_t)pk.nf, ncol = 2 + 3 * nf, n_mg = (size_t)ctx->st.mg_pad * pk.nfp;
    // the call's parts: {the pivots, log(sigma sqrt(2 pi))} in the caller's order [2][n][nf] and in the mg_* copy's [2][mg_pad][nfp],
    // and 1 / sigma [n][nf]
    const ChainCall c{"b9_filter_loo", ncol, ncol, 1 + 6 * nf, B9_LOO_MAX_ROWS, B9_LOO_SCRATCH_BYTES, (flags & B9_LOO_CONTINUE) != 0, star_loo, row_loo,
                      {2 * 8 * n * nf, 2 * 8 * n_mg, 8 * n * nf}};
    auto in = [](const ChainDev &d) { return reinterpret_cast<double *>(d.extra[0]); };
    auto mg = [](const ChainDev &d) { return reinterpret_cast<double *>(d.extra[1]); };
    auto isig = [](const ChainDev &d) { return reinterpret_cast<double *>(d.extra[2]); };
    std::vector<double> pl, is;          // (the uploads' sources: they live until the driver has waited for the stream)
    return chain_reduce(ctx, c, params, n_rows, [&](const ChainDev &d, int m) {
        return b9k_filter_loo(pk, ctx->st, d, m, mg(d), mg(d) + n_mg, in(d) + n * nf, isig(d), ctx->stream);
    }, [&](const ChainDev &d) {
        // the pivots (the caller's obs bits where sigma > 0, else 0), log(sigma sqrt(2 pi)) (0: filter unused) and 1 / sigma (0: unused)
        const HostStars &h = ctx->hs;
        pl.resize(2 * n * nf); is.resize(n * nf);
        for (size_t k = 0; k < n * nf; ++k) {
            const bool used = h.sigma[k] > 0.0;
            pl[k] = used ? h.obs[k] : 0.0;
            pl[n * nf + k] = used ? std::log(h.sigma[k] * 2.5066282746310002) : 0.0;
            is[k] = used ? 1.0 / h.sigma[k] : 0.0;
        }
        HIPCHK(ctx, hipMemcpyAsync(in(d), pl.data(), sizeof(double) * pl.size(), hipMemcpyHostToDevice, ctx->stream));
        if (d.rows) HIPCHK(ctx, hipMemcpyAsync(isig(d), is.data(), sizeof(double) * is.size(), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, b9k_resid_stage(pk, ctx->st, in(d), mg(d), ctx->stream));
        HIPCHK(ctx, b9k_resid_stage(pk, ctx->st, in(d) + n * nf, mg(d) + n_mg, ctx->stream));
        return (int)B9_OK;
    });
}

int b9_star_offset(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t flags, int32_t n_dir, const double *k, const double *tau, double *star_off,
                   double *row_off)
{
    if (!ctx || !params || n_rows < 1 || (!star_off && !row_off) || n_dir < 1 || n_dir > B9_OFF_MAX_DIRECTIONS || !k || !tau) return B9_ERR_INVALID;
    for (int j = 0; j < n_dir; ++j)
        if (!(tau[j] > 0.0) || !std::isfinite(tau[j])) return B9_ERR_INVALID;
    if (const int rc = chain_ready(ctx)) return rc;
    const DevPack &pk = ctx->pk;
    const size_t n = (size_t)ctx->st.n, nf = (size_t)pk.nf, D = (size_t)n_dir, ncol = 2 + 3 * D, n_mg = (size_t)ctx->st.mg_pad * pk.nfp;
    for (size_t q = 0; q < D * nf; ++q)
        if (!std::isfinite(k[q])) return B9_ERR_INVALID;
    // the call's parts: the scaled directions in the caller's order [D][n][nf] and in the mg_* copy's [D][mg_pad][nfp], and the
    // stars' {C, V} and {pruning factor, Occam term} [2][n][D][2]
    const ChainCall c{"b9_star_offset", ncol, ncol, 1 + 4 * D, B9_OFF_MAX_ROWS, B9_OFF_SCRATCH_BYTES, (flags & B9_OFF_CONTINUE) != 0, star_off, row_off,
                      {8 * D * n * nf, 8 * D * n_mg, 2 * 8 * n * D * 2}};
    std::vector<double> cs;              // (the upload's source: it lives until the driver has waited for the stream)
    B9Offset o{n_dir, k, tau, nullptr, nullptr, nullptr, nullptr};
    return chain_reduce(ctx, c, params, n_rows, [&](const ChainDev &d, int m) {
        return b9k_star_offset(pk, ctx->st, d, m, o, ctx->stream);
    }, [&](const ChainDev &d) {
        // c_f = k_f / sigma_f (0: filter unused), per direction in the caller's star order
        const HostStars &h = ctx->hs;
        cs.resize(D * n * nf);
        for (size_t j = 0; j < D; ++j)
            for (size_t i = 0; i < n; ++i)
                for (size_t f = 0; f < nf; ++f) {
                    const double sg = h.sigma[i * nf + f];
                    cs[(j * n + i) * nf + f] = sg > 0.0 ? k[j * nf + f] / sg : 0.0;
                }
        double *const c_in = reinterpret_cast<double *>(d.extra[0]);
        o.c_in = c_in; o.c_mg = reinterpret_cast<double *>(d.extra[1]);
        o.cv = reinterpret_cast<double *>(d.extra[2]); o.ob = o.cv + n * D * 2;
        HIPCHK(ctx, hipMemcpyAsync(c_in, cs.data(), sizeof(double) * cs.size(), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, b9k_offset_stage(pk, ctx->st, o, ctx->stream));
        return (int)B9_OK;
    });
}

int b9_pointwise(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t flags, int32_t tail_len, double *acc, double *tail, double *row_lpd)
{
    if (!ctx || !params || n_rows < 1 || (!acc && !row_lpd)) return B9_ERR_INVALID;
    if (tail_len < 0 || tail_len > B9_PW_MAX_TAIL) return fail(ctx, B9_ERR_INVALID, "b9_pointwise: tail_len must lie in 0 .. B9_PW_MAX_TAIL");
    if (tail && !acc) return fail(ctx, B9_ERR_INVALID, "b9_pointwise: tail requires acc");
    if (const int rc = chain_ready(ctx)) return rc;
    const int n = ctx->st.n, T = (tail && tail_len > 0) ? tail_len : 0;
    const bool cont = (flags & B9_PW_CONTINUE) != 0;
    const size_t tail_bytes = sizeof(double) * (size_t)n * T;
    // the call's parts: the rows' inside-the-grid words, and the tail twice: the device's [tail_len][n] and the caller's [n][tail_len]
    const ChainCall c{"b9_pointwise", 1, B9_PW_N, 1, B9_PW_MAX_ROWS, B9_PW_SCRATCH_BYTES, cont, acc, row_lpd, {4 * (size_t)B9_PW_MAX_ROWS, tail_bytes, tail_bytes}};
    auto d_tail = [&](const ChainDev &d) { return T ? reinterpret_cast<double *>(d.extra[1]) : nullptr; };
    auto d_tail_io = [](const ChainDev &d) { return reinterpret_cast<double *>(d.extra[2]); };
    return chain_reduce(ctx, c, params, n_rows, [&](const ChainDev &d, int m) {
        return b9k_pointwise(ctx->pk, ctx->st, d, m, reinterpret_cast<int *>(d.extra[0]), d_tail(d), T, ctx->stream);
    }, [&](const ChainDev &d) {
        if (!T) return (int)B9_OK;
        if (cont) HIPCHK(ctx, hipMemcpyAsync(d_tail_io(d), tail, tail_bytes, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, b9k_pw_tail_load(cont ? d_tail_io(d) : nullptr, n, T, d_tail(d), ctx->stream));
        return (int)B9_OK;
    }, [&](const ChainDev &d) {
        if (!T) return (int)B9_OK;
        HIPCHK(ctx, b9k_pw_tail_store(d_tail(d), n, T, d_tail_io(d), ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(tail, d_tail_io(d), tail_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return (int)B9_OK;
    });
}

int b9_star_influence(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t flags, int32_t n_q, const double *q, double *acc, int32_t tail_len, double *tail,
                      int32_t n_groups, const int32_t *group, double *group_lpd)
{
    if (!ctx || !params || n_rows < 1 || (!acc && !group_lpd)) return B9_ERR_INVALID;
    if (acc && (n_q < 1 || n_q > B9_INF_MAX_Q || !q)) return fail(ctx, B9_ERR_INVALID, "b9_star_influence: acc needs q and n_q in 1 .. B9_INF_MAX_Q");
    if (tail_len < 0 || tail_len > B9_PW_MAX_TAIL) return fail(ctx, B9_ERR_INVALID, "b9_star_influence: tail_len must lie in 0 .. B9_PW_MAX_TAIL");
    if (tail && !acc) return fail(ctx, B9_ERR_INVALID, "b9_star_influence: tail requires acc");
    if (group_lpd && (n_groups < 1 || n_groups > B9_INF_MAX_GROUPS || !group))
        return fail(ctx, B9_ERR_INVALID, "b9_star_influence: group_lpd needs group and n_groups in 1 .. B9_INF_MAX_GROUPS");
    const size_t Q = acc ? (size_t)n_q : 0, G = group_lpd ? (size_t)n_groups : 0;
    for (size_t k = 0; k < (size_t)n_rows * Q; ++k)
        if (!std::isfinite(q[k])) return fail(ctx, B9_ERR_INVALID, "b9_star_influence: q must be finite");
    if (!ctx->have_stars) return fail(ctx, B9_ERR_STATE, "load the pack and the stars first");
    for (size_t i = 0; G && i < (size_t)ctx->hs.n; ++i)
        if (group[i] < -1 || group[i] >= n_groups) return fail(ctx, B9_ERR_INVALID, "b9_star_influence: star " + std::to_string(i) + ": group id outside -1 .. n_groups - 1");
    if (const int rc = chain_ready(ctx)) return rc;
    const int n = ctx->st.n, T = (tail && tail_len > 0) ? tail_len : 0;
    const bool cont = (flags & B9_INF_CONTINUE) != 0;
    const size_t tail_bytes = sizeof(double) * (size_t)n * T;
    // the call's parts: {the rows' inside-the-grid words, the chunk's rows of q, the stars' group ids}, and the tail twice as b9_pointwise's
    const size_t o_q = 256, o_group = o_q + 8 * (size_t)B9_PW_MAX_ROWS * B9_INF_MAX_Q;
    const ChainCall c{"b9_star_influence", 1, B9_INF_N(Q), G, B9_PW_MAX_ROWS, B9_PW_SCRATCH_BYTES, cont, acc, group_lpd, {o_group + 4 * (size_t)n, tail_bytes, tail_bytes}};
    auto d_tail = [&](const ChainDev &d) { return T ? reinterpret_cast<double *>(d.extra[1]) : nullptr; };
    auto d_tail_io = [](const ChainDev &d) { return reinterpret_cast<double *>(d.extra[2]); };
    int r0 = 0;                          // the chunk's first row: the driver takes the chunks in ascending order
    return chain_reduce(ctx, c, params, n_rows, [&](const ChainDev &d, int m) {
        double *const d_q = reinterpret_cast<double *>(d.extra[0] + o_q);
        if (Q) {
            const hipError_t e = hipMemcpyAsync(d_q, q + (size_t)r0 * Q, sizeof(double) * m * Q, hipMemcpyHostToDevice, ctx->stream);
            if (e != hipSuccess) return e;
        }
        r0 += m;
        const B9Influence f{(int)Q, d_q, (int)G, reinterpret_cast<const int *>(d.extra[0] + o_group)};
        return b9k_star_influence(ctx->pk, ctx->st, d, m, reinterpret_cast<int *>(d.extra[0]), d_tail(d), T, f, ctx->stream);
    }, [&](const ChainDev &d) {
        if (G) HIPCHK(ctx, hipMemcpyAsync(d.extra[0] + o_group, group, sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream));
        if (!T) return (int)B9_OK;
        if (cont) HIPCHK(ctx, hipMemcpyAsync(d_tail_io(d), tail, tail_bytes, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, b9k_pw_tail_load(cont ? d_tail_io(d) : nullptr, n, T, d_tail(d), ctx->stream));
        return (int)B9_OK;
    }, [&](const ChainDev &d) {
        if (!T) return (int)B9_OK;
        HIPCHK(ctx, b9k_pw_tail_store(d_tail(d), n, T, d_tail_io(d), ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(tail, d_tail_io(d), tail_bytes, hipMemcpyDeviceToHost, ctx->stream));
        return (int)B9_OK;
    });
}

int b9_sample_wd_mass(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t n_nodes, uint64_t seed, int64_t row0,
                      double *out_zams, double *out_wd_mass, double *out_prec_log_age, double *out_log_cool_age,
                      double *out_log_teff, double *out_logg, double *out_member, int32_t *out_pop)
{
    if (!ctx || !params || n_rows < 1 || n_nodes < 1 || !out_zams || !out_member) return B9_ERR_INVALID;
    if (const int rc = chain_ready(ctx)) return rc;
    // the seven outputs are the chunk's scratch columns [7][rows][n_wd]; nothing is accumulated
    const WdGridCall c{"b9_sample_wd_mass", false, 1, 7, 0, 0, true, 0, false, nullptr};
    double *const host[7] = {out_zams, out_member, out_wd_mass, out_prec_log_age, out_log_cool_age, out_log_teff, out_logg};
    hipStream_t s = ctx->stream;
    return wd_grid_reduce(ctx, c, params, n_rows, n_nodes, [&](const WdGridDev &d, int r0, int m) {
        hipError_t e = hipMemsetAsync(d.scratch, 0, sizeof(double) * d.per * 7, s);        // rows outside the grid write nothing
        if (e == hipSuccess) e = hipMemsetAsync(d.pop, 0, sizeof(int) * d.per, s);
        if (e != hipSuccess) return e;
        const auto col = [&](int q) { return host[q] ? d.scratch + q * d.per : nullptr; };
        B9WdSample smp{};
        smp.zams = col(0); smp.member = col(1);
        smp.wd_mass = col(2); smp.prec_log_age = col(3); smp.log_cool_age = col(4); smp.log_teff = col(5); smp.logg = col(6);
        smp.pop = d.pop;
        split_seed(seed, &smp.k0, &smp.k1); smp.row0 = (long long)(row0 + r0);
        // the kernel indexes its outputs [row][n_wd] with the launch's own rows: they are contiguous for any m
        return b9k_wd_sample(ctx->pk, ctx->st, d, m, smp, s);
    }, nullptr, [&](const WdGridDev &d, int r0, int m) {
        const size_t cnt = (size_t)m * d.n_wd, o = (size_t)r0 * d.n_wd;
        for (int q = 0; q < 7; ++q)
            if (host[q]) HIPCHK(ctx, hipMemcpyAsync(host[q] + o, d.scratch + q * d.per, sizeof(double) * cnt, hipMemcpyDeviceToHost, s));
        if (out_pop) HIPCHK(ctx, hipMemcpyAsync(out_pop + o, d.pop, sizeof(int) * cnt, hipMemcpyDeviceToHost, s));
        HIPCHK(ctx, hipStreamSynchronize(s));      // (the next chunk reuses the same device buffers)
        return (int)B9_OK;
    });
}

int b9_wd_moments(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t n_nodes, int32_t flags, double *acc)
{
    if (!ctx || !params || !acc || n_rows < 1 || n_nodes < 1) return B9_ERR_INVALID;
    if (const int rc = chain_ready(ctx)) return rc;
    const WdGridCall c{"b9_wd_moments", true, 1, B9_WDM_N, B9_WDM_N, 0, false, 0, (flags & B9_WDM_CONTINUE) != 0, acc};
    // the star kernel writes every (row, WD-stage star) of the chunk, so nothing is cleared
    return wd_grid_reduce(ctx, c, params, n_rows, n_nodes, [&](const WdGridDev &d, int, int m) {
        return b9k_wd_moments(ctx->pk, ctx->st, d, m, ctx->stream);
    });
}

int b9_wd_bins(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t n_nodes, int32_t quantity_mask, const double *edges, int32_t n_bins,
               int32_t flags, double *acc)
{
    if (!ctx || !params || !edges || !acc || n_rows < 1 || n_nodes < 1) return B9_ERR_INVALID;
    if (n_bins < 1 || n_bins > B9_WBIN_MAX_BINS) return fail(ctx, B9_ERR_INVALID, "b9_wd_bins: n_bins must lie in 1 .. B9_WBIN_MAX_BINS");
    if (quantity_mask < 1 || quantity_mask >= (1 << B9_WQ_N)) return fail(ctx, B9_ERR_INVALID, "b9_wd_bins: the quantity mask must select some of the B9_WQ_N quantities and nothing else");
    if (!ctx->have_stars) return fail(ctx, B9_ERR_STATE, "load the pack and the stars first");
    const size_t n_sel = (size_t)__builtin_popcount((unsigned)quantity_mask), ne = (size_t)n_bins + 1, ncol = (size_t)n_bins + 3;
    const size_t n_lines = (size_t)ctx->n_wd_stage * n_sel;
    for (size_t l = 0; l < n_lines; ++l)
        for (size_t b = 0; b < ne; ++b)
            if (!std::isfinite(edges[l * ne + b]) || (b > 0 && !(edges[l * ne + b] > edges[l * ne + b - 1])))
                return fail(ctx, B9_ERR_INVALID, "b9_wd_bins: WD-stage star " + std::to_string(l / n_sel) + ", selected quantity " + std::to_string(l % n_sel) +
                                                     ": the edges must be finite and strictly ascending");
    if (const int rc = chain_ready(ctx)) return rc;
    // the call's part: every line's edges, the caller's order (the upload's source is the caller's array: it lives until the wait)
    const WdGridCall c{"b9_wd_bins", true, n_sel, ncol, ncol, B9_WBIN_SCRATCH_BYTES, false, ne, (flags & B9_WBIN_CONTINUE) != 0, acc};
    // the star kernel writes every (row, line) of the chunk, so nothing is cleared
    return wd_grid_reduce(ctx, c, params, n_rows, n_nodes, [&](const WdGridDev &d, int, int m) {
        return b9k_wd_bins(ctx->pk, ctx->st, d, m, quantity_mask, n_bins, ctx->stream);
    }, [&](const WdGridDev &d) {
        HIPCHK(ctx, hipMemcpyAsync(d.edges, edges, sizeof(double) * n_lines * ne, hipMemcpyHostToDevice, ctx->stream));
        return (int)B9_OK;
    });
}

}  // extern "C"
