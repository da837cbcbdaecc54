// b9_ctx.h -- what the translation units of the C ABI share (internal; not installed): the context, and the helpers of
// one file that another one calls.  The ABI itself is include/base9_hip.h; its implementation is
//   b9_capi_ctx.cpp     context life cycle, options / tuning, work buffers, introspection, timing
//   b9_capi_stage.cpp   validation and staging of the model pack and the star catalogue into HBM (b9_load_pack, b9_load_stars)
//   b9_capi_plan.cpp    launch plans: canonical tile groups, the fused step's and the tree step's plans
//   b9_capi_margplan.cpp  the marginalised mode's catalogue plan: measured dispatch order, pieces of small catalogues
//   b9_capi_eval.cpp    b9_logpost / b9_logpost_device / b9_sample_mass / b9_derive_isochrone / b9_predict_mags / b9_sample_wd_mass / b9_star_moments / b9_mass_hist / b9_phot_resid / b9_filter_loo / b9_star_offset / b9_pointwise / b9_star_influence
//   b9_capi_blocks.cpp  the sampler's device-resident blocks (fused, tree-speculative, two-launch), b9_mcmc_run_block / b9_mcmc_wait
// and, shared by all of them,
//   b9_devbuf.h         who owns the memory: the owning buffer, the upload list, the arena carve, the sizing rules (no HIP in it;
//                       the two allocation policies below give it hipMalloc and mapped hipHostMalloc)
#pragma once
#include "../../include/base9_hip.h"
#include "b9_device.h"
#include "b9_launch.h"
#include "b9_devbuf.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

namespace b9i {

struct HostStars {
    int n = 0, nf = 0;
    std::vector<double> obs, sigma, mass1, q, prior, fmin, fmax;
    std::vector<int> stage, wd_type;
    double min_mass1 = 0.0;
};

// Which runner of b9_capi_blocks.cpp enqueued a sampler block.
enum class BlockKind { Fused, TwoLaunch, Tree };

// Where a sampler block's pieces sit in its device block and in the pinned mirror, in doubles.  One of the three layout
// functions of b9_capi_blocks.cpp fills it (there are the layouts themselves); a field another kind does not have stays 0.
struct BlockLayout {
    size_t n_samp = 0, n_lps = 0, n_rows = 0, n_int = 0;      // chain record, log-posterior record, summary rows, [free_idx, walker_ids]
    size_t o_chol = 0, o_org = 0, o_int = 0, o_rows = 0, o_lps = 0, o_samp = 0, n_total = 0;     // every kind
    size_t o_nacc = 0;                                        // fused, two-launch: the accepted count (64 bits)
    size_t o_st[2] = {0, 0};                                  // fused, tree: the two parities' state rows
    size_t o_cur0 = 0, o_lp0 = 0, o_dec = 0;                  // fused: starting state as D0 reads it, decision words
    size_t o_desc = 0;                                        // fused: the step kernel's per-block descriptor (StepBlockDev), 64-byte aligned
    size_t o_tab = 0;                                         // tree: step table
    size_t o_cur = 0, o_lp = 0;                               // two-launch: [cur] and [lp], two halves each
};

// b9_devbuf.h's allocation policies: device memory, and pinned host memory mapped into the device
struct DeviceAlloc {
    static int alloc(void **p, void **dev, size_t bytes)
    {
        const hipError_t e = hipMalloc(p, bytes);
        *dev = *p = e == hipSuccess ? *p : nullptr;
        return (int)e;
    }
    static void release(void *p) { (void)hipFree(p); }
    static int copy_in(void *dst, const void *src, size_t bytes) { return (int)hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
};
struct MappedAlloc {
    static int alloc(void **p, void **dev, size_t bytes)
    {
        hipError_t e = hipHostMalloc(p, bytes, hipHostMallocMapped);
        if (e != hipSuccess) { *p = nullptr; return (int)e; }
        if ((e = hipHostGetDevicePointer(dev, *p, 0)) != hipSuccess) { (void)hipHostFree(*p); *p = nullptr; }
        return (int)e;
    }
    static void release(void *p) { (void)hipHostFree(p); }
};
template <class T> using DeviceBuf = Buf<T, DeviceAlloc>;
template <class T> using PinnedBuf = Buf<T, MappedAlloc>;      // get(): the host's view, dev(): the device's
using Uploads = UploadList<DeviceAlloc>;

}  // namespace b9i

struct b9_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;

    bool have_pack = false;
    DevPack pk{};
    b9i::Uploads pack_allocs;

    bool have_stars = false, stars_dirty = false;
    b9i::HostStars hs;
    DevStars st{};
    b9i::Uploads star_allocs;

    DevPriors pr{};
    b9_options opt{B9_MODE_GIVEN_MASS, 1, 8, 8};

    // per-call work buffers (grown on demand, never shrunk; every buffer carries its own capacity)
    b9i::WorkBufs<IsoHdr, b9i::DeviceAlloc> work;   // isochrone headers, isochrones, parameter rows, log-posteriors: four sets, one key
    b9i::DeviceBuf<double> d_partial, d_perstar;
    b9i::DeviceBuf<double> d_marg_tab;       // marginalised mode: the companions' flux table of the current call (k_marg_table)
    b9i::DeviceBuf<double> d_marg_wd_tab;    // ... and the WD-stage stars' node table (k_marg_wd_table)
    b9i::DeviceBuf<double> d_marg_shares;    // ... and the per-star shares of a split k_star_marg launch (small catalogues)
    // the marginalised mode's catalogue plan (b9_capi_margplan.cpp): measured dispatch order and pieces; remade after the stars,
    // the pack, the priors or the options change
    bool marg_plan_ok = false;
    int marg_piece_units = 0;                 // b9_tuning.marg_piece_units: 0 = default
    b9i::Uploads marg_plan_allocs;
    const int *marg_order_spread = nullptr;   // the load-time order (photometric spread), owned by star_allocs
    std::vector<double> marg_cost;            // measured cost per star chunk (units; empty: not measured)
    std::vector<double> h_log_age, h_feh, h_y;   // host copies of the pack's grid axes (the plan's reference row is clamped into them)
    struct McmcSlot {                // one enqueued sampler block of any runner: device block, pinned mirror, events, and what
                                     // b9_mcmc_wait and a B9_BLOCK_CONTINUE successor need to find its results
        b9i::DeviceBuf<double> d;
        b9i::PinnedBuf<double> h;          // the pinned mirror (mapped: h.dev() is the device's view of it)
        hipEvent_t done = nullptr;         // recorded behind the block's last command (the download, unless the block is zero-copy)
        hipEvent_t rows_ready = nullptr;   // recorded right after the block's last kernel: the summary rows are in HBM
        bool in_flight = false;
        const void *owner = nullptr; // the b9_mcmc_block it was enqueued for
        b9i::BlockKind kind = b9i::BlockKind::Fused;   // the runner that enqueued it: it decides how the final state is read
        int W = 0;
        int final_parity = 0;        // which of lay.o_st[] (two-launch blocks: which half of [cur] / [lp]) holds the final state
        b9i::BlockLayout lay;        // where everything sits in d and h
        bool host_samples = false;   // the caller asked for the chain record (else it only exists on the device, for the rows)
    } slot[2];
    int next_slot = 0, last_slot = -1;
    const char *cont_dropped_by = nullptr;   // the configuration call that dropped last_slot (drop_continuation); open_block names it
    b9i::PinnedBuf<double> h_lp;                   // b9_logpost: 8 log-posteriors + 8 completion words in mapped pinned host memory
    unsigned long long lp_seq = 0;                 // ... and the number of the call the completion words announce

    // launch plan
    int n_cu = 256;            // compute units of the device (hipDeviceAttributeMultiprocessorCount)
    int plan_debug_key = -1;
    int logpost_plan_debug_key = -1, logpost_plan_debug_walkers = -1, logpost_plan_debug_groups = -1;      // make_plan's line: once per (configuration, walker count)
    int step_blocks_per_cu = 0, step_occ_key = -1;   // k_mcmc_step workgroups per CU for (nfp, n_pops, mass_cap), and the key it was queried for
    int heavy_parts = 4;       // workgroups per walker for the stars above the AGB tip (sized in check_ready)
    int n_wd_stage = 0;        // stars the catalogue marks as white dwarfs
    b9_tuning tuning{};        // the tuning in force (b9_get_tuning): the environment's at creation, then the last b9_set_tuning
    int tiles_per_block = 0;   // 0 = auto
    int derive_parts = 0;      // fused sampler step: workgroups per candidate isochrone (0 = one value per thread)
    int derive_order = 1;      // fused sampler step: 1 writers + derivation lead the grid and the heavy-star workgroups follow them (default),
                               // 0 heavy-star workgroups first, < 0 derivation workgroups trail the hot ones (B9_DERIVE_ORDER)
    bool two_launch_steps = false;   // b9_tuning.two_launch_steps: the derive + star launch pair per step also in given-mass mode
    int plan_debug = 0;              // b9_tuning.plan_debug: print the fused step's launch plan to stderr when it changes (2: the marginalised catalogue's pieces too)
    bool marg_prune = true;          // marginalised kernel: field floor + box pruning (b9_tuning.marg_no_pruning turns both off)
    int heavy_parts_fixed = 0;       // b9_tuning.heavy_parts: 0 = sized from the catalogue (check_ready)
    int tree_depth = 0;              // b9_tuning.tree_depth: 0 = automatic
    int tree_blocks_per_cu = 0, tree_occ_key = -1;   // k_mcmc_tree workgroups per CU, and the key it was queried for
    // candidate buffers of the tree-speculative step (grown on demand): [2 parities][W][outcomes][nodes]([pops])
    b9i::TreeBufs<IsoHdr, b9i::DeviceAlloc> tree;

    // b9_predict_mags: buffers of its own (grown on demand, never shrunk), so that a call leaves everything a sampler block
    // keeps on the device -- work buffers, candidate isochrones, final state -- untouched
    b9i::DeviceBuf<IsoHdr> d_pred_hdr;    // [2] one per population
    b9i::DeviceBuf<double> d_pred_iso;    // [2][iso_stride]
    b9i::DeviceBuf<double> d_pred_par;    // [B9_NPARAM]
    b9i::DeviceBuf<char> d_pred_io;       // one chunk of systems (pred_arena): mass1, mass ratio, magnitudes, then wd_type, pop, stage

    // b9_sample_wd_mass, b9_wd_moments, b9_wd_bins: one allocation for the three (grown on demand, never shrunk), for the same
    // reason: a chunk of rows' parameters, headers, derived isochrones and node table, the chunk's outputs or increments, the
    // accumulators, the stars' columns and the lines' edges (wd_grid_arena)
    b9i::DeviceBuf<char> d_wds;

    // b9_star_moments, b9_mass_hist, b9_phot_resid, b9_pointwise, b9_star_influence: one allocation for them all (grown on demand, never shrunk),
    // for the same reason: a chunk of rows' parameters, headers, derived isochrones and node tables, the chunk's increments,
    // the accumulators, the chunk's per-row sums and the call's own parts (chain_arena).  The calls are synchronous and keep
    // nothing on the device between them, so only one of them is using it at any time.
    b9i::DeviceBuf<char> d_chain;

    // b9_cmd_band: an allocation of its own (grown on demand, never shrunk), for the same reason: a chunk of rows' parameters,
    // headers, derived isochrones, WD node table and value table, the lines' pivots, moments, bins and edges (band_arena)
    b9i::DeviceBuf<char> d_band;

    // timing of the dominant kernel
    int timing = 0;            // 0 off, n > 0: bracket every n-th launch of the dominant kernel with events
    unsigned long long launch_no = 0;
    std::vector<hipEvent_t> ev_start, ev_stop;
    size_t ev_used = 0;
    std::vector<int> ev_count;      // launches covered by each bracket
    int timing_group = 8;            // fused step: a bracket spans this many consecutive launches (B9_TIMING_GROUP)
    double ms_accum = 0.0;
    int launches = 0;
    b9i::DeviceBuf<unsigned long long> d_clock;   // b9_clock_stamp: [2 stamps][B9_CLOCK_SLOTS]{s_memtime, s_memrealtime}
};

namespace b9i {

inline int fail(b9_ctx *ctx, int code, const std::string &msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

#define HIPCHK(ctx, call)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(ctx, B9_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));  \
    } while (0)

// an enqueued sampler block owns the context's work buffers (candidate isochrones, partial sums) until it is collected
inline bool block_outstanding(const b9_ctx *ctx)
{
    for (const auto &sl : ctx->slot) if (sl.in_flight) return true;
    return false;
}
constexpr const char *kBlockOutstanding = "a sampler block is outstanding: collect it with b9_mcmc_wait first (it owns the context's work buffers)";

// A successful b9_load_pack / b9_load_stars / b9_set_priors / b9_set_options changes the posterior: the previous block's final
// state carries a log-posterior of the old one, so no B9_BLOCK_CONTINUE block may start from it (include/base9_hip.h)
inline void drop_continuation(b9_ctx *ctx, const char *call)
{
    ctx->last_slot = -1;
    ctx->cont_dropped_by = call;
}

// a failed reservation or upload as the call's error: names the buffer and the bytes asked for
inline int alloc_failed(b9_ctx *ctx, const Reserved &r)
{
    return fail(ctx, B9_ERR_HIP, std::string(r.what) + ": allocating " + std::to_string(r.bytes) + " bytes: " + hipGetErrorString((hipError_t)r.err));
}
#define RESERVE(ctx, buf, count)                                                              \
    do {                                                                                      \
        if (const Reserved r_ = (buf).reserve(count); r_.err) return alloc_failed(ctx, named(r_, #buf)); \
    } while (0)

template <class T>
int upload(b9_ctx *ctx, Uploads &owner, const T *src, size_t count, const T **out)
{
    const Reserved r = b9i::upload<T, DeviceAlloc>(owner, src, count, out);
    return r.err ? alloc_failed(ctx, r) : B9_OK;
}

// the marginalisation grid in force: nodes per EEP interval, mass ratios (an option left at 0 counts as 1)
struct MargGrid { int K, Q; };
inline MargGrid marg_grid(const b9_ctx *ctx)
{
    return MargGrid{ctx->opt.marg_iso_increm > 0 ? ctx->opt.marg_iso_increm : 1, ctx->opt.marg_n_q > 0 ? ctx->opt.marg_n_q : 1};
}
// k_derive_iso with no previous step to finish
inline B9Prev no_prev() { return B9Prev{}; }
// a 64-bit seed as the RNG's two key words
inline void split_seed(uint64_t seed, unsigned *k0, unsigned *k1) { *k0 = (unsigned)(seed & 0xFFFFFFFFull); *k1 = (unsigned)(seed >> 32); }

// ---- b9_capi_stage.cpp
int build_stars(b9_ctx *ctx);

// ---- b9_capi_ctx.cpp
int ensure_capacity(b9_ctx *ctx, int n_walkers, int n_pops, size_t n_partial, bool want_perstar);
int ensure_marg_table(b9_ctx *ctx, int n_walkers, int n_pops, int K, int Q);
int check_ready(b9_ctx *ctx);
int timing_begin(b9_ctx *ctx, hipStream_t stream, long *slot);
int timing_end(b9_ctx *ctx, hipStream_t stream, long slot);

// Timing of the dominant kernel: every ctx->timing-th launch opens an event bracket that spans up to ctx->timing_group
// consecutive launches of that kernel (never past `last`), so the two event records cost 1/group of what a bracket around a
// single launch adds; the bracket's time / its launch count is the kernel's launch period.  bracket_before / bracket_after go
// around every launch of a loop; a lone launch passes last = true.
struct TimingBracket { long slot = -1; int covered = 0; };
inline int bracket_before(b9_ctx *ctx, hipStream_t stream, TimingBracket &b)
{
    if (b.slot >= 0) { ctx->launch_no++; return B9_OK; }      // inside an open bracket
    b.covered = 0;
    return timing_begin(ctx, stream, &b.slot);
}
inline int bracket_after(b9_ctx *ctx, hipStream_t stream, TimingBracket &b, bool last)
{
    if (b.slot < 0 || (++b.covered < ctx->timing_group && !last)) return B9_OK;
    ctx->ev_count[b.slot] = b.covered;
    const int rc = timing_end(ctx, stream, b.slot);
    b.slot = -1;
    return rc;
}

// ---- b9_capi_margplan.cpp
int ensure_marg_plan(b9_ctx *ctx);

// ---- b9_capi_plan.cpp
struct Groups { int group_tiles, n_groups; };
struct StepPlan { B9Groups plan; int derive_parts; };
struct TreePlan { int depth, group_tiles, n_groups, derive_parts; };
B9Groups make_plan(b9_ctx *ctx, int n_walkers, int n_pops);
StepPlan make_step_plan(b9_ctx *ctx, int n_walkers, int n_pops);
TreePlan make_tree_plan(b9_ctx *ctx, int n_walkers, int n_pops);
int ensure_tree_buffers(b9_ctx *ctx, int n_walkers, int n_pops, const TreePlan &tp);
void apply_tuning(b9_ctx *ctx, const b9_tuning &t);
bool tuning_from_env(b9_tuning *t);

// ---- b9_capi_eval.cpp
B9IsoSet buffer_set(const b9_ctx *ctx, int set);
B9Marg marg_tables(const b9_ctx *ctx);
int partial_count(const b9_ctx *ctx, const B9Groups &plan);
long long partial_stride(const b9_ctx *ctx);
B9Partial partials(const b9_ctx *ctx, const B9Groups &plan);
int launch_stars(b9_ctx *ctx, const B9IsoSet &bf, int32_t n_walkers, double *d_perstar, const B9Groups &plan, hipStream_t stream);

}  // namespace b9i
