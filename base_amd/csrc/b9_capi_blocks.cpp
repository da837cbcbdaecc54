// b9_capi_blocks.cpp -- the sampler's device-resident Metropolis blocks (the caller of the hot path):
// three runners -- fused one-launch steps (k_mcmc_step / k_marg_step), tree-speculative launches (k_mcmc_tree), two-launch
// steps -- around one block frame (open_block / close_block / collect_block); b9_mcmc_run_block enqueues a block,
// b9_mcmc_wait collects it.
#include "b9_ctx.h"

using namespace b9i;

namespace {

using McmcSlot = b9_ctx::McmcSlot;

// ---- the three block layouts (in doubles; BlockLayout in b9_ctx.h).  L.n_samp / n_lps / n_rows / n_int are filled in already.

// Fused block: one device allocation, laid out so that the block needs ONE upload and ONE download (each small pageable copy
// costs 10-20 us of host time, a block used to make six + four of them):
//   [step descriptor][cur0][lp0][chol][origin][decided][free, ids][n_acc][state 0] | [state 1][rows][lps][samples]
//   upload   = descriptor .. state 0  (k_mcmc_step's per-block descriptor -- whole 64-byte lines at the block's head --,
//              starting state, proposal factor, moment origin, RNG streams, cleared counters)
//   download = n_acc .. lps (.. samples when the caller wants the chain)   (acceptance count, both state parities,
//              summary rows, log-posterior record, chain record)
void layout_fused(BlockLayout &L, size_t W, size_t d, size_t)
{
    const size_t n_state = W * B9_STATE_STRIDE;
    L.o_desc = 0; L.o_cur0 = L.o_desc + B9_STEP_DESC_DOUBLES;
    L.o_lp0 = L.o_cur0 + W * B9_NPARAM; L.o_chol = L.o_lp0 + W; L.o_org = L.o_chol + d * d; L.o_dec = L.o_org + d;
    L.o_int = L.o_dec + W; L.o_nacc = L.o_int + L.n_int; L.o_st[0] = L.o_nacc + 1; L.o_st[1] = L.o_st[0] + n_state;
    L.o_rows = L.o_st[1] + n_state; L.o_lps = L.o_rows + L.n_rows; L.o_samp = L.o_lps + L.n_lps; L.n_total = L.o_samp + L.n_samp;
}

// Tree block:   [chol][origin][free, ids][state 0][state 1] | [rows][lps][samples][step table]        upload = chol .. state 1
//   download = state 0 .. lps (.. samples when the caller wants the chain)
void layout_tree(BlockLayout &L, size_t W, size_t d, size_t S)
{
    const size_t n_state = W * B9_TREE_STATE_STRIDE, n_tab = W * (S + B9_TREE_MAX_DEPTH) * B9_TREE_TAB_ROW;
    L.o_chol = 0; L.o_org = L.o_chol + d * d; L.o_int = L.o_org + d; L.o_st[0] = L.o_int + L.n_int; L.o_st[1] = L.o_st[0] + n_state;
    L.o_rows = L.o_st[1] + n_state; L.o_lps = L.o_rows + L.n_rows; L.o_samp = L.o_lps + L.n_lps; L.o_tab = L.o_samp + L.n_samp;
    L.n_total = L.o_tab + n_tab;
}

// Two-launch block:   [chol][origin][free, ids][n_acc][cur: two halves][lp: two halves][rows][lps][samples]
//   upload = chol .. first half of lp's start state;  download = n_acc .. lps (.. samples when the caller wants the chain)
void layout_two_launch(BlockLayout &L, size_t W, size_t d, size_t)
{
    L.o_chol = 0; L.o_org = L.o_chol + d * d; L.o_int = L.o_org + d; L.o_nacc = L.o_int + L.n_int; L.o_cur = L.o_nacc + 1;
    L.o_lp = L.o_cur + 2 * W * B9_NPARAM; L.o_rows = L.o_lp + 2 * W; L.o_lps = L.o_rows + L.n_rows; L.o_samp = L.o_lps + L.n_lps;
    L.n_total = L.o_samp + L.n_samp;
}

// where a block's final state sits in its device block and mirror: the final parity's state rows, or -- two-launch -- the
// final half of [cur] (and of [lp])
size_t final_off(const McmcSlot &sl)
{
    return sl.kind == BlockKind::TwoLaunch ? sl.lay.o_cur + (size_t)sl.final_parity * sl.W * B9_NPARAM : sl.lay.o_st[sl.final_parity];
}
size_t final_lp_off(const McmcSlot &sl) { return sl.lay.o_lp + (size_t)sl.final_parity * sl.W; }

// ---- the block contract every runner shares: open_block ... the runner's launch sequence ... close_block; collect_block

// Collect an enqueued block: wait for its download, unpack the pinned mirror into the caller's arrays.
int collect_block(b9_ctx *ctx, McmcSlot &sl, b9_mcmc_block *blk)
{
    HIPCHK(ctx, hipEventSynchronize(sl.done));
    sl.in_flight = false;
    const BlockLayout &L = sl.lay;
    const double *stage = sl.h.get(), *fin = stage + final_off(sl);
    if (sl.kind == BlockKind::TwoLaunch) {       // [cur][lp] of the final half, n_acc as a 64-bit count
        std::memcpy(blk->params, fin, sizeof(double) * (size_t)sl.W * B9_NPARAM);
        std::memcpy(blk->logpost, stage + final_lp_off(sl), sizeof(double) * (size_t)sl.W);
        unsigned long long n_acc = 0;
        std::memcpy(&n_acc, stage + L.o_nacc, sizeof n_acc);
        blk->n_accept = (int64_t)n_acc;
    } else {                                     // state rows, the per-walker accepted counts carried in them
        const bool tree = sl.kind == BlockKind::Tree;
        const size_t stride = tree ? B9_TREE_STATE_STRIDE : B9_STATE_STRIDE;
        const int o_cur = tree ? B9_TS_CUR : B9_ST_CUR, o_lp = tree ? B9_TS_LP : B9_ST_LP, o_nacc = tree ? B9_TS_NACC : B9_ST_NACC;
        double n_acc = 0.0;
        for (int w = 0; w < sl.W; ++w) {
            const double *row = fin + (size_t)w * stride;
            std::memcpy(blk->params + (size_t)w * B9_NPARAM, row + o_cur, sizeof(double) * B9_NPARAM);
            blk->logpost[w] = row[o_lp];
            n_acc += row[o_nacc];
        }
        blk->n_accept = (int64_t)n_acc;
    }
    if (L.n_samp && sl.host_samples && blk->samples) std::memcpy(blk->samples, stage + L.o_samp, L.n_samp * 8);
    if (L.n_rows && blk->rows) std::memcpy(blk->rows, stage + L.o_rows, L.n_rows * 8);
    if (L.n_lps && blk->lps) std::memcpy(blk->lps, stage + L.o_lps, L.n_lps * 8);
    return B9_OK;
}

struct BlockFrame {             // an opened block: what a runner's launch sequence works with
    McmcSlot *sl;
    const BlockLayout *L;       // &sl->lay
    double *dev, *stage, *mirror;      // the device block; the pinned mirror as the host and as the device see it
    bool cont, want_rows;
    const double *prev_final, *prev_final_lp;   // continuing: the previous block's final state on the device (final_off / final_lp_off)
};

// Opening: two slots (device block + pinned mirror + events) alternate, so that a block can be enqueued while its predecessor
// is still running or waiting to be collected.  Takes the next slot, lays the block out, grows the slot's memory, stages the
// upload words every kind has (proposal factor, moment origin, RNG streams) in the mirror.
int open_block(b9_ctx *ctx, const b9_mcmc_block *blk, BlockKind kind, void (*layout)(BlockLayout &, size_t, size_t, size_t), BlockFrame *f)
{
    const size_t W = blk->n_walkers, d = blk->n_free, S = blk->n_steps;
    McmcSlot &sl = ctx->slot[ctx->next_slot];
    f->cont = (blk->flags & B9_BLOCK_CONTINUE) != 0;
    f->want_rows = blk->row_origin != nullptr;
    if (sl.in_flight) return fail(ctx, B9_ERR_STATE, "two blocks are already outstanding: collect one with b9_mcmc_wait first");
    const McmcSlot *pv = ctx->last_slot >= 0 ? &ctx->slot[ctx->last_slot] : nullptr;
    if (f->cont && !pv && ctx->cont_dropped_by)
        return fail(ctx, B9_ERR_STATE, std::string("B9_BLOCK_CONTINUE after ") + ctx->cont_dropped_by +
                    ": the previous block's state belongs to another posterior; start the block from host state");
    if (f->cont && (!pv || pv->W != (int)W || pv->kind != kind))
        return fail(ctx, B9_ERR_STATE, "B9_BLOCK_CONTINUE needs a previous block of this context with the same n_walkers and mode");
    BlockLayout &L = sl.lay;
    L = BlockLayout{};
    L.n_samp = (blk->samples || f->want_rows) ? S * W * d : 0;
    L.n_lps = blk->lps ? S * W : 0;
    L.n_rows = f->want_rows ? W * B9_ROW_LEN(d) : 0;
    L.n_int = (d + W + 1) / 2;                                            // ints, in units of 8 bytes
    layout(L, W, d, S);
    RESERVE(ctx, sl.d, L.n_total);        // (a CONTINUE block reads the OTHER slot's final state, never this slot's old contents)
    RESERVE(ctx, sl.h, L.n_total);        // pinned staging mirror, mapped into the device
    if (!sl.done) HIPCHK(ctx, hipEventCreateWithFlags(&sl.done, hipEventDisableTiming));
    if (!sl.rows_ready) HIPCHK(ctx, hipEventCreateWithFlags(&sl.rows_ready, hipEventDisableTiming));
    f->sl = &sl; f->L = &L;
    f->dev = sl.d.get(); f->stage = sl.h.get(); f->mirror = sl.h.dev();
    std::memcpy(f->stage + L.o_chol, blk->chol, d * d * 8);
    if (f->want_rows) std::memcpy(f->stage + L.o_org, blk->row_origin, d * 8); else std::memset(f->stage + L.o_org, 0, d * 8);
    int *hi = reinterpret_cast<int *>(f->stage + L.o_int);
    std::memcpy(hi, blk->free_idx, d * sizeof(int));
    std::memcpy(hi + d, blk->walker_ids, W * sizeof(int));
    // continuing: the previous block's final state, stream-ordered behind its last launch
    f->prev_final = f->cont ? pv->d.get() + final_off(*pv) : nullptr;
    f->prev_final_lp = (f->cont && kind == BlockKind::TwoLaunch) ? pv->d.get() + final_lp_off(*pv) : nullptr;
    sl.kind = kind; sl.W = (int)W;           // (this slot is never last_slot: nothing reads it before close_block puts it in flight)
    return B9_OK;
}

// Closing, behind the block's last kernel: rows_ready when the caller asked for it, the download of [down_from, lps or samples]
// unless the last kernel wrote the mirror itself (zero_copy), done; then the slot is in flight and the next block gets the other one.
int close_block(b9_ctx *ctx, b9_mcmc_block *blk, const BlockFrame &f, int final_parity, size_t down_from, bool zero_copy)
{
    McmcSlot &sl = *f.sl;
    const BlockLayout &L = *f.L;
    hipStream_t s = ctx->stream;
    const bool rows_event = f.want_rows && (blk->flags & B9_BLOCK_ROWS_EVENT) != 0;
    if (rows_event) HIPCHK(ctx, hipEventRecord(sl.rows_ready, s));
    blk->d_rows = f.want_rows ? (void *)(f.dev + L.o_rows) : nullptr;
    blk->rows_ready = rows_event ? (void *)sl.rows_ready : nullptr;
    const size_t down_end = L.o_samp + (blk->samples ? L.n_samp : 0);
    if (!zero_copy) HIPCHK(ctx, hipMemcpyAsync(f.stage + down_from, f.dev + down_from, (down_end - down_from) * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(ctx, hipEventRecord(sl.done, s));
    sl.final_parity = final_parity;
    sl.host_samples = blk->samples != nullptr;
    sl.in_flight = true; sl.owner = blk;
    ctx->last_slot = ctx->next_slot;
    ctx->cont_dropped_by = nullptr;
    ctx->next_slot ^= 1;
    return (blk->flags & B9_BLOCK_ASYNC) ? B9_OK : collect_block(ctx, sl, blk);
}

/* Device-resident Metropolis block, given-mass mode: ONE launch per step (StepDev in b9_device.h).
 * Launch sequence for S steps:  D0  K(0) K(1) ... K(S-1)  F
 *   D0   = k_mcmc_begin (the upload from the mapped mirror) + k_derive_iso: draws step 0's proposal from the starting state
 *          and derives its isochrones
 *   K(t) = k_mcmc_step: decision of step t-1, star likelihood of step t's proposal, and -- on a few
 *          extra workgroups -- both candidate isochrone sets of step t+1
 *   F    = k_mcmc_finish: decision of step S-1.
 * The marginalised mode runs the same block with k_marg_step in K(t)'s place (b9_marg_step.hip.h: the candidates are node
 * tables, built inside the launch; no isochrone is materialised) and, for the block's first proposal, k_marg_table behind D0. */
struct MargBlock {             // what the marginalised flavour adds to a fused block
    B9Marg mg{};                               // the grid; four candidate sets (two parities x two candidates) of node tables, WD tables and split shares
    double *partial = nullptr;                 // [W][stride]: two parities of (star chunks + WD-stage stars) partials
    long long stride = 0, tab_doubles = 0, wd_doubles = 0;       // (the two tables' doubles per (walker, population))
    int n_partial = 0;
};

// can the marginalised mode run fused steps on this context?  (the table builders' mass column must fit beside the star role's
// workgroups in LDS: isochrones of more than ~600 points at 8 filters keep the two-launch step)
bool marg_fused_ok(const b9_ctx *ctx) { return b9k_marg_step_lds(ctx->pk.nfp, ctx->work.mass_cap) <= B9_MSTEP_LDS_MAX(ctx->pk.nfp); }

int run_block_fused(b9_ctx *ctx, b9_mcmc_block *blk, bool marg)
{
    const int W = blk->n_walkers, d = blk->n_free, S = blk->n_steps, n_pops = ctx->opt.n_pops;
    StepPlan sp{};
    MargBlock mb;
    if (marg) {
        int rc = ensure_marg_table(ctx, 4 * W, n_pops, marg_grid(ctx).K, marg_grid(ctx).Q);
        if (rc) return rc;
        mb.mg = marg_tables(ctx);
        mb.n_partial = ctx->st.mg_pad / 64 + (ctx->st.n_wd + 3) / 4;
        mb.stride = 2 * (((long long)mb.n_partial + 7) & ~7ll);
        rc = ensure_capacity(ctx, W, n_pops, (size_t)std::max<long long>(mb.stride, partial_stride(ctx)) * W, false);
        if (rc) return rc;
        mb.partial = ctx->d_partial.get();
        mb.tab_doubles = b9k_marg_table_doubles(ctx->pk.nfp, ctx->work.mass_cap, mb.mg.K, mb.mg.Q);
        mb.wd_doubles = b9k_marg_wd_table_doubles(ctx->pk.nfp, mb.mg.K);
    } else {
        sp = make_step_plan(ctx, W, n_pops);
    }
    const B9Groups &plan = sp.plan;
    const int derive_parts = sp.derive_parts;
    BlockFrame f;
    int rc = open_block(ctx, blk, BlockKind::Fused, layout_fused, &f);
    if (rc) return rc;
    const BlockLayout &L = *f.L;
    double *const dev = f.dev, *const stage = f.stage;
    const size_t n_state = (size_t)W * B9_STATE_STRIDE, n_cur = (size_t)W * B9_NPARAM;
    double *d_state = dev + L.o_st[0];               // [2][W][stride]; the block's first launch has parity 1 and reads parity 0
    double *d_cur0 = dev + L.o_cur0, *d_lp0 = dev + L.o_lp0, *d_chol = dev + L.o_chol;
    unsigned long long *d_decided = reinterpret_cast<unsigned long long *>(dev + L.o_dec);
    int *d_free = reinterpret_cast<int *>(dev + L.o_int), *d_ids = d_free + d;
    unsigned long long *d_nacc = reinterpret_cast<unsigned long long *>(dev + L.o_nacc);
    hipStream_t s = ctx->stream;
    const B9IsoSet cand = buffer_set(ctx, 0);      // the work buffers from their start: the block's four candidate sets, W walkers each (cand_at)
    StepDev sd{};
    sd.d = d; sd.n_walkers = W; sd.n_pops = n_pops;
    sd.n_partial = marg ? mb.n_partial : partial_count(ctx, plan); sd.mass_cap = cand.mass_cap; sd.heavy_parts = marg ? 0 : ctx->heavy_parts;
    split_seed(blk->seed, &sd.k0, &sd.k1);
    sd.partial_stride = marg ? mb.stride : partial_stride(ctx); sd.iso_stride = cand.iso_stride;
    sd.state = d_state; sd.partial = marg ? mb.partial : ctx->d_partial.get();
    sd.cand_par = cand.params; sd.cand_hdr = cand.hdr; sd.cand_iso = cand.iso;
    sd.chol = d_chol; sd.free_idx = d_free; sd.walker_ids = d_ids;
    sd.samples = L.n_samp ? dev + L.o_samp : nullptr; sd.lps = L.n_lps ? dev + L.o_lps : nullptr; sd.n_acc = d_nacc; sd.decided = d_decided;
    sd.rows = nullptr; sd.row_origin = dev + L.o_org; sd.n_steps = S;
    // (a parity's row: the hot waves' partials + one set of heavy-star partials per candidate)
    if (2 * ((long long)sd.n_partial + sd.heavy_parts) > sd.partial_stride) return fail(ctx, B9_ERR_CAPACITY, "partial buffer too small for two parities");
    // k_mcmc_step's descriptor of THIS block (views, block-constant step fields, the grid's cut), rebuilt for every block --
    // priors, tuning or the catalogue may have changed since the slot's last one -- at the head of the upload: it reaches the
    // device with the starting state, in k_mcmc_begin.  `desc` stays with the host to size the launches.
    StepBlockDev desc{};                  // (k_marg_step keeps its by-value arguments: its block uploads zeros here)
    const StepBlockDev *const d_desc = reinterpret_cast<const StepBlockDev *>(dev + L.o_desc);
    if (!marg) b9k_mcmc_step_desc(&desc, ctx->pk, ctx->st, sd, ctx->pr, plan, ctx->heavy_parts, derive_parts, ctx->derive_order);
    std::memcpy(stage + L.o_desc, &desc, sizeof desc);
    {
        std::memset(stage + L.o_cur0, 0, (n_cur + W) * 8);
        if (!f.cont) {
            std::memcpy(stage + L.o_cur0, blk->params, n_cur * 8);
            std::memcpy(stage + L.o_lp0, blk->logpost, (size_t)W * 8);
        }
        std::memset(stage + L.o_dec, 0xFF, (size_t)W * 8);               // no step published yet
        std::memset(stage + L.o_nacc, 0, 8);
        double *st0 = stage + L.o_st[0];                                  // starting state -> parity 0, which K(0) (parity 1) reads
        std::memset(st0, 0, n_state * 8);
        if (!f.cont)
            for (int w = 0; w < W; ++w) {
                std::memcpy(st0 + (size_t)w * B9_STATE_STRIDE + B9_ST_CUR, blk->params + (size_t)w * B9_NPARAM, sizeof(double) * B9_NPARAM);
                st0[(size_t)w * B9_STATE_STRIDE + B9_ST_LP] = blk->logpost[w];
                st0[(size_t)w * B9_STATE_STRIDE + B9_ST_LPRIOR] = -INFINITY;
            }
        // one launch: the upload (cur0 .. state 0), read by the device from the mapped mirror, and -- continuing -- the previous
        // block's final state in place of the starting state
        HIPCHK(ctx, b9k_mcmc_begin(f.mirror, dev, (int)L.o_st[1], f.prev_final, d_cur0, d_lp0, d_state, W, s));
    }
    {   // D0: proposal of step 0 and its isochrones -> candidate 0 of parity 1 (K(t) has parity (t + 1) & 1)
        McmcDev mc{};
        mc.enabled = 1; mc.d = d; mc.n_walkers = W; mc.has_prev = 0; mc.pin = 0; mc.row = 0;
        mc.cur = d_cur0; mc.lp_cur = d_lp0; mc.chol = d_chol; mc.free_idx = d_free; mc.walker_ids = d_ids;
        mc.k0 = sd.k0; mc.k1 = sd.k1; mc.step = (unsigned long long)blk->step0; mc.n_acc = d_nacc;
        const CandAt c10 = cand_at(1, 0, W, n_pops);
        const B9IsoSet first = cand.at(c10.row);
        HIPCHK(ctx, b9k_derive_iso(ctx->pk, first, W, mc, ctx->pr, no_prev(), s));
        if (marg) {     // ... and its node tables (every later candidate's are built inside k_marg_step)
            B9Marg mg = mb.mg;
            mg.tab += c10.wp * mb.tab_doubles;
            mg.wd_tab = ctx->st.n_wd > 0 ? mg.wd_tab + c10.wp * mb.wd_doubles : nullptr;
            HIPCHK(ctx, b9k_marg_tables(ctx->pk, first, W, mg, s));
        }
    }
    TimingBracket tb;
    for (int t = 0; t < S; ++t) {
        sd.set = (t + 1) & 1; sd.has_prev = t > 0; sd.derive_next = t + 1 < S; sd.row = t - 1;
        sd.step = (unsigned long long)(blk->step0 + t);
        rc = bracket_before(ctx, s, tb);
        if (rc) return rc;
        if (marg)
            HIPCHK(ctx, b9k_marg_step(ctx->pk, ctx->st, sd, ctx->pr, mb.mg, ctx->n_cu, s));
        else
            HIPCHK(ctx, b9k_mcmc_step(desc, d_desc, sd, s));
        rc = bracket_after(ctx, s, tb, t == S - 1);
        if (rc) return rc;
    }
    const int fin = (S + 1) & 1;
    sd.set = fin; sd.has_prev = 1; sd.derive_next = 0; sd.row = S - 1;
    sd.step = (unsigned long long)(blk->step0 + S);
    sd.rows = f.want_rows ? dev + L.o_rows : nullptr;
    // a block whose chain record stays on the device needs no download: its last launch writes what the host reads (final
    // state, accepted counts, summary rows) into the mapped mirror as well
    const bool zero_copy = !blk->samples && !blk->lps;
    sd.host_state = zero_copy ? f.mirror + L.o_st[fin] : nullptr;
    sd.host_rows = (zero_copy && f.want_rows) ? f.mirror + L.o_rows : nullptr;
    HIPCHK(ctx, b9k_mcmc_finish(ctx->pk, sd, ctx->pr, s));
    return close_block(ctx, blk, f, fin, L.o_nacc, zero_copy);
}

/* Device-resident Metropolis block, given-mass mode, tree-speculative launches (TreeDev in b9_device.h): `depth` steps per launch.
 * Launch sequence for S steps, M = ceil(S / depth):   B  P  K(0) K(1) ... K(M-1)  F
 *   B    = k_tree_begin: the upload from the mapped mirror; the starting state into both parities' state rows
 *   P    = k_mcmc_tree, prologue: derives the first tree (2^depth - 1 candidates) from the starting state
 *   K(m) = k_mcmc_tree: walks the tree K(m-1) evaluated (the sequential accept tests of its `depth` steps), evaluates the tree
 *          rooted at the resulting state, derives K(m+1)'s tree for every possible outcome of its own
 *   F    = k_tree_finish: the last walk, final state, summary rows.
 * Same block contract as run_block_fused (slots, mapped mirror, B9_BLOCK_ASYNC / CONTINUE, rows in HBM behind rows_ready). */
int run_block_tree(b9_ctx *ctx, b9_mcmc_block *blk, const TreePlan &tp)
{
    const int W = blk->n_walkers, d = blk->n_free, S = blk->n_steps, n_pops = ctx->opt.n_pops, depth = tp.depth;
    int rc = ensure_tree_buffers(ctx, W, n_pops, tp);
    if (rc) return rc;
    BlockFrame f;
    rc = open_block(ctx, blk, BlockKind::Tree, layout_tree, &f);
    if (rc) return rc;
    const BlockLayout &L = *f.L;
    double *const dev = f.dev, *const stage = f.stage;
    hipStream_t s = ctx->stream;
    {   // B
        std::memset(stage + L.o_st[0], 0, (L.o_rows - L.o_st[0]) * 8);
        if (!f.cont)
            for (int p = 0; p < 2; ++p)
                for (int w = 0; w < W; ++w) {
                    double *row = stage + L.o_st[p] + (size_t)w * B9_TREE_STATE_STRIDE;
                    std::memcpy(row + B9_TS_CUR, blk->params + (size_t)w * B9_NPARAM, sizeof(double) * B9_NPARAM);
                    row[B9_TS_LP] = blk->logpost[w];
                }
        HIPCHK(ctx, b9k_tree_begin(f.mirror, dev, (int)L.o_rows, f.prev_final, dev + L.o_st[0], W, s));
    }
    const B9IsoSet cand{ctx->tree.par.get(), ctx->tree.hdr.get(), ctx->tree.iso.get(), ctx->work.iso_stride, ctx->work.mass_cap, n_pops};     // every candidate of the tree
    TreeDev td{};
    td.d = d; td.n_walkers = W; td.n_pops = cand.n_pops; td.depth = depth;
    td.n_groups = tp.n_groups; td.heavy_parts = ctx->heavy_parts; td.mass_cap = cand.mass_cap;
    td.part_stride = (int)tree_part_stride(tp.n_groups, ctx->heavy_parts);
    split_seed(blk->seed, &td.k0, &td.k1);
    td.iso_stride = cand.iso_stride;
    td.state = dev + L.o_st[0]; td.partial = ctx->tree.partial.get();
    td.cand_par = cand.params; td.cand_hdr = cand.hdr; td.cand_iso = cand.iso;
    td.chol = dev + L.o_chol; td.free_idx = reinterpret_cast<int *>(dev + L.o_int); td.walker_ids = td.free_idx + d;
    td.samples = L.n_samp ? dev + L.o_samp : nullptr; td.lps = L.n_lps ? dev + L.o_lps : nullptr;
    td.row_origin = dev + L.o_org; td.n_steps = S;
    td.step_tab = dev + L.o_tab; td.tab_steps = S + B9_TREE_MAX_DEPTH; td.block_step0 = (unsigned long long)blk->step0;
    const int M = (S + depth - 1) / depth;
    {   // P: the block's first tree from the starting state -> candidates of parity 0, outcome slot 0
        td.set = 1; td.levels_prev = 0; td.levels = 0; td.derive_mode = 2; td.row = 0;
        td.step = (unsigned long long)blk->step0; td.next_step = (unsigned long long)blk->step0;
        HIPCHK(ctx, b9k_mcmc_tree(ctx->pk, ctx->st, td, ctx->pr, tp.group_tiles, tp.derive_parts, s));
    }
    TimingBracket tb;
    for (int m = 0; m < M; ++m) {
        td.set = m & 1;
        td.levels_prev = m > 0 ? depth : 0;
        td.levels = std::min(depth, S - m * depth);
        td.derive_mode = (m + 1 < M) ? 1 : 0;
        td.row = (m - 1) * depth;
        td.step = (unsigned long long)(blk->step0 + (long long)m * depth);
        td.next_step = td.step + (unsigned)depth;
        rc = bracket_before(ctx, s, tb);
        if (rc) return rc;
        HIPCHK(ctx, b9k_mcmc_tree(ctx->pk, ctx->st, td, ctx->pr, tp.group_tiles, tp.derive_parts, s));
        rc = bracket_after(ctx, s, tb, m == M - 1);
        if (rc) return rc;
    }
    // F
    const int fin = M & 1;
    td.set = fin;
    td.levels_prev = std::min(depth, S - (M - 1) * depth);
    td.levels = 0; td.derive_mode = 0;
    td.row = (M - 1) * depth;
    td.step = (unsigned long long)(blk->step0 + S); td.next_step = td.step;
    td.rows = f.want_rows ? dev + L.o_rows : nullptr;
    const bool zero_copy = !blk->samples && !blk->lps;      // (as in run_block_fused: the finish writes the mirror itself)
    td.host_state = zero_copy ? f.mirror + L.o_st[fin] : nullptr;
    td.host_rows = (zero_copy && f.want_rows) ? f.mirror + L.o_rows : nullptr;
    HIPCHK(ctx, b9k_tree_finish(td, ctx->pr, s));
    return close_block(ctx, blk, f, fin, L.o_st[0], zero_copy);
}

/* Device-resident Metropolis block with TWO launches per step (marginalised mode; b9_tuning.two_launch_steps):
 *   D(0) L(0)  D(1) L(1)  ...  D(S-1) L(S-1)  F  [R]
 *   D(t) = k_derive_iso: finishes step t-1 (sum + prior + accept; t > 0), proposes step t, derives its isochrones
 *   L(t) = the star likelihood of step t's proposals;   F = k_finalize: finishes the last step;
 *   R    = k_chain_rows: the block's per-walker summary rows, condensed from the chain record on the device.
 * Same contract as the fused path: one pinned mirror per slot for the upload and the download, B9_BLOCK_ASYNC /
 * B9_BLOCK_CONTINUE / summary rows in HBM behind rows_ready -- a star launch here takes milliseconds, so none of this is for
 * speed; it gives a multi-GPU driver ONE way to run blocks and to read rows, whatever the evaluation mode. */
int run_block_two_launch(b9_ctx *ctx, b9_mcmc_block *blk, const B9Groups &plan)
{
    const int W = blk->n_walkers, d = blk->n_free, S = blk->n_steps;
    BlockFrame f;
    int rc = open_block(ctx, blk, BlockKind::TwoLaunch, layout_two_launch, &f);
    if (rc) return rc;
    const BlockLayout &L = *f.L;
    double *const dev = f.dev, *const stage = f.stage;
    const size_t n_cur = (size_t)W * B9_NPARAM;
    hipStream_t s = ctx->stream;
    // upload: proposal factor, moment origin, RNG streams, cleared counter and (unless continuing) the starting state
    std::memset(stage + L.o_nacc, 0, 8);
    HIPCHK(ctx, hipMemcpyAsync(dev + L.o_chol, stage + L.o_chol, (L.o_cur - L.o_chol) * 8, hipMemcpyHostToDevice, s));
    if (!f.cont) {
        std::memcpy(stage + L.o_cur, blk->params, n_cur * 8);
        std::memcpy(stage + L.o_lp, blk->logpost, (size_t)W * 8);
        HIPCHK(ctx, hipMemcpyAsync(dev + L.o_cur, stage + L.o_cur, n_cur * 8, hipMemcpyHostToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(dev + L.o_lp, stage + L.o_lp, (size_t)W * 8, hipMemcpyHostToDevice, s));
    } else {      // the previous block's final half -> this block's half 0
        HIPCHK(ctx, hipMemcpyAsync(dev + L.o_cur, f.prev_final, n_cur * 8, hipMemcpyDeviceToDevice, s));
        HIPCHK(ctx, hipMemcpyAsync(dev + L.o_lp, f.prev_final_lp, (size_t)W * 8, hipMemcpyDeviceToDevice, s));
    }
    McmcDev mc{};
    mc.enabled = 1; mc.d = d; mc.n_walkers = W;
    mc.cur = dev + L.o_cur; mc.lp_cur = dev + L.o_lp;
    mc.chol = dev + L.o_chol;
    mc.free_idx = reinterpret_cast<int *>(dev + L.o_int); mc.walker_ids = mc.free_idx + d;
    mc.samples = L.n_samp ? dev + L.o_samp : nullptr; mc.lps = L.n_lps ? dev + L.o_lps : nullptr;
    mc.n_acc = reinterpret_cast<unsigned long long *>(dev + L.o_nacc);
    split_seed(blk->seed, &mc.k0, &mc.k1);
    const B9Partial part = partials(ctx, plan);
    for (int t = 0; t < S; ++t) {
        const B9IsoSet bf = buffer_set(ctx, t & 1);
        mc.step = (unsigned long long)(blk->step0 + t);     // the step being proposed
        mc.has_prev = t > 0;
        mc.pin = t > 0 ? (t - 1) & 1 : 0;                   // state half on entry
        mc.row = t - 1;                                     // chain row of the step being finished
        HIPCHK(ctx, b9k_derive_iso(ctx->pk, bf, W, mc, ctx->pr, B9Prev{part, buffer_set(ctx, (t & 1) ^ 1)}, s));
        rc = launch_stars(ctx, bf, W, nullptr, plan, s);
        if (rc) return rc;
    }
    {   // finish the last step
        const B9IsoSet bf = buffer_set(ctx, (S - 1) & 1);
        mc.step = (unsigned long long)(blk->step0 + S - 1);
        mc.has_prev = 0;
        mc.pin = S > 1 ? (S - 2) & 1 : 0;                   // the half D(S-1) wrote (or the initial half)
        if (S > 1) mc.pin ^= 1;
        mc.row = S - 1;
        HIPCHK(ctx, b9k_finalize(bf, part, ctx->pr, W, ctx->work.logpost.get(), nullptr, ctx->st.n, mc, s));
    }
    const int fin = mc.pin ^ 1;                             // half that holds the final state
    if (f.want_rows) {
        StepDev sd{};
        sd.d = d; sd.n_walkers = W; sd.n_steps = S; sd.samples = mc.samples; sd.free_idx = mc.free_idx;
        sd.row_origin = dev + L.o_org; sd.rows = dev + L.o_rows; sd.host_rows = nullptr;
        HIPCHK(ctx, b9k_chain_rows(sd, dev + L.o_cur + (size_t)fin * n_cur, dev + L.o_lp + (size_t)fin * W, s));
    }
    return close_block(ctx, blk, f, fin, L.o_nacc, false);
}

/* The heavy role of a given-mass block keeps the pack's axes, its AGB tips and the candidates' mass columns in LDS
 * (heavy_lds_doubles): a block whose pack asks for more than a CU has is refused here, on the host, before it uploads or launches
 * anything.  With the tips staged as corner columns (n_age doubles each) it is the age axis that decides, and the message says so. */
int check_step_lds(b9_ctx *ctx, int n_pops, B9StepKind kind, int n_groups)
{
    size_t dyn = 0, stat = 0;
    HIPCHK(ctx, b9k_step_lds(ctx->pk, n_pops, ctx->work.mass_cap, kind, n_groups, &dyn, &stat));
    if (dyn + stat <= B9_LDS_PER_CU) return B9_OK;
    const bool corner_columns = (size_t)ctx->pk.n_feh * ctx->pk.n_y * ctx->pk.n_age > B9_TIPS_LDS_MAX;
    const std::string what = corner_columns
        ? "the age axis of " + std::to_string(ctx->pk.n_age) + " entries is too long for the sampler step"
        : "the pack's tables (axes of " + std::to_string(ctx->pk.hc_len) + " entries, isochrones of up to " +
          std::to_string(ctx->work.mass_cap) + " points) are too large for the sampler step";
    return fail(ctx, B9_ERR_CAPACITY, "b9_mcmc_run_block: " + what + ": its heavy role needs " + std::to_string(dyn) + " dynamic + " +
                std::to_string(stat) + " static bytes of LDS, a compute unit has " + std::to_string(B9_LDS_PER_CU));
}

}  // namespace

extern "C" {

/* Device-resident Metropolis block (the caller of the hot path): validates the block, sizes the work buffers
 * for its walkers and hands it to one of the three runners above --
 *   given-mass mode:     run_block_tree when the tree plan's depth is >= 2 (b9_tuning.tree_depth, or automatic: few walkers),
 *                        else run_block_fused (k_mcmc_step, one launch per step);
 *   marginalised mode:   run_block_fused with k_marg_step while the table builders' LDS fits beside the star role (marg_fused_ok);
 *   either mode:         run_block_two_launch when b9_tuning.two_launch_steps is set, and for the marginalised isochrones too
 *                        long for the fused step.
 * All three keep the same block contract (open_block / close_block / collect_block). */
int b9_mcmc_run_block(b9_ctx *ctx, b9_mcmc_block *blk)
{
    if (!ctx || !blk || blk->n_walkers < 1 || blk->n_steps < 0 || blk->n_free < 1 || blk->n_free > 11 ||
        !blk->free_idx || !blk->chol || !blk->walker_ids || !blk->params || !blk->logpost)
        return B9_ERR_INVALID;
    int rc = check_ready(ctx);
    if (rc) return rc;
    const int W = blk->n_walkers, d = blk->n_free, S = blk->n_steps, n_pops = ctx->opt.n_pops;
    for (int i = 0; i < d; ++i)
        if (blk->free_idx[i] < 0 || blk->free_idx[i] >= B9_NPARAM) return fail(ctx, B9_ERR_INVALID, "free_idx out of range");
    if (S == 0) { blk->n_accept = 0; return B9_OK; }
    // (the work buffers are sized for the walker count: they must not be re-allocated under an enqueued block)
    for (const auto &sl : ctx->slot)
        if (sl.in_flight && sl.W != W) return fail(ctx, B9_ERR_STATE, "collect the outstanding block(s) before running a block with another number of walkers");
    rc = ensure_capacity(ctx, W, n_pops, (size_t)partial_stride(ctx) * W, false);      // (before any plan: the plans key on mass_cap)
    if (rc) return rc;
    const B9Groups plan = make_plan(ctx, W, n_pops);
    if (ctx->opt.mode == B9_MODE_GIVEN_MASS && !ctx->two_launch_steps) {
        const TreePlan tp = make_tree_plan(ctx, W, n_pops);
        rc = check_step_lds(ctx, n_pops, tp.depth >= 2 ? B9_STEP_TREE : B9_STEP_FUSED, tp.n_groups);
        if (rc) return rc;
        return tp.depth >= 2 ? run_block_tree(ctx, blk, tp) : run_block_fused(ctx, blk, false);
    }
    if (ctx->opt.mode == B9_MODE_GIVEN_MASS) {          // two launches per step: k_star_like carries the heavy role
        rc = check_step_lds(ctx, n_pops, B9_STEP_STAR_LIKE, 0);
        if (rc) return rc;
    }
    if (ctx->opt.mode == B9_MODE_MARGINALISED && !ctx->two_launch_steps && marg_fused_ok(ctx)) return run_block_fused(ctx, blk, true);
    return run_block_two_launch(ctx, blk, plan);
}

int b9_mcmc_wait(b9_ctx *ctx, b9_mcmc_block *blk)
{
    if (!ctx || !blk || !blk->params || !blk->logpost) return B9_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // blocks are collected in the order they were enqueued: the older outstanding one is in next_slot when both
    // are in flight, else in the other slot
    for (int k = 0; k < 2; ++k) {
        b9_ctx::McmcSlot &sl = ctx->slot[(ctx->next_slot + k) & 1];
        if (sl.in_flight) {
            if (sl.owner != blk) return fail(ctx, B9_ERR_STATE, "b9_mcmc_wait: blocks must be collected in the order they were enqueued");
            return collect_block(ctx, sl, blk);
        }
    }
    return fail(ctx, B9_ERR_STATE, "b9_mcmc_wait: no block is outstanding");
}

}  // extern "C"
