// b9_launch.h -- host-callable launch wrappers of the kernels in b9_kernels.hip.
#pragma once
#include "b9_device.h"
#include "../../include/base9_hip.h"

// A derived isochrone set: the parameter rows and what k_derive_iso makes of them.  Device pointers; the number of rows in use
// is each call's own argument (it changes per chunk).
struct B9IsoSet {
    double *params;             // [rows][B9_NPARAM]: the rows the isochrones are derived from
    IsoHdr *hdr;                // [rows][n_pops]
    double *iso;                // [rows][n_pops][iso_stride]: population k of a row at + k iso_stride
    long long iso_stride;       // doubles of one isochrone (pack_iso_stride)
    int mass_cap;               // rows of one isochrone (pack_mass_cap)
    int n_pops;
    // the set that starts k rows in
    B9IsoSet at(size_t k) const { return B9IsoSet{params + k * B9_NPARAM, hdr + k * n_pops, iso + k * n_pops * iso_stride, iso_stride, mass_cap, n_pops}; }
};

// the star kernel's partial sums: row w at ptr + w stride, n of them in use
struct B9Partial { double *ptr; int n; long long stride; };

// what k_derive_iso needs to FINISH the previous MCMC step before proposing the next one: the star kernel's partials of the
// previous launch, and the previous step's set (its headers: validity; its parameter rows: the proposals)
struct B9Prev { B9Partial partial; B9IsoSet set; };

hipError_t b9k_derive_iso(const DevPack &pk, const B9IsoSet &set, int n_walkers, const McmcDev &mc, const DevPriors &pr, const B9Prev &prev,
                          hipStream_t stream);

// up to 8 HOST rows carried in the kernel arguments (no upload); also stored to set.params for the later launches
hipError_t b9k_derive_iso_rows(const DevPack &pk, const double *host_rows, const B9IsoSet &set, int n_walkers, hipStream_t stream);

// How a launch's hot workgroups take the catalogue's CANONICAL tile groups (b9_star_like.hip.h): n_groups groups of group_tiles
// tiles are fixed by the catalogue (so is the partial-sum layout: 4 per group); a workgroup takes groups_per_block of them,
// n_blocks workgroups per walker.
struct B9Groups { int group_tiles, n_groups, groups_per_block, n_blocks; };

// (partial.n is not read: the plan fixes the layout)
hipError_t b9k_star_like(const DevPack &pk, const DevStars &st, const B9IsoSet &set, int n_walkers, const B9Partial &partial, double *perstar,
                         const B9Groups &gr, int heavy_parts, hipStream_t stream);

hipError_t b9k_finalize(const B9IsoSet &set, const B9Partial &partial, const DevPriors &pr, int n_walkers, double *d_logpost, double *perstar,
                        int n_stars, const McmcDev &mc, hipStream_t stream,
                        unsigned long long *done_flag = nullptr /* [n_walkers] in mapped host memory: done_seq is stored there behind the log-posterior */,
                        unsigned long long done_seq = 0);

// The marginalisation grid of a call and its node tables (device pointers, the caller's own)
struct B9Marg {
    int K, Q;                   // nodes per EEP interval, mass ratios
    bool prune;                 // false: every node of every star is evaluated
    double *tab;                // the call's node table: rows * n_pops * b9k_marg_table_doubles(nfp, mass_cap, K, Q) doubles
    double *wd_tab;             // the WD-stage stars' node table: rows * n_pops * b9k_marg_wd_table_doubles(nfp, K) doubles (read when the
                                // catalogue has WD-stage stars; b9k_marg_tables: null = not built)
    double *shares;             // per-star shares of split launches: rows * b9k_marg_shares_doubles(pieces, n_pops) doubles (the saved-chain
                                // calls and b9k_marg_tables read none)
};

// b9_sample_mass: where the per-star draws go (device pointers), RNG key and the global index of row 0
struct B9MargSample {
    double *mass, *ratio, *member;
    int *pop;
    unsigned k0, k1;
    long long row0;
};

// smp == nullptr: the plain marginal likelihood; else every star also draws one (mass, ratio[, population]) node.
// partial: per walker one sum per 64-star chunk, then one value per WD-stage star (n is not read).  n_cu: compute units of the
// context's device: a split launch of at most 5 workgroups per CU takes the sparse tile setting.
hipError_t b9k_star_marg(const DevPack &pk, const DevStars &st, const B9IsoSet &set, int n_walkers, const B9Partial &partial, double *perstar,
                         const B9Marg &mg, const B9MargSample *smp, int n_cu, hipStream_t stream);
int b9k_marg_split(int n_star_chunks, int n_pops);           // 1: the catalogue's star chunks are split into pieces (DevStars::mg_piece)
long long b9k_marg_shares_doubles(int n_pieces, int n_pops);   // per walker
// the catalogue plan's counting pass (one row, unsplit; the set's isochrones are not read): cost[star chunk][4] = units each wave evaluated
hipError_t b9k_star_marg_cost(const DevPack &pk, const DevStars &st, const B9IsoSet &set, const B9Partial &partial, const B9Marg &mg, unsigned *cost,
                              hipStream_t stream);
long long b9k_marg_table_doubles(int nfp, int mass_cap, int K, int Q);
long long b9k_marg_wd_table_doubles(int nfp, int K);

// marginalised mode, fused sampler step (b9_marg_step.hip.h): decision of step t-1 + stars of step t against one of its two candidate
// node tables + both candidate tables of step t+1 (+ the merge launch of a split catalogue).  sd: StepDev with heavy_parts = 0,
// n_partial = star chunks + WD-stage stars, cand_iso unused.  mg.tab / mg.wd_tab: [2 parities][2 candidates] blocks of n_walkers * n_pops
// tables (cand_at, b9_devbuf.h).  n_cu: as b9k_star_marg's.
hipError_t b9k_marg_step(const DevPack &pk, const DevStars &st, const StepDev &sd, const DevPriors &pr, const B9Marg &mg, int n_cu, hipStream_t stream);
// the tables alone (k_marg_table [+ k_marg_wd_table when mg.wd_tab]) of derived isochrones: the fused block's prologue
hipError_t b9k_marg_tables(const DevPack &pk, const B9IsoSet &set, int n_walkers, const B9Marg &mg, hipStream_t stream);
size_t b9k_marg_step_lds(int nfp, int mass_cap);
// the most dynamic LDS k_marg_step may take and keep the star role's occupancy (7 workgroups per CU up to 8 filters, 4 with 16)
#define B9_MSTEP_LDS_MAX(nfp) ((nfp) > 8 ? (size_t)30 * 1024 : (size_t)15 * 1024)

// fused sampler step (given-mass mode): decision of step t-1 + stars of step t + candidates of step t+1.
// b9k_mcmc_step_desc: the HOST image of a block's descriptor (StepBlockDev, b9_device.h) from the views, sd's block-constant
// fields and the plan; the caller puts it into device memory once per block (the block's upload).
// b9k_mcmc_step: one launch -- desc: that image (sizes the grid), d_desc: its device copy, sd: the launch's own words
// (set, has_prev, derive_next, row, step; nothing else of it is read).
void b9k_mcmc_step_desc(StepBlockDev *desc, const DevPack &pk, const DevStars &st, const StepDev &sd, const DevPriors &pr,
                        const B9Groups &gr, int heavy_parts, int derive_parts,
                        int derive_order /* >= 0: derivation workgroups lead the grid, < 0: they trail it */);
hipError_t b9k_mcmc_step(const StepBlockDev &desc, const StepBlockDev *d_desc, const StepDev &sd, hipStream_t stream);
// resident workgroups per CU of k_mcmc_step's instantiation for this pack (occupancy query; no launch)
hipError_t b9k_mcmc_step_occupancy(const DevPack &pk, int n_pops, int mass_cap, int *blocks_per_cu);
// the block's opening: upload from the mapped host mirror (+ the previous block's final state when continuing), one launch
hipError_t b9k_mcmc_begin(const double *host_up, double *dev, int up_words, const double *prev_final, double *cur0, double *lp0,
                          double *state0, int n_walkers, hipStream_t stream);
// the block's last decision only (one workgroup per walker)
hipError_t b9k_mcmc_finish(const DevPack &pk, const StepDev &sd, const DevPriors &pr, hipStream_t stream);

// LDS the launch that carries a given-mass block's heavy role asks for -- the fused step, the tree launch (n_groups: the
// catalogue's canonical groups, which select the kernel build) or the two-launch form's k_star_like.  Once the tip table
// passes B9_TIPS_LDS_MAX entries the heavy role stages 4 AGB-tip columns of n_age doubles per candidate and population, so the
// age axis bounds it.  The caller refuses a block whose request passes B9_LDS_PER_CU before it launches anything.
#define B9_LDS_PER_CU ((size_t)160 * 1024)
enum B9StepKind { B9_STEP_FUSED, B9_STEP_TREE, B9_STEP_STAR_LIKE };
hipError_t b9k_step_lds(const DevPack &pk, int n_pops, int mass_cap, B9StepKind kind, int n_groups, size_t *dynamic_bytes, size_t *static_bytes);

// tree-speculative step (given-mass mode, few walkers): one launch = `depth` steps of every chain (TreeDev in b9_device.h)
hipError_t b9k_mcmc_tree(const DevPack &pk, const DevStars &st, const TreeDev &td, const DevPriors &pr, int group_tiles /* tiles of a canonical group */,
                         int derive_parts, hipStream_t stream);
hipError_t b9k_mcmc_tree_occupancy(const DevPack &pk, int n_pops, int mass_cap, int n_groups /* of the catalogue: selects the kernel build */, int *blocks_per_cu);
hipError_t b9k_tree_finish(const TreeDev &td, const DevPriors &pr, hipStream_t stream);
hipError_t b9k_tree_begin(const double *host_up, double *dev, int up_words, const double *prev_final, double *state, int n_walkers, hipStream_t stream);

// summary rows of a two-launch block from its chain record on the device (sd: d, n_walkers, n_steps, samples, free_idx, row_origin, rows)
hipError_t b9k_chain_rows(const StepDev &sd, const double *cur_fin, const double *lp_fin, hipStream_t stream);

// b9_predict_mags: n systems at the ONE row of `set`; device pointers; wd_type and pop nullable; out_mags [n][pk.nf] (real filters
// only), out_stage [n]; at most n_wgs workgroups
hipError_t b9k_predict_mags(const DevPack &pk, const B9IsoSet &set, long long n, const double *mass1, const double *mass_ratio, const int *wd_type,
                            const int *pop, double *out_mags, int *out_stage, int n_wgs, hipStream_t stream);
size_t b9k_predict_lds(int nfp, int mass_cap, int n_pops);      // its dynamic LDS per workgroup, bytes (at most 160 KB launches)

// b9_sample_wd_mass: where the draws go (device pointers, [n_rows][st.n_wd]; the five derived ones and pop nullable), RNG key and
// the global index of row 0
struct B9WdSample {
    double *zams, *wd_mass, *prec_log_age, *log_cool_age, *log_teff, *logg, *member;
    int *pop;
    unsigned k0, k1;
    long long row0;
};
// The node table of the three WD-grid calls, doubles per (row, population): k_wd_node_table's, or with status k_wd_node_table_status'
// (every node's wd_chain status behind it)
long long b9k_wd_grid_table_doubles(int nfp, long long n_nodes, bool status);

// What a WD-grid call works on, one chunk of n_rows derived rows (n_rows * n_pops <= 65535).  Device pointers, all the caller's own.
struct B9WdGrid {
    B9IsoSet set;               // the chunk's rows
    int n_nodes;                // of the call's mass grid
    double *tab;                // n_rows * n_pops * b9k_wd_grid_table_doubles doubles (the draws: without status, the other two: with)
    int *rank;                  // [st.n] the column of every star (rank[original index]: the WD-stage stars before it); only read
    double *scratch;            // the chunk's words [n_rows][lines][n_col] (the draws do not read it: their columns travel in B9WdSample)
    double *acc;                // [lines][n_col] += the rows in ascending order (the draws: null)
    double *edges;              // b9_wd_bins: [st.n_wd][n_sel][n_bins + 1], validated by the caller (else null); only read
};
// k_wd_node_table + k_wd_sample
hipError_t b9k_wd_sample(const DevPack &pk, const DevStars &st, const B9WdGrid &g, int n_rows, const B9WdSample &smp, hipStream_t stream);
// b9_wd_moments: k_wd_node_table_status + k_wd_moments: every WD-stage star's sixteen increments into scratch
// [n_rows][st.n_wd][B9_WDM_N], then acc [st.n_wd][B9_WDM_N]
hipError_t b9k_wd_moments(const DevPack &pk, const DevStars &st, const B9WdGrid &g, int n_rows, hipStream_t stream);
// b9_wd_bins: k_wd_node_table_status (b9_wd_moments' table, built once per chunk) + k_wd_bins: every (WD-stage star, selected
// quantity)'s increments on its own edges into scratch [n_rows][st.n_wd][n_sel][n_bins + 3] (below, the bins, at or above, the
// total), then acc [st.n_wd][n_sel][n_bins + 3]; n_sel: the bits of quantity_mask
hipError_t b9k_wd_bins(const DevPack &pk, const DevStars &st, const B9WdGrid &g, int n_rows, int quantity_mask, int n_bins, hipStream_t stream);

// b9_cmd_band: the call's spec as the kernels take it (by value), validated by the caller
struct B9BandSpec {
    int eep0, n_eep, n_ratio;
    int n_wd_nodes, n_types, type_id[2];         // type_id[t]: the atmosphere type (0 DA, 1 DB) of the t-th selected one
    int n_colour, colour[B9_BAND_MAX_COLOURS][2];
    int P, C;                                    // points per population, columns per point (1 + nf + n_colour)
    long long n_lines;                           // n_pops P C
    double ratio[B9_BAND_MAX_RATIOS];
};
// ... and what it works on, one chunk of n_rows derived rows (n_rows * n_pops <= 65535).  Device pointers, all the caller's own.
struct B9Band {
    B9IsoSet set;               // the chunk's rows
    B9BandSpec spec;
    double *wd_tab;             // n_rows * n_pops * b9k_wd_grid_table_doubles(nfp, n_wd_nodes, true) doubles (n_wd_nodes == 0: not read)
    double *values;             // the chunk's value table [n_rows][n_lines]
    double *pivot;              // [n_lines]; only read
    double *mom;                // [n_lines][B9_BAND_NMOM], in/out (null: not asked for)
    double *bins;               // [n_lines][n_bins + 3], in/out (null: not asked for)
    double *edges_t;            // [n_bins + 1][n_lines]: the lines' edges TRANSPOSED, validated by the caller (read with bins); only read
    int n_bins;
};
// k_derive_iso'd rows -> [k_wd_node_table_status] + k_band_points + k_band_wd_points (the value table) + k_band_accumulate
hipError_t b9k_cmd_band(const DevPack &pk, const B9Band &b, int n_rows, hipStream_t stream);

// What a reduction over a saved chain works on, one chunk of n_rows derived rows (1 .. 65535).  Device pointers, all the caller's own.
struct B9Chain {
    B9IsoSet set;               // the chunk's rows
    B9Marg mg;                  // the grid; tab / wd_tab are built here per chunk (k_marg_table [+ k_marg_wd_table])
    double *scratch;            // every star's increments of the chunk, [n_rows][st.n][the call's columns]
    double *acc;                // [st.n][the call's accumulator words] += the rows in ascending order (null where the call allows: not asked for)
    double *rows;               // [n_rows][the call's row words]: the stars' sum in ascending order (null: not asked for)
};

// b9_star_moments: every star's eight increments into scratch [n_rows][st.n][B9_MOM_N], then acc [st.n][B9_MOM_N]
hipError_t b9k_star_moments(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, hipStream_t stream);

// b9_mass_hist: every star's binned increments into scratch [n_rows][st.n][n_bins + 1], then acc [st.n][n_bins + 1] (may be null)
// and rows [n_rows][n_bins + 1] (may be null).  edges: HOST, [n_bins + 1], validated by the caller; they travel as kernel arguments.
hipError_t b9k_mass_hist(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, int quantity, const double *edges, int n_bins,
                         hipStream_t stream);

// b9_ratio_hist: every star's (primary-mass bin, ratio node) increments into scratch [n_rows][st.n][n_mbins Q + 1] (Q = c.mg.Q,
// at most B9_RH_MAX_Q), then acc [st.n][n_mbins Q + 1] (may be null) and rows [n_rows][n_mbins Q + 1] (may be null).
// mass_edges: HOST, [n_mbins + 1], validated by the caller; they travel as kernel arguments.
#define B9_RH_MAX_Q 64
hipError_t b9k_ratio_hist(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, const double *mass_edges, int n_mbins, hipStream_t stream);

// b9_star_bins: every star's increments on its own edges into scratch [n_rows][st.n][n_bins + 3] (below, the bins, at or above, the
// total), then acc [st.n][n_bins + 3].  edges: DEVICE, [st.n][n_bins + 1] in the caller's star order, validated by the caller.
hipError_t b9k_star_bins(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, int quantity, const double *edges, int n_bins,
                         hipStream_t stream);

// b9_phot_resid.  b9k_resid_stage: the call's pivots piv_in [st.n][pk.nf] (the caller's star order) into the mg_* copy's order,
// piv_mg [st.mg_pad / 64][pk.nfp][64].  b9k_phot_resid: every star's increments into scratch [n_rows][st.n][2 + 2 nf], then acc
// [st.n][2 + 2 nf] (may be null) and rows [n_rows][1 + 5 nf] = the stars' standardised sums (may be null; isig [st.n][nf] =
// 1 / sigma, 0 for an unused filter, is read for them only).
hipError_t b9k_resid_stage(const DevPack &pk, const DevStars &st, const double *piv_in, double *piv_mg, hipStream_t stream);
hipError_t b9k_phot_resid(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, const double *piv_mg, const double *isig, hipStream_t stream);

// b9_filter_loo: every star's increments into scratch [n_rows][st.n][2 + 3 nf], then acc [st.n][2 + 3 nf] (may be null) and rows
// [n_rows][1 + 6 nf] (may be null; isig as b9k_phot_resid's).  piv_mg, lsn_mg: the pivots and log(sigma sqrt(2 pi)) (0 for an
// unused filter) in the mg_* copy's order (b9k_resid_stage); lsn [st.n][nf]: the latter in the caller's star order.
hipError_t b9k_filter_loo(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, const double *piv_mg, const double *lsn_mg, const double *lsn,
                          const double *isig, hipStream_t stream);

// b9_star_offset.  The call's directions: k [n_dir][nf] and tau [n_dir] on the HOST (they travel as kernel arguments); c_in
// [n_dir][st.n][nf] the scaled directions k_f / sigma_f (0: filter unused) in the caller's star order, and what b9k_offset_stage
// forms from them: c_mg [n_dir][mg_pad][nfp] in the mg_* copy's order, cv [st.n][n_dir][2] = {C, V} and ob [st.n][n_dir][2] = {the
// pruning factor, the Occam term} (device).
struct B9Offset {
    int n_dir;
    const double *k, *tau;
    const double *c_in;
    double *c_mg, *cv, *ob;
};
hipError_t b9k_offset_stage(const DevPack &pk, const DevStars &st, const B9Offset &o, hipStream_t stream);
// every star's increments into scratch [n_rows][st.n][2 + 3 n_dir], then acc [st.n][2 + 3 n_dir] (may be null) and rows
// [n_rows][1 + 4 n_dir] (may be null)
hipError_t b9k_star_offset(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, const B9Offset &o, hipStream_t stream);

// rows of one b9k_pointwise launch: the reducers hold a chunk's rows in registers (k_pw_accumulate, k_pw_tail), and b9_pointwise
// chunks its rows by the same number
#define B9_PW_MAX_ROWS 32
// b9_pointwise: every star's v = finish_star().v into scratch [n_rows][st.n] (n_rows <= B9_PW_MAX_ROWS) and row_in [n_rows] (1: the
// row lies inside the grid; 0: it wrote no value), then -- each optional -- acc [st.n][B9_PW_N] through the recurrence, rows
// ascending; tail [tail_len][st.n] (the DEVICE layout) the largest -v; rows [n_rows].  b9k_pw_tail_load: tail from the caller's
// layout tail_io [st.n][tail_len], or -inf everywhere when tail_io is null; b9k_pw_tail_store: back to it.  Device pointers.
hipError_t b9k_pw_tail_load(const double *tail_io, int n_stars, int tail_len, double *tail, hipStream_t stream);
hipError_t b9k_pw_tail_store(const double *tail, int n_stars, int tail_len, double *tail_io, hipStream_t stream);
hipError_t b9k_pointwise(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, int *row_in, double *tail, int tail_len, hipStream_t stream);

// b9_star_influence: b9k_pointwise's values and row_in, then -- each optional -- acc [st.n][B9_INF_N(n_q)] through the influence
// recurrence (k_infl_accumulate), tail as b9k_pointwise's, rows [n_rows][n_groups] the groups' sums (k_infl_groups).  q [n_rows][n_q]:
// the chunk's rows of the caller's quantities; group [st.n]: the stars' group ids, the caller's order.  Device pointers.
struct B9Influence {
    int n_q;
    const double *q;
    int n_groups;
    const int *group;
};
hipError_t b9k_star_influence(const DevPack &pk, const DevStars &st, const B9Chain &c, int n_rows, int *row_in, double *tail, int tail_len, const B9Influence &f,
                              hipStream_t stream);

hipError_t b9k_noop(hipStream_t stream);
hipError_t b9k_spin(double microseconds, hipStream_t stream);
constexpr int B9_CLOCK_SLOTS = 8 * 256;      // (XCD, HW_ID[15:8]) -> one slot per compute unit
hipError_t b9k_clock_stamp(unsigned long long *d_out /* [B9_CLOCK_SLOTS][2] */, hipStream_t stream);
