/*
 * base9_hip.h -- C ABI of the MI355X-native BASE-9 per-step log-posterior path.
 *
 * This is the drop-in boundary of the hot path.  In the reference
 * the boundary is an in-process C++ call -- the MCMC driver calls "logPost(proposed cluster)"
 * once per step, which derives one isochrone from the loaded model pack and loops over the
 * cluster's stars.  That source is NOT mounted (/root/reference/README.md:4 redirects to
 * BayesianStellarEvolution/base-cpp), so no entry point below can cite a reference file:line;
 * each cites instead the SURVEY.md section-8a row it implements and, tagged [RECALL], the
 * upstream function it is believed to replace.  Parity with BASE-9 is therefore UNPINNED.
 *
 * Conventions
 *  - plain C structs, plain pointers and sizes; no C++/torch types cross this boundary;
 *  - the caller owns every host buffer passed in; the context owns all device memory;
 *  - every function returns B9_OK (0) or a negative b9_status; b9_last_error() gives text;
 *  - proposed parameters outside the model grid are NOT an error: that walker's
 *    log-posterior is -INFINITY (the reference rejects such a step [RECALL]);
 *  - one context per GPU, not thread-safe, all work stream-ordered on the context's stream;
 *  - there is NO CPU fallback: without a HIP device b9_ctx_create fails with B9_ERR_NO_DEVICE.
 */
#ifndef BASE9_HIP_H
#define BASE9_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define B9_ABI_VERSION 6

/* ---- status codes ------------------------------------------------------------------ */
typedef enum b9_status {
    B9_OK = 0,
    B9_ERR_NO_DEVICE = -1,   /* no HIP device / HIP runtime failure at create            */
    B9_ERR_INVALID   = -2,   /* bad argument (NULL, negative size, unsorted axis ...)    */
    B9_ERR_STATE     = -3,   /* call order: pack/stars not loaded yet                    */
    B9_ERR_HIP       = -4,   /* a HIP call failed; see b9_last_error                     */
    B9_ERR_CAPACITY  = -5    /* table too large for the kernel's LDS plan                */
} b9_status;

/* ---- cluster parameter row ([RECALL] Cluster::getParam order) ------ */
enum {
    B9_P_LOGAGE = 0,      /* log10(age/yr)                                              */
    B9_P_Y = 1,           /* helium mass fraction (population A in a two-pop run)        */
    B9_P_FEH = 2,         /* [Fe/H]                                                      */
    B9_P_MOD = 3,         /* distance modulus (m-M)_V, includes A_V                      */
    B9_P_ABS = 4,         /* absorption A_V                                              */
    B9_P_CARBONICITY = 5, /* WD core carbon fraction                                     */
    B9_P_IFMR_INTERCEPT = 6,
    B9_P_IFMR_SLOPE = 7,
    B9_P_IFMR_QUAD = 8,
    B9_P_Y2 = 9,          /* helium of population B (two-pop only; [RECALL] multiPopMcmc)*/
    B9_P_LAMBDA = 10,     /* fraction of stars in population A (two-pop only)            */
    B9_P_RESERVED = 11,
    B9_NPARAM = 12        /* row stride, in doubles                                      */
};

/* ---- star status codes ([RECALL] .phot "stage" column) -------------------------------- */
enum { B9_STAGE_MSRG = 1, B9_STAGE_WD = 3, B9_STAGE_NSBH = 4, B9_STAGE_BD = 5, B9_STAGE_DNE = 9 };

/* ---- IFMR ids ----------------------------------------------------- */
enum {
    B9_IFMR_WEIDEMANN = 0, B9_IFMR_WILLIAMS = 1, B9_IFMR_SALARIS_LIN = 2,
    B9_IFMR_SALARIS_PW = 3, B9_IFMR_LINEAR = 4, B9_IFMR_QUADRATIC = 5
};

/* Magnitude assigned to "contributes no flux" ([RECALL] 99.999 sentinel). */
#define B9_MAG_NOFLUX 99.999

/*
 * Model pack: the tables a loaded MS/RGB model + WD cooling model + WD atmosphere model +
 * filter set expose to the hot path ([RECALL] MsRgbModel /
 * WdCoolingModel / WdAtmosphereModel / Model aggregate).  All axes strictly ascending.
 *
 * Isochrone (ifeh, iy, iage) has index  iso = (ifeh * n_y + iy) * n_age + iage,  holds
 * iso_n_eep[iso] evolutionary points whose EEP ids are iso_first_eep[iso] + 0,1,2,...  and
 * whose data start at point offset iso_offset[iso] in mass[] / mags[] (mags point-major:
 * mags[(off + k) * n_filt + f]).  Masses ascend along an isochrone.
 */
typedef struct b9_pack {
    int32_t n_filt;
    /* MS/RGB grid */
    int32_t n_feh, n_y, n_age;
    const double *feh;            /* [n_feh]                                             */
    const double *y;              /* [n_y]   (n_y == 1: helium is not a grid axis)        */
    const double *log_age;        /* [n_age]                                             */
    const int32_t *iso_first_eep; /* [n_feh*n_y*n_age]                                   */
    const int32_t *iso_n_eep;     /* [n_feh*n_y*n_age]                                   */
    const int64_t *iso_offset;    /* [n_feh*n_y*n_age]                                   */
    int64_t n_points;             /* total evolutionary points                            */
    const double *mass;           /* [n_points]                                          */
    const double *mags;           /* [n_points*n_filt]                                   */
    const double *abs_coeff;      /* [n_filt]  A_f / A_V                                  */
    /* WD cooling model (ABI 2): one cooling track per (carbonicity, WD mass) node, EACH WITH ITS OWN cooling-age axis --
     * real cooling tracks are ragged: every mass was evolved over its own sequence of ages.  Track (ic, im) has index
     * t = ic * n_wc_mass + im and holds wc_n_age[t] >= 2 points (log cooling age strictly ascending) starting at point
     * offset wc_offset[t] of wc_log_age / wc_log_teff / wc_log_radius.  A lookup brackets the cooling age in each of
     * the (2 carbonicities x) 2 masses' own axes, interpolates along each track, then across mass, then across
     * carbonicity.  n_wc_mass == 0: no WD models.  n_wc_carb <= 1: carbonicity is not an axis. */
    int32_t n_wc_carb, n_wc_mass;
    const double *wc_carb;        /* [n_wc_carb]                                         */
    const double *wc_mass;        /* [n_wc_mass] WD mass, Msun                            */
    const int32_t *wc_n_age;      /* [max(1,n_wc_carb)*n_wc_mass] points of each track      */
    const int64_t *wc_offset;     /* [max(1,n_wc_carb)*n_wc_mass] first point of each track */
    int64_t n_wc_points;          /* total cooling-track points                           */
    const double *wc_log_age;     /* [n_wc_points] log10 cooling age / yr                 */
    const double *wc_log_teff;    /* [n_wc_points]                                       */
    const double *wc_log_radius;  /* [n_wc_points] log10 R / cm                           */
    /* WD atmospheres: [n_at_type][n_at_logg][n_at_teff][n_filt], type 0 = DA, 1 = DB      */
    int32_t n_at_type, n_at_logg, n_at_teff;
    const double *at_logg;        /* [n_at_logg]                                         */
    const double *at_log_teff;    /* [n_at_teff]                                         */
    const double *at_mags;        /* [n_at_type*n_at_logg*n_at_teff*n_filt]              */
    /* IFMR + mass limits */
    int32_t ifmr_id;
    int32_t reserved0;
    double m_wd_up;               /* upper ZAMS mass that still makes a WD ([RECALL] M_wd_up) */
} b9_pack;

/*
 * Stars: what the photometry file gives per stellar system ([RECALL]
 * StellarSystem).  obs/sigma are star-major as read from the file: obs[i * n_filt + f].
 * sigma < 0 (or == 0) marks a filter as unused for that star.
 */
typedef struct b9_stars {
    int32_t n_stars, n_filt;
    const double *obs;            /* [n_stars*n_filt] observed magnitudes                 */
    const double *sigma;          /* [n_stars*n_filt] 1-sigma errors, <=0 -> unused       */
    const double *mass1;          /* [n_stars] primary ZAMS mass, Msun                    */
    const double *mass_ratio;     /* [n_stars] secondary/primary, 0 -> single             */
    const double *clust_prior;    /* [n_stars] prior cluster-membership probability       */
    const int32_t *stage;         /* [n_stars] B9_STAGE_* (used by the marginalised mode) */
    const int32_t *wd_type;       /* [n_stars] 0 DA, 1 DB; may be NULL (all DA)           */
    const double *filter_prior_min; /* [n_filt] field-star magnitude range ...           */
    const double *filter_prior_max; /* [n_filt] ... fsLike = prod_f 1/(max-min)           */
} b9_stars;

/* Cluster-level priors (SURVEY section 2 "Priors"; scalar per walker, added on device).   */
typedef struct b9_priors {
    double mean[B9_NPARAM];       /* Gaussian prior means                                 */
    double var[B9_NPARAM];        /* variances; <= 0 -> flat (no term)                    */
    double log_age_min, log_age_max; /* flat prior support in logAge; outside -> -inf      */
} b9_priors;

/* Evaluation modes */
enum {
    B9_MODE_GIVEN_MASS   = 0,  /* BASELINE.json north_star: one interpolation per star at its (mass1, mass_ratio) */
    B9_MODE_MARGINALISED = 1   /* [RECALL] marg.cpp: integrate each star over primary mass and mass ratio        */
};

typedef struct b9_options {
    int32_t mode;             /* B9_MODE_*                                                */
    int32_t n_pops;           /* 1 (singlePopMcmc) or 2 (multiPopMcmc)                    */
    int32_t marg_iso_increm;  /* sub-steps per EEP interval in the primary-mass integral  */
    int32_t marg_n_q;         /* mass-ratio quadrature nodes                              */
} b9_options;

/*
 * Launch-plan tuning (ABI 4).  Every field 0 = automatic (what a context starts with); results are the same for every
 * setting to the stated tolerance -- these only regroup the same work (tests/test_gpu_mcmc.py runs the combinations).
 * The one field that touches the ROUNDING of a walker's log-posterior is tiles_per_block: the catalogue's tiles are dealt
 * into canonical groups of that many tiles and every wave forms one partial per group.  Its automatic value is a function
 * of the catalogue, the pack, the options and the device ONLY -- not of the number of walkers on the GPU -- so a walker's
 * chain is the same bits whatever the number of GPUs the walkers are spread over (since ABI 4; before, the automatic value
 * followed the local walker count and a driver had to pin it).
 * The same fields can be set through the environment, read ONCE when the context is created: B9_TILES_PER_BLOCK,
 * B9_DERIVE_PARTS, B9_DERIVE_ORDER (historical coding: 1 default, 0 heavy first, < 0 derivation trails), B9_HEAVY_PARTS,
 * B9_TWO_LAUNCH_STEPS, B9_MARG_NO_PRUNING, B9_TIMING_GROUP, B9_PLAN_DEBUG, B9_TREE_DEPTH;
 * B9_STREAM_PRIORITY=default gives the context's stream the default priority instead of the lowest.
 */
typedef struct b9_tuning {
    int32_t tiles_per_block;   /* star tiles (256 stars) per CANONICAL tile group of k_star_like / k_mcmc_step / k_mcmc_tree  */
    int32_t derive_parts;      /* fused step: workgroups per candidate isochrone                                         */
    int32_t derive_order;      /* fused step grid: 1 writers + derivation lead (default), 2 heavy-star workgroups lead,  */
                               /* 3 derivation workgroups trail the hot ones                                            */
    int32_t heavy_parts;       /* workgroups per walker for the stars above the AGB tip (default: sized from the catalogue) */
    int32_t two_launch_steps;  /* 1: the derive + star launch pair per sampler step also in given-mass mode                */
    int32_t marg_no_pruning;   /* 1: marginalised kernel evaluates every node of every star (no floor, no boxes): the      */
                               /* brute-force statement of the same sum on the GPU, for tests                            */
    int32_t timing_group;      /* launches per HIP-event bracket of b9_enable_timing in the fused step (default 8)        */
    int32_t plan_debug;        /* 1: print the fused step's launch plan to stderr whenever it changes; 2: also the marginalised catalogue's pieces */
    int32_t tree_depth;        /* given-mass sampler blocks: Metropolis steps per launch.  1 = the one-step fused launch;   */
                               /* 2 / 3 = the tree-speculative launch (every proposal of the chain's next 2 / 3 steps --   */
                               /* 3 / 7 of them -- evaluated at once, same chain); default: the deepest tree whose          */
                               /* workgroups are all resident at once AND whose estimated cost per step beats the one-step  */
                               /* launch's (few walkers per GPU, catalogues that leave the chip under-filled), else 1.      */
                               /* Env: B9_TREE_DEPTH                                                                        */
    int32_t marg_piece_units;  /* marginalised mode, small catalogues: the smallest share of a star chunk's node window worth a   */
                               /* workgroup of its own, in (16 nodes x one mass ratio) units per wave (default 4; 6 from 8 mass ratios on).  Part of what a */
                               /* star's sum rounds like: every rank of a run must use the same value.  Env: B9_MARG_PIECE_UNITS   */
    int32_t reserved[6];
} b9_tuning;

typedef struct b9_ctx b9_ctx;

/* ---- lifecycle ---------------------------------------------------------------------- */
int         b9_abi_version(void);
/* device_id < 0 -> current device.  Fails with B9_ERR_NO_DEVICE when no GPU is present.  */
int         b9_ctx_create(int device_id, b9_ctx **out);
void        b9_ctx_destroy(b9_ctx *ctx);
const char *b9_last_error(const b9_ctx *ctx);   /* ctx may be NULL: last create error      */

/* ---- staging (cold; once per run) ---------------------------------------------------- */
/* A staging or configuration call that is REFUSED for its arguments (B9_ERR_INVALID, B9_ERR_CAPACITY: a pack of more than
 * 16 filters, non-finite photometry in a filter in use, n_pops = 3, ...) changes nothing: both loaders validate the whole
 * table before they touch the context, so the next evaluating call returns the bits of the configuration in force before the
 * refused call (tests/test_gpu_history.py pins this).  Only a HIP failure in the middle of an upload (B9_ERR_HIP) leaves the
 * context without a pack; evaluating calls then return B9_ERR_STATE until a valid b9_load_pack.
 * A pack may be reloaded under loaded stars when it has the same number of filters: the stars are staged again against it
 * at the next evaluating call.  With another filter count every call that needs the stars is B9_ERR_INVALID until matching stars are loaded. */
/* Replaces [RECALL] Model construction: copies the pack's tables to HBM.                   */
int b9_load_pack(b9_ctx *ctx, const b9_pack *pack);
/* Replaces [RECALL] reading the .phot into vector<StellarSystem>: SoA + staged to HBM.     */
int b9_load_stars(b9_ctx *ctx, const b9_stars *stars);
int b9_set_priors(b9_ctx *ctx, const b9_priors *priors);
int b9_set_options(b9_ctx *ctx, const b9_options *opt);
/* tuning NULL = everything automatic again.  Not while a block is outstanding. */
int b9_set_tuning(b9_ctx *ctx, const b9_tuning *tuning);
/* The tuning in force: the B9_* environment overrides read at creation, then whatever the last b9_set_tuning passed -- a
 * caller that wants to change ONE field reads, modifies and writes back (ABI 4). */
int b9_get_tuning(const b9_ctx *ctx, b9_tuning *out);

/* ---- the hot path -------------------------------------------------------------------- */
/*
 * Log-posterior of n_walkers proposed parameter rows ([RECALL]
 * MpiMcmcApplication::logPostStep).  params: host, [n_walkers * B9_NPARAM].
 * out_logpost: host, [n_walkers].  out_perstar: host, [n_walkers * n_stars] per-star
 * log( (1-p) fsLike + p L_i ) in the ORIGINAL star order, or NULL.
 * Synchronous (returns after the results are on the host).
 */
int b9_logpost(b9_ctx *ctx, const double *params, int32_t n_walkers,
               double *out_logpost, double *out_perstar);

/*
 * Same, device-resident and asynchronous: d_params / d_logpost (/ d_perstar, nullable) are
 * DEVICE pointers; launches on `stream` (a hipStream_t passed as void*, NULL = the context's
 * stream) and returns without synchronising.  This is the entry the walker-parallel driver
 * uses so that the RCCL all-gather reads log-posteriors straight from HBM.
 */
int b9_logpost_device(b9_ctx *ctx, const double *d_params, int32_t n_walkers,
                      double *d_logpost, double *d_perstar, void *stream);

/*
 * Device-resident Metropolis block: advances the n_walkers local chains n_steps steps without
 * returning to the host between steps (SURVEY 8f row 1 -- the per-step caller of the hot path;
 * [RECALL] the body of MpiMcmcApplication's sampling loop: propose from the adapted covariance,
 * logPost, accept/reject).  Per step and walker w: z ~ N(0, I_d) and u ~ U(0,1) from the
 * counter-based stream Philox4x32-10(key = seed, counter = (step, walker_ids[w], draw));
 * proposal = current, proposal[free_idx[i]] += sum_j chol[i*d+j] z_j; accepted when
 * log u < logpost(proposal) - logpost(current).  All pointers are HOST pointers; params and
 * logpost are updated in place; samples ([n_steps][n_walkers][n_free]) and lps
 * ([n_steps][n_walkers]) receive the chain and may be NULL.  Synchronous.
 */
typedef struct b9_mcmc_block {
    int32_t n_walkers, n_free;
    const int32_t *free_idx;     /* [n_free] parameter indices being sampled                  */
    const double *chol;          /* [n_free*n_free] row-major proposal factor                 */
    const int32_t *walker_ids;   /* [n_walkers] global walker ids (random-number streams)     */
    uint64_t seed;
    int64_t step0;               /* global number of the block's first step                   */
    int32_t n_steps, flags;      /* flags: B9_BLOCK_* (0 = start from params/logpost, synchronous)          */
    double *params;              /* [n_walkers*B9_NPARAM] in/out                              */
    double *logpost;             /* [n_walkers] in/out                                        */
    double *samples;             /* out, nullable                                             */
    double *lps;                 /* out, nullable                                             */
    int64_t n_accept;            /* out                                                       */
    /* ---- block summary rows (ABI 2; both evaluation modes since ABI 3).  row_origin != NULL: the block's last launch also condenses
     * every walker's chain into ONE row of B9_ROW_DOUBLES(n_free) doubles on the device,
     *     [0] log-posterior after the block   [1..12] position after the block
     *     [13] steps after the block's first on which the walker moved   [14] n_steps
     *     [15 .. 15+d) sum_s x_s    [15+d .. 15+d+d*d) sum_s x_s x_s^T (row-major),   x_s = sample_s - row_origin,
     * sums over the steps in ascending order, plain multiply and add.  These rows are what a walker-parallel driver
     * exchanges between GPUs for the adaptive proposal: d_rows is their DEVICE address (valid until the second-next
     * block of this context is enqueued) and rows_ready (flag B9_BLOCK_ROWS_EVENT) a hipEvent_t recorded on the context's
     * stream once they are written, so a collective on another stream can read them from HBM without a host round trip.  `rows` (host,
     * nullable) receives a copy when the block is collected. */
    const double *row_origin;    /* [n_free] or NULL                                          */
    double *rows;                /* out, nullable: [n_walkers][B9_ROW_DOUBLES(n_free)]         */
    void *d_rows;                /* out: device pointer to the same rows                       */
    void *rows_ready;            /* out: hipEvent_t                                            */
} b9_mcmc_block;
#define B9_ROW_DOUBLES(d) (15 + (d) + (d) * (d))
/* B9_ERR_CAPACITY (given-mass mode, every launch form): the pack is too large for the LDS of the kernel that carries the heavy
 * role -- which stages 4 AGB-tip columns of n_age doubles per candidate and population once the tip table passes 2048 entries,
 * so in practice the age axis is too long.  Refused before anything is uploaded or launched; the message names the axis length
 * (or, with the tips staged whole, the pack's table sizes) and the bytes asked for. */
int b9_mcmc_run_block(b9_ctx *ctx, b9_mcmc_block *blk);

/*
 * Pipelining blocks (both evaluation modes; a block may only continue a block of the same mode).  B9_BLOCK_ASYNC: b9_mcmc_run_block returns as soon as the block is
 * enqueued on the context's stream; b9_mcmc_wait(ctx, blk) -- same blk, whose host arrays must stay valid --
 * blocks until it has run and fills params / logpost / samples / lps / n_accept.  B9_BLOCK_CONTINUE: the block
 * starts from the state the PREVIOUS block of this context left on the device (its params / logpost inputs are
 * ignored; n_walkers must match), so it can be enqueued before that block has finished.  At most two blocks
 * may be outstanding; they are collected in the order they were enqueued.  A successful b9_load_pack, b9_load_stars,
 * b9_set_priors or b9_set_options changes the posterior: the previous block's state carries a log-posterior of the old
 * one, so the next B9_BLOCK_CONTINUE block returns B9_ERR_STATE (the message names the call that intervened) and the chain
 * restarts from host state.  b9_set_tuning (plans change rounding only), b9_predict_mags, b9_sample_wd_mass, b9_star_moments,
 * b9_wd_moments, b9_wd_bins, b9_mass_hist, b9_ratio_hist, b9_phot_resid, b9_filter_loo, b9_star_offset, b9_pointwise and b9_star_influence (buffers of their own) between continued blocks are allowed.  While a block is outstanding it owns the
 * context's work buffers: b9_logpost / b9_sample_mass / b9_derive_isochrone, the staging calls, b9_set_options and a block
 * with another n_walkers return B9_ERR_STATE until it has been collected.  A driver that adapts the proposal
 * from block b-1 while block b runs keeps the GPU's queue non-empty: enqueue b+1 (CONTINUE | ASYNC), wait(b), ...
 */
#define B9_BLOCK_CONTINUE 1
#define B9_BLOCK_ASYNC 2
#define B9_BLOCK_ROWS_EVENT 4   /* with row_origin: also record rows_ready (a multi-GPU exchange waits on it); off, one event less in the stream */
int b9_mcmc_wait(b9_ctx *ctx, b9_mcmc_block *blk);

/*
 * Per-star mass posterior draws (the sampleMass counterpart; [RECALL] sampleMass
 * re-reads the cluster chain and, for every saved row and every star, draws the primary mass and the
 * mass ratio from the star's conditional posterior on a grid, and reports the membership
 * probability).  The grid is the one of the marginalised mode (b9_options.marg_iso_increm sub-steps
 * per EEP interval x marg_n_q mass ratios; WD-stage stars: 8 * marg_iso_increm steps above the AGB
 * tip), whatever b9_options.mode says.  For row r (a full parameter row, as in b9_logpost) and star
 * i ONE node is drawn by the Gumbel-max rule: argmax over nodes of
 *     log( prior(M1) dM / n_q * like_i(M1, q) [* lambda_k] )  -  log(-log u),
 *     u = Philox4x32-10(key = (seed lo, seed hi ^ row hi), counter = (row lo, i, node lo, 2 * node hi + k)),
 * node = (EEP interval * marg_iso_increm + sub-step) * n_q + j for main-sequence/giant nodes and the
 * step number for WD nodes, k = population; row = row0 + r.  An argmax does not depend on the order
 * in which nodes are visited, so any implementation picks the same node.
 * Outputs, host, [n_rows][n_stars] in the caller's star order: out_mass (primary mass of the node),
 * out_ratio (j / n_q; 0 for WD nodes), out_member = p_i L_i / (p_i L_i + (1 - p_i) fieldLike),
 * out_pop (0 / 1; may be NULL).  A row outside the grid gives mass = ratio = member = 0.
 */
int b9_sample_mass(b9_ctx *ctx, const double *params, int32_t n_rows, uint64_t seed, int64_t row0,
                   double *out_mass, double *out_ratio, double *out_member, int32_t *out_pop);

/*
 * Derive the isochrone for one parameter row ([RECALL]
 * MsRgbModel::deriveIsochrone; this is all that makeCMD needs).  Outputs, host:
 * out_mass[cap], out_mags[cap*n_filt] (absolute magnitudes, no modulus/absorption),
 * *out_first_eep, *out_n (0 when the row is outside the grid).  pop = 0 uses B9_P_Y,
 * pop = 1 uses B9_P_Y2.
 */
int b9_derive_isochrone(b9_ctx *ctx, const double *param_row, int32_t pop, int32_t cap,
                        double *out_mass, double *out_mags,
                        int32_t *out_first_eep, int32_t *out_n, double *out_agb_tip);

/*
 * Predicted apparent magnitudes of n stellar systems at one parameter row (the forward half of rows a4-a7, a9; [RECALL]
 * what simCluster evaluates per star).  Added in ABI 6 without a version change: it is purely additive, and nothing
 * else in this header changed.  Needs a loaded pack, not loaded stars, and never touches the stars or the work buffers
 * a sampler block uses (a B9_BLOCK_CONTINUE block enqueued after this call gives the same bits as one enqueued without
 * it); B9_ERR_STATE while a block is outstanding.  All pointers are host pointers; synchronous, like b9_sample_mass.
 * System i: primary ZAMS mass mass1[i] (finite), mass ratio mass_ratio[i] >= 0 (0 = single), wd_type[i] (0 DA, 1 DB;
 * NULL = all DA), pop[i] (0 uses B9_P_Y, 1 uses B9_P_Y2 as b9_derive_isochrone does; NULL = all 0; the second
 * isochrone is derived only when some system needs it).  out_mags [n * n_filt] receives exactly what the likelihood
 * compares with obs: the primary's magnitudes (MS/RGB, the WD branch, or B9_MAG_NOFLUX below the isochrone's first mass
 * and above m_wd_up), flux-combined with the secondary at mass_ratio * mass1 when mass_ratio > 0, plus
 * mod + (abs_coeff - 1) * Av -- except that a filter in which neither component gives flux is exactly B9_MAG_NOFLUX.
 * out_stage (nullable, [n]): B9_STAGE_MSRG for mass1 <= the population's AGB tip, B9_STAGE_WD up to m_wd_up,
 * B9_STAGE_NSBH above.  A row outside the grid (for a system's population) is not an error: that system's magnitudes
 * are all B9_MAG_NOFLUX and its stage B9_STAGE_DNE.  Every system's result depends on that system alone, so results are
 * the same bits however the systems are batched or ordered; n is unbounded (the call works in chunks of 2^20).
 */
int b9_predict_mags(b9_ctx *ctx, const double *param_row, int64_t n,
                    const double *mass1, const double *mass_ratio,
                    const int32_t *wd_type /* nullable: all DA */, const int32_t *pop /* nullable: all 0 */,
                    double *out_mags /* [n * n_filt] */, int32_t *out_stage /* nullable, [n] */);

/*
 * Posterior draws of the WD-stage stars on a mass grid of the call's own, with the quantities that follow from the
 * drawn mass (the sampleWDMass counterpart).  Added in ABI 6 without a version change, as b9_predict_mags
 * was: purely additive.  b9_n_wd_stars: the stars of stage B9_STAGE_WD in the loaded catalogue (or a negative b9_status).
 *
 * All pointers are host pointers; synchronous.  Outputs are [n_rows][n_wd], the WD-stage stars in the caller's star
 * order (n_wd = b9_n_wd_stars); any of the five derived outputs (wd_mass, prec_log_age, log_cool_age, log_teff, logg)
 * and out_pop may be NULL.  Needs a loaded pack and loaded stars; honours b9_options.n_pops (1 or 2) and ignores mode,
 * marg_iso_increm and marg_n_q.  B9_ERR_STATE while a sampler block is outstanding; B9_ERR_INVALID for n_nodes < 1;
 * n_wd == 0 is B9_OK with nothing written.  The call uses buffers of its own: a B9_BLOCK_CONTINUE block enqueued after
 * it gives the same bits as one enqueued without it.  Rows are worked in chunks of at most 256 rows, and of as few rows
 * as keep the chunk's node table (n_pops * n_nodes * (2 * padded filters + 6) doubles per row) within 64 MiB -- one row
 * at a time when one row's table is larger than that (B9_ERR_CAPACITY beyond 8 GiB per row); n_rows is otherwise
 * unbounded, and every (row, star) result depends on that row and star alone.
 *
 * Definition.  For row r (global number row = row0 + r), WD-stage star i (its index in the caller's catalogue) and
 * population k:
 *   - nodes j = 1 .. n_nodes, dM = (m_wd_up - agb_tip_k) / n_nodes, m_j = agb_tip_k + dM * j;
 *   - term_j = log_prior_mass(m_j) + sum_f Gaussian log-density(obs_f | wd magnitudes of m_j + mod + (abs_coeff_f - 1) Av)
 *     + log(dM): no companion, the star's own wd_type; a node whose chi-square is not finite does not take part (a node
 *     that rounding puts above m_wd_up has no flux, B9_MAG_NOFLUX, as everywhere in this library);
 *   - drawn node = argmax over (k, j) of term_j [+ log lambda_k] + gumbel(seed, row, i, j, k), the counter coding
 *     b9_sample_mass uses for WD nodes (node = j).  Equal keys: lowest k, then lowest j;
 *   - out_member = p_i L_i / (p_i L_i + (1 - p_i) fieldLike), L_i the log-sum-exp of the terms (two populations: the
 *     lambda mixture), as b9_sample_mass forms it; a star's terms are summed in ascending j, so the value is a function
 *     of the data only;
 *   - at the drawn node: out_zams = m_j; out_wd_mass = ifmr(m_j); out_prec_log_age the precursor log-age;
 *     out_log_cool_age = log10(10^logAge - 10^prec); out_log_teff, out_logg as the WD branch forms them before the
 *     atmosphere lookup -- the values the node's magnitudes were computed FROM, not a second evaluation;
 *   - a node whose precursor has not yet died (prec >= logAge: magnitudes -4.0) can be drawn; it reports zams, wd_mass
 *     and prec_log_age as above and log_cool_age = log_teff = logg = 0.  A pack without WD models (every node
 *     B9_MAG_NOFLUX) and a node above m_wd_up report the five derived values as 0;
 *   - a row outside the grid, dM <= 0, or a star with no live node: every output of that (row, star) is 0.
 * Consequence: for n_nodes = 8 K the drawn ZAMS mass, the population and the membership are the ones b9_sample_mass
 * gives that star at marg_iso_increm = K.
 */
int b9_n_wd_stars(const b9_ctx *ctx);
int b9_sample_wd_mass(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t n_nodes,
                      uint64_t seed, int64_t row0,
                      double *out_zams, double *out_wd_mass, double *out_prec_log_age,
                      double *out_log_cool_age, double *out_log_teff, double *out_logg,
                      double *out_member, int32_t *out_pop /* nullable */);

/*
 * Exact per-star posterior moments over a saved chain (the starSummary counterpart).  Added in ABI 6 without a version
 * change, as b9_predict_mags was: purely additive.  Where b9_sample_mass DRAWS one node per (row, star), this call forms the
 * conditional expectations over all of them and keeps only their sum over the rows: no random numbers, n_stars * B9_MOM_N
 * doubles back instead of 3 per (row, star), and a result that is a deterministic function of the chain.
 *
 * Definition.  The grid is b9_sample_mass's (marg_iso_increm sub-steps per EEP interval x marg_n_q mass ratios; WD-stage
 * stars: 8 * marg_iso_increm steps above the AGB tip, mass ratio 0); n_pops is honoured, mode ignored.  For row r and star
 * i let t_(k,n) = log( prior(M1) dM / n_q * like_i(M1, q) ) [+ log lambda_k] over every node n of population k --
 * b9_sample_mass's key without the Gumbel term; terms that are not finite do not take part --  L = logsumexp t,
 * w = exp(t - L), and p = p_i e^L / (p_i e^L + (1 - p_i) fieldLike) the membership as b9_sample_mass forms it.  The row adds
 *     acc[i][B9_MOM_ROWS]   += 1                  acc[i][B9_MOM_MEMBER] += p
 *     acc[i][B9_MOM_M1]     += p sum w M1         acc[i][B9_MOM_M1SQ]   += p sum w M1^2       (M1: the node's primary ZAMS mass,
 *     acc[i][B9_MOM_Q]      += p sum w q          acc[i][B9_MOM_QSQ]    += p sum w q^2         b9_sample_mass's out_mass)
 *     acc[i][B9_MOM_BINARY] += p sum_{q > 0} w    acc[i][B9_MOM_POP1]   += p sum_{k = 1} w    (0 with one population)
 * A (row, star) for which b9_sample_mass reports all zeros -- a row outside the grid, a star with no live node -- adds
 * nothing, not even to B9_MOM_ROWS.  The sums are weighted by membership: acc[M1] / acc[MEMBER] is E[M1 | data, member]
 * under the chain -- what a membership-weighted average of b9_sample_mass draws estimates.  Terms more than 40 e-folds
 * below a lower bound of the star's largest term may be dropped (b9_tuning.marg_no_pruning: none are): below
 * N_nodes e^-40 of the sums.
 *
 * acc (host, [n_stars][B9_MOM_N], the caller's star order) is in/out: flags = 0 starts from zeros, B9_MOM_CONTINUE from the
 * caller's values (doubles round-trip exactly).  Every accumulator is updated as acc + x_r, one plain add per row in ascending
 * row order: the result is the same bits for any split of the rows over successive continued calls, and for the call's own
 * chunking (at most 32 rows at a time, fewer while the chunk's per-(row, star) scratch would exceed 64 MiB).  A (row, star)
 * increment depends on that row and star alone.  Synchronous; host pointers.  B9_ERR_STATE while a sampler block is
 * outstanding, B9_ERR_INVALID for n_rows < 1 or NULL pointers.  The call uses buffers of its own (isochrones, node tables,
 * scratch, accumulators): a B9_BLOCK_CONTINUE block enqueued after it gives the same bits as one enqueued without it.
 */
enum b9_moment {
    B9_MOM_ROWS = 0, B9_MOM_MEMBER = 1, B9_MOM_M1 = 2, B9_MOM_M1SQ = 3, B9_MOM_Q = 4, B9_MOM_QSQ = 5, B9_MOM_BINARY = 6, B9_MOM_POP1 = 7,
    B9_MOM_N = 8
};
#define B9_MOM_CONTINUE 1
int b9_star_moments(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t flags,
                    double *acc /* host, [n_stars][B9_MOM_N], in/out */);

/*
 * Exact per-WD posterior moments over a saved chain (the wdSummary counterpart).  Added in ABI 6 without a version change, as
 * its siblings were: purely additive.  b9_wd_moments is to b9_sample_wd_mass what b9_star_moments is to b9_sample_mass: where
 * that call DRAWS one node per (row, WD-stage star), this one forms the conditional expectations of the ZAMS mass and of the
 * five derived values over ALL nodes of the call's grid, weights them by membership and keeps only their sum over the rows:
 * no random numbers, n_wd * B9_WDM_N doubles back instead of seven [n_rows][n_wd] arrays.
 *
 * Definition.  Grid, terms and membership are exactly b9_sample_wd_mass's: per population k the n_nodes equal steps
 * m_j = tip_k + dM_k j, j = 1 .. n_nodes, dM_k = (m_wd_up - tip_k) / n_nodes (a population with dM_k <= 0 has no nodes);
 * t_(k,j) = (log prior(m_j) - chi^2 / 2) + log dM_k [+ log lambda_k] through the WD branch with the star's own wd_type at mass
 * ratio 0; terms that are not finite do not take part; L = logsumexp t, w = exp(t - L), p the membership as b9_sample_wd_mass
 * forms it.  n_pops is honoured, mode ignored.  No pruning: every finite term takes part.  A node is COOLED if the WD branch
 * made a white dwarf of it with every derived value set (not: the precursor still alive, a node above m_wd_up or on the tip,
 * a pack without WD models); the node's status travels with the table -- it is not inferred from a value being zero.  Row r
 * adds to WD-stage star i
 *     acc[i][B9_WDM_ROWS]   += 1                     acc[i][B9_WDM_MEMBER] += p
 *     acc[i][B9_WDM_POP1]   += p sum_{k = 1} w       acc[i][B9_WDM_COOLED] += p sum_cooled w
 *     acc[i][B9_WDM_M1]     += p sum w m             acc[i][B9_WDM_M1SQ]   += p sum w m^2          (all nodes)
 *     acc[i][B9_WDM_<V>]    += p sum_cooled w v      acc[i][B9_WDM_<V>_SQ] += p sum_cooled w v^2
 * for v in {wd_mass, precursor log-age, log cooling age, log Teff, log g}: the values the node's magnitudes were computed FROM.
 * A (row, star) for which b9_sample_wd_mass reports all zeros -- a row outside the grid, a row whose AGB tips are not below
 * m_wd_up in any population, a star with no finite term -- adds nothing at all, B9_WDM_ROWS included.
 *
 * acc (host, [n_wd][B9_WDM_N], n_wd = b9_n_wd_stars, the order of b9_sample_wd_mass's columns) is in/out: flags = 0 starts
 * from zeros, B9_WDM_CONTINUE from the caller's values.  Every accumulator is updated as acc + x_r, one plain add per row in
 * ascending row order, and a star's sums take its terms in ascending node order, population by population: the order is a
 * function of the data only.  The result is the same bits for any chunking of the rows inside the call (at most 256 rows,
 * fewer while the chunk's node table -- n_pops * n_nodes * (2 * padded filters + 7) doubles per row -- would exceed 64 MiB,
 * one row at a time above that), for any split of the rows over successive B9_WDM_CONTINUE calls, for any set of other stars
 * in the catalogue, for a repeated call and after any other call on the context.  Synchronous; host pointers.  n_wd == 0 is
 * B9_OK with nothing touched; B9_ERR_INVALID for n_nodes < 1, n_rows < 1 or NULL params / acc; B9_ERR_STATE while a sampler
 * block is outstanding; B9_ERR_CAPACITY when one row's node table would exceed 8 GiB.  The call uses buffers of its own: a
 * B9_BLOCK_CONTINUE block enqueued after it gives the same bits as one enqueued without it.
 */
enum b9_wd_moment {
    B9_WDM_ROWS = 0, B9_WDM_MEMBER = 1, B9_WDM_POP1 = 2, B9_WDM_COOLED = 3,
    B9_WDM_M1 = 4, B9_WDM_M1SQ = 5,
    B9_WDM_WDMASS = 6,  B9_WDM_WDMASS_SQ = 7,   B9_WDM_PREC = 8,     B9_WDM_PREC_SQ = 9,
    B9_WDM_LOGCOOL = 10, B9_WDM_LOGCOOL_SQ = 11, B9_WDM_LOGTEFF = 12, B9_WDM_LOGTEFF_SQ = 13,
    B9_WDM_LOGG = 14,   B9_WDM_LOGG_SQ = 15,    B9_WDM_N = 16
};
#define B9_WDM_CONTINUE 1
int b9_wd_moments(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t n_nodes, int32_t flags,
                  double *acc /* host, [b9_n_wd_stars][B9_WDM_N], in/out */);

/*
 * Exact binned mass posteriors over a saved chain (the massFunction counterpart).  Added in ABI 6 without a version change, as
 * b9_predict_mags and b9_star_moments were: purely additive.  Where b9_star_moments keeps the first two moments of the
 * primary mass per star, this call keeps the DISTRIBUTION: per star summed over the rows (star_hist) and per row summed over
 * the stars (row_hist).
 *
 * Definition.  Grid, terms t_(k,n), L = logsumexp t, w = exp(t - L) and the membership p are exactly b9_star_moments':
 * terms that are not finite do not take part; n_pops is honoured, mode ignored; WD-stage stars use 8 * marg_iso_increm steps
 * above the AGB tip at mass ratio 0; terms more than 40 e-folds below a data-only lower bound of the star's largest term may be
 * dropped (b9_tuning.marg_no_pruning: none are).  A node's value v is, by `quantity`,
 *     B9_HQ_PRIMARY    M1, the node's primary ZAMS mass as b9_sample_mass reports it (MS/RGB: fma(s, dM, a); WD stage: tip + dM j)
 *     B9_HQ_SECONDARY  m2 = ((double)j / (double)n_q) * M1, for the nodes with j > 0 only (WD-stage stars contribute nothing)
 *     B9_HQ_SYSTEM     M1 + m2, every operation rounded on its own (j = 0 and WD-stage stars: M1)
 * edges (host, [n_bins + 1]) must be finite and strictly ascending, 1 <= n_bins <= B9_HIST_MAX_BINS.  Bin b holds
 * e_b <= v < e_(b+1), decided on the value's own bits; a value below e_0, or at or above the last edge, falls in no bin -- but
 * still normalises, since w is taken over ALL nodes: a bin's value does not depend on which other bins were asked for, and
 * calls with disjoint edge sets compose exactly.  Row r adds to star i
 *     x[b] = p sum_{(k,n): v in bin b} w   (b < n_bins),        x[n_bins] = p   (the total column)
 * and nothing at all (every entry 0) where b9_star_moments would add nothing: a row outside the grid, a star with no live node.
 *
 * star_hist (host, [n_stars][n_bins + 1], the caller's star order, in/out, nullable): acc + x_r, one plain add per row in
 * ascending row order; flags = 0 starts from zeros, B9_HIST_CONTINUE from the caller's values.  The same bits for the call's
 * own chunking (at most 32 rows at a time, fewer while the per-(row, star) scratch would exceed 64 MiB) and for any split of the
 * rows over continued calls.  row_hist (host, [n_rows][n_bins + 1], out, nullable): sum_i x_r[i][c] over the caller's star
 * order, ascending, one plain add per star; a row's line depends on that row alone; column n_bins is the expected number of
 * members under that row.  Synchronous; host pointers.  B9_ERR_INVALID (outputs untouched) for bad edges or n_bins, an unknown
 * quantity, n_rows < 1, NULL params or edges, or both outputs NULL; B9_ERR_STATE while a sampler block is outstanding.  The
 * call uses buffers of its own: a B9_BLOCK_CONTINUE block enqueued after it gives the same bits as one enqueued without it.
 */
enum b9_hist_quantity { B9_HQ_PRIMARY = 0, B9_HQ_SECONDARY = 1, B9_HQ_SYSTEM = 2 };
#define B9_HIST_MAX_BINS 64
#define B9_HIST_CONTINUE 1
int b9_mass_hist(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t quantity,
                 const double *edges /* [n_bins + 1] */, int32_t n_bins, int32_t flags,
                 double *star_hist /* host [n_stars][n_bins + 1], in/out, may be NULL */,
                 double *row_hist  /* host [n_rows][n_bins + 1], out,    may be NULL */);

/*
 * Exact mass-ratio posteriors by primary mass over a saved chain (the binaryStats counterpart).  Added in ABI 6 without a version
 * change, as its siblings were: purely additive.  Where b9_star_moments keeps P(q > 0) and two moments of q, and b9_mass_hist bins
 * one mass over the cluster, this call keeps the JOINT table (primary-mass bin x mass-ratio node): which primaries own the
 * companions, at which ratios -- per star summed over the rows (star_cells) and per row summed over the stars (row_cells).
 *
 * Definition.  Grid, terms t_(k,n), L = logsumexp t, w = exp(t - L), the membership p and the pruning are exactly b9_mass_hist's:
 * terms that are not finite do not take part; n_pops is honoured, mode ignored; b9_tuning.marg_no_pruning disables the pruning.
 * Q is the grid's number of mass ratios (marg_n_q; the ratio of node j is (double)j / (double)Q, j = 0 .. Q - 1).  mass_edges
 * (host, [n_mbins + 1]) must be finite and strictly ascending, 1 <= n_mbins <= B9_RH_MAX_MBINS, n_cells = n_mbins * Q <=
 * B9_RH_MAX_CELLS, Q <= 64.  Mass bin b holds e_b <= M1 < e_(b+1) on the value's own bits, M1 being b9_mass_hist's B9_HQ_PRIMARY
 * value (MS/RGB: fma(s, dM, a); WD stage: tip + dM j); a node outside the edges falls in no cell but still normalises.  Row r adds
 * to star i the n_cells + 1 columns
 *     x[b * Q + j] = p sum_{nodes of ratio j with M1 in bin b} w,        x[n_cells] = p   (the total column)
 * WD-stage stars have ratio 0 only: their weight goes to column b * Q.  Every entry is 0 where b9_star_moments would add nothing:
 * a row outside the grid, a star with no live node.
 *
 * Order of a column's sum (b9_mass_hist's): every live term is added to its column one at a time in the wave's walk order, the
 * four waves are merged in wave order, the column is divided by the merged sum of weights, the populations are mixed with the
 * membership's population weights, the result is multiplied by p.  Hence column n_cells is B9_MOM_MEMBER and b9_mass_hist's total
 * bit for bit; with marg_n_q = 1 columns 0 .. n_mbins - 1 are b9_mass_hist(B9_HQ_PRIMARY)'s bit for bit; and a cell's bits do not
 * depend on which other mass bins were asked for.
 *
 * star_cells (host, [n_stars][n_cells + 1], the caller's star order, in/out, nullable): acc + x_r, one plain add per row in
 * ascending row order; flags = 0 starts from zeros, B9_RH_CONTINUE from the caller's values.  row_cells (host,
 * [n_rows][n_cells + 1], out, nullable): sum_i x_r[i][c] over the caller's star order, ascending, one plain add per star.  The
 * same bits for the call's own chunking (at most 32 rows at a time, fewer while the per-(row, star) scratch would exceed 64 MiB),
 * for any split of the rows over continued calls, for any other stars in the catalogue, for a repeated call and after any other
 * call on the context.  Synchronous; host pointers.  B9_ERR_INVALID (outputs untouched; checked on the host before anything is
 * launched) for bad edges, n_mbins outside 1 .. B9_RH_MAX_MBINS, n_mbins * Q > B9_RH_MAX_CELLS, Q > 64, n_rows < 1, NULL params or
 * mass_edges, or both outputs NULL; B9_ERR_STATE while a sampler block is outstanding; B9_ERR_CAPACITY as its siblings.  The call
 * uses buffers of its own: a B9_BLOCK_CONTINUE block enqueued after it gives the same bits as one enqueued without it.
 */
#define B9_RH_MAX_MBINS 16
#define B9_RH_MAX_CELLS 128
#define B9_RH_CONTINUE 1
int b9_ratio_hist(b9_ctx *ctx, const double *params, int32_t n_rows,
                  const double *mass_edges /* [n_mbins + 1] */, int32_t n_mbins, int32_t flags,
                  double *star_cells /* host [n_stars][n_mbins * Q + 1], in/out, may be NULL */,
                  double *row_cells  /* host [n_rows][n_mbins * Q + 1], out,    may be NULL */);

/*
 * Per-star bins over a saved chain (the starIntervals counterpart).  Added in ABI 6 without a version change, as its siblings
 * were: purely additive.  b9_mass_hist bins every star on one shared set of edges; here star i has its OWN strictly ascending
 * finite edges e_i0 < ... < e_iB (1 <= B = n_bins <= B9_SBIN_MAX_BINS), so that a host can narrow each star's bins around its own
 * quantile levels pass by pass (base9_host.h: b9h_refine_star_edges) and end with brackets that provably contain them.
 *
 * Definition.  Grid, terms, L, w = exp(t - L), the membership p, the pruning and the node value v per `quantity` are exactly
 * b9_mass_hist's.  Row r adds to star i
 *     x[0]     = p sum_{v < e_i0} w                 (below)
 *     x[1 + b] = p sum_{e_ib <= v < e_i,b+1} w      (bin b, closed on the left)
 *     x[B + 1] = p sum_{v >= e_iB} w                (at or above)
 *     x[B + 2] = p                                  (the total)
 * Under B9_HQ_SECONDARY the nodes with j = 0 and the WD-stage stars enter no column but the total.  Where b9_star_moments adds
 * nothing (a row outside the grid, a star with no live node) every entry is 0.
 *
 * acc (host, [n_stars][n_bins + 3], the caller's star order, in/out): acc + x_r, one plain add per row in ascending row order;
 * flags = 0 starts from zeros, B9_SBIN_CONTINUE from the caller's values.  The same bits for the call's own chunking (at most
 * 32 rows at a time), for any split of the rows over continued calls, for a repeated call and after any other call on the
 * context.  A star's line depends on that star's edges and data alone.  With the same edges for every star, acc[:, 1 .. B] and
 * acc[:, B + 2] are bit for bit b9_mass_hist's star_hist[:, 0 .. B - 1] and star_hist[:, B]; acc[:, B + 2] is b9_star_moments'
 * B9_MOM_MEMBER.  Synchronous; host pointers.  B9_ERR_INVALID (acc untouched; checked on the host before anything is launched)
 * for n_bins outside 1 .. B9_SBIN_MAX_BINS, an unknown quantity, n_rows < 1, NULL pointers, or any star's edges not finite or
 * not strictly ascending; B9_ERR_STATE while a sampler block is outstanding; B9_ERR_CAPACITY as its siblings.  The call uses
 * buffers of its own: a B9_BLOCK_CONTINUE block enqueued after it gives the same bits as one enqueued without it.
 */
#define B9_SBIN_MAX_BINS 30
#define B9_SBIN_CONTINUE 1
int b9_star_bins(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t quantity,
                 const double *edges /* host [n_stars][n_bins + 1], caller's star order */, int32_t n_bins, int32_t flags,
                 double *acc /* host [n_stars][n_bins + 3], in/out */);

/*
 * Per-WD bins over a saved chain (the wdIntervals counterpart).  Added in ABI 6 without a version change, as its siblings
 * were: purely additive.  b9_wd_bins is to b9_wd_moments what b9_star_bins is to b9_star_moments: where that call keeps a mean
 * and a second moment of a WD-stage star's six quantities, this one bins the node weights of the same grid on every WD's OWN
 * edges, for any subset of the six quantities in one call, so that a host can narrow each line's bins around its own quantile
 * levels (base9_host.h: b9h_refine_star_edges, with n = n_wd * n_sel lines) -- the summary a truncated, stretched or bimodal
 * posterior needs.
 *
 * Definition.  Grid, terms t_(k,j), L = logsumexp t, w = exp(t - L), the membership p, "no pruning" and the COOLED status of a
 * node are exactly b9_wd_moments'.  quantity_mask selects quantities (bit q = enum b9_wd_quantity q); n_sel is the number of its
 * bits and the selected quantities appear in ascending q.  Line (i, s) -- WD-stage star i in the column order of
 * b9_sample_wd_mass, s-th selected quantity -- has its own finite edges e_0 < ... < e_B (1 <= B = n_bins <= B9_WBIN_MAX_BINS).
 * A node's value v is, under B9_WQ_ZAMS, m_j = tip_k + dM_k * (double)j; under the other five the node's derived value (WD mass,
 * precursor log-age, log cooling age, log Teff, log g: the values the node's magnitudes were computed FROM), and there only
 * COOLED nodes count: a node that is not COOLED enters no column but the total.  Row r adds to line (i, s)
 *     x[0]     = p sum_{v < e_0} w                  (below)
 *     x[1 + b] = p sum_{e_b <= v < e_(b+1)} w       (bin b, closed on the left, decided on the value's own bits)
 *     x[B + 1] = p sum_{v >= e_B} w                 (at or above)
 *     x[B + 2] = p                                  (the total)
 * and nothing at all (every entry 0) where b9_wd_moments adds nothing.
 *
 * Order of the sums (a function of the data only): a star's terms enter its population's online log-sum-exp one by one in
 * ascending j, every column rescaled together on a jump of the reference; each column is divided by that population's sum of
 * weights, the populations are mixed with the membership's population weights in population order, then multiplied by p --
 * the sequence b9_wd_moments applies to B9_WDM_COOLED.  Hence a line's total is B9_WDM_MEMBER bit for bit, and with n_bins = 1
 * and edges that enclose every value column 1 of a derived quantity is B9_WDM_COOLED bit for bit.
 *
 * acc (host, [n_wd][n_sel][n_bins + 3], in/out): acc + x_r, one plain add per row in ascending row order; flags = 0 starts from
 * zeros, B9_WBIN_CONTINUE from the caller's values.  The same bits for the call's own chunking (at most 256 rows, fewer while
 * the chunk's node table -- b9_wd_moments' size -- or the per-(row, line) scratch would exceed 64 MiB, down to one row at a
 * time), for any split of the rows over continued calls, for any other stars in the catalogue, any other line's edges, any
 * other quantities in the mask, for a repeated call and after any other call on the context.  Synchronous; host pointers.
 * n_wd == 0 is B9_OK with nothing touched.  B9_ERR_INVALID (acc untouched; checked on the host before anything is launched) for
 * n_bins outside 1 .. B9_WBIN_MAX_BINS, a mask of 0 or with bits at or above B9_WQ_N, n_nodes < 1, n_rows < 1, NULL pointers, or
 * any line's edges not finite or not strictly ascending; B9_ERR_STATE and B9_ERR_CAPACITY as b9_wd_moments.  The call uses
 * buffers of its own: a B9_BLOCK_CONTINUE block enqueued after it gives the same bits as one enqueued without it.
 */
enum b9_wd_quantity { B9_WQ_ZAMS = 0, B9_WQ_WDMASS = 1, B9_WQ_PREC = 2, B9_WQ_LOGCOOL = 3,
                      B9_WQ_LOGTEFF = 4, B9_WQ_LOGG = 5, B9_WQ_N = 6 };
#define B9_WBIN_MAX_BINS 30
#define B9_WBIN_CONTINUE 1
int b9_wd_bins(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t n_nodes, int32_t quantity_mask,
               const double *edges /* host [n_wd][n_sel][n_bins + 1] */, int32_t n_bins, int32_t flags,
               double *acc         /* host [n_wd][n_sel][n_bins + 3], in/out */);

/*
 * Exact per-filter posterior-predictive residuals over a saved chain (the photResiduals counterpart).  Added in ABI 6 without a
 * version change, as b9_star_moments and b9_mass_hist were: purely additive.  Where those calls say what the fit implies for a
 * star's masses, this one says what it implies for the star's MAGNITUDES, filter by filter, and how far the observed ones lie
 * from that: per star summed over the rows (star_resid) and, standardised, per row summed over the stars (row_resid).
 *
 * Definition.  Grid, terms t_(k,n), L = logsumexp t, w = exp(t - L) and the membership p are exactly b9_star_moments':
 * terms that are not finite do not take part; n_pops is honoured, mode ignored; WD-stage stars use 8 * marg_iso_increm steps
 * above the AGB tip at mass ratio 0, through the WD branch with the star's own wd_type; terms more than 40 e-folds below a
 * data-only lower bound of the star's largest term may be dropped (b9_tuning.marg_no_pruning: none are).  pred_f(k,n) is the
 * node's combined apparent magnitude in filter f, the value the likelihood compares with obs_f.  The pivot c_if is obs_if, the
 * caller's bits, where sigma_if > 0, and 0 for an unused filter; d_f = pred_f - c_if, one rounded subtraction.  Row r adds to
 * star i the 2 + 2 n_filt columns
 *     x[0] = 1 (ROWS),  x[1] = p (MEMBER),  x[2 + 2f] = p sum w d_f,  x[3 + 2f] = p sum w d_f^2
 * and nothing at all (every entry 0, ROWS included) where b9_star_moments would add nothing: a row outside the grid, a star
 * with no live node.  An unused filter still gets its two sums about the pivot 0: the magnitude the posterior predicts in a
 * band the star was not observed in.  A star with every filter unused is weighted by the prior over the grid.
 *
 * star_resid (host, [n_stars][2 + 2 n_filt], the caller's star order, in/out, nullable): acc + x_r, one plain add per row in
 * ascending row order; flags = 0 starts from zeros, B9_RESID_CONTINUE from the caller's values.  The same bits for the call's
 * own chunking (at most 32 rows at a time, fewer while the per-(row, star) scratch would exceed 64 MiB) and for any split of the
 * rows over continued calls.  predMag_f = c_f + acc[2 + 2f] / acc[1]; its variance acc[3 + 2f] / acc[1] - (acc[2 + 2f] / acc[1])^2.
 *
 * row_resid (host, [n_rows][1 + 5 n_filt], out, nullable): column 0 is sum_i p_i over all stars.  For filter f, over the stars
 * with sigma_if > 0 only, with s = 1 / sigma_if (one rounded division) and z = (obs - pred) / sigma (observed minus computed):
 *     [1 + 5f] N_f = sum p              [2 + 5f] R_f = sum p E_w[z]   = sum -(x[2 + 2f] s)
 *     [3 + 5f] C_f = sum p E_w[z^2] = sum (x[3 + 2f] s) s             [4 + 5f] W_f = sum (p s) s
 *     [5 + 5f] D_f = sum -((x[2 + 2f] s) s)
 * over the caller's star order, ascending, one plain add per star; a row's line depends on that row alone.  R_f / N_f is the
 * members' mean standardised residual in the band, C_f / N_f its reduced chi^2, D_f / W_f the inverse-variance-weighted
 * zero-point offset in magnitudes.
 *
 * Synchronous; host pointers.  B9_ERR_INVALID (outputs untouched) for n_rows < 1, NULL params or both outputs NULL;
 * B9_ERR_STATE while a sampler block is outstanding; B9_ERR_CAPACITY as its siblings.  The call uses buffers of its own: a
 * B9_BLOCK_CONTINUE block enqueued after it gives the same bits as one enqueued without it.
 */
#define B9_RESID_CONTINUE 1
int b9_phot_resid(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t flags,
                  double *star_resid /* host [n_stars][2 + 2 n_filt], in/out, may be NULL */,
                  double *row_resid  /* host [n_rows][1 + 5 n_filt], out,    may be NULL */);

/*
 * Exact leave-one-filter-out predictions over a saved chain (the filterCheck counterpart).  Added in ABI 6 without a version
 * change, as its siblings were: purely additive.  b9_phot_resid's residuals are in-sample -- the band being judged helped choose
 * the node weights --; this call gives, for every filter, the magnitude the star's OTHER filters predict and the density of the
 * observed value under that prediction, from one walk of the node table.
 *
 * Definition.  The grid, the terms t_(k,n), the finite-term rule, L = logsumexp t, the membership p and the WD-stage steps are
 * exactly b9_star_moments'; p is the FULL-DATA membership (no leave-out has one of its own).  For a filter f the star uses
 * (sigma_if > 0) let g_f(n) = ((pred_f(n) - obs_if) / sigma_if)^2 / 2, the node's share of its own chi^2, formed from the same
 * scaled pair as the node's chi^2; for an unused filter g_f = 0.  Leave-out f has the terms t^f = t + g_f over the same node
 * set, L^f = logsumexp t^f -- the populations mixed by that leave-out's own weights e^(log lambda_k + lg^f_k) / sum -- and the
 * weights w^f = exp(t^f - L^f).  With d_f = pred_f - c_if (b9_phot_resid's pivot, one rounded subtraction) row r adds to star i
 * the 2 + 3 n_filt columns
 *     x[0] = 1 (ROWS),  x[1] = p (MEMBER),  x[2 + 3f] = p sum w^f d_f,  x[3 + 3f] = p sum w^f d_f^2,  x[4 + 3f] = p l_f
 * with l_f = (L - L^f) - log(sigma_if sqrt(2 pi)) = log p(obs_f | the other filters, row, member); l_f = 0 exactly for an unused
 * filter, whose two sums are then the in-sample ones.  Where b9_star_moments adds nothing this call adds nothing either, ROWS
 * included.
 *
 * Pruning.  A node may be left out of leave-out f's sums only when t^f lies more than 40 e-folds below a data-only lower bound
 * of max t^f: the star's seed (a valid bound because t^f >= t), then that leave-out's own running maximum.  A chunk's or unit's
 * box is skipped only when every leave-out may skip it (the box's chi^2 bound less its largest per-filter part) and the
 * full-data sum may.  What is dropped is below N_nodes e^-40 of that sum's weight; b9_tuning.marg_no_pruning: nothing is.
 * x[0] and x[1] are b9_phot_resid's bits.
 *
 * star_loo (host, [n_stars][2 + 3 n_filt], the caller's star order, in/out, nullable): acc + x_r, one plain add per row in
 * ascending row order; flags = 0 starts from zeros, B9_LOO_CONTINUE from the caller's values.  looMag_f = c_f + acc[2 + 3f] /
 * acc[1], its between-node variance acc[3 + 3f] / acc[1] - (acc[2 + 3f] / acc[1])^2, the mean log predictive density
 * acc[4 + 3f] / acc[1].
 *
 * row_loo (host, [n_rows][1 + 6 n_filt], out, nullable): column 0 is sum_i p_i over all stars.  For filter f, over the stars
 * with sigma_if > 0 only, in the caller's ascending star order, one plain add each: N_f, R_f, C_f, W_f, D_f by b9_phot_resid's
 * five formulas on the leave-out sums at [1 + 6f .. 5 + 6f], and E_f = sum x[4 + 3f] at [6 + 6f].
 *
 * The same bits for the call's own chunking (at most 32 rows at a time, fewer while the per-(row, star) scratch would exceed
 * 64 MiB), any split of the rows over continued calls, a repeated call, any history of the context, any other stars in the
 * catalogue, and either output being NULL.  Synchronous; host pointers.  B9_ERR_INVALID (outputs untouched) for n_rows < 1, NULL
 * params or both outputs NULL; B9_ERR_STATE while a sampler block is outstanding; B9_ERR_CAPACITY as its siblings.  The call
 * uses buffers of its own: a B9_BLOCK_CONTINUE block enqueued after it gives the same bits as one enqueued without it.
 */
#define B9_LOO_CONTINUE 1
int b9_filter_loo(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t flags,
                  double *star_loo /* host [n_stars][2 + 3 n_filt], in/out, may be NULL */,
                  double *row_loo  /* host [n_rows][1 + 6 n_filt], out,    may be NULL */);

/*
 * Exact per-star reddening and distance offsets over a saved chain (the starOffsets counterpart).  Added in ABI 6 without a
 * version change, as its siblings were: purely additive.  Every other saved-chain call assumes one extinction and one distance
 * modulus for every member; this call asks, star by star, how far the star lies off the cluster's values along up to
 * B9_OFF_MAX_DIRECTIONS fixed directions in magnitude space, and how strongly the data want that freedom.
 *
 * Definition.  The grid, the terms t_(k,n), the finite-term rule, L = logsumexp t, the FULL-DATA membership p and the WD-stage
 * steps are exactly b9_star_moments'.  Direction j is a vector k[j][f] over the pack's filters and a prior width tau[j] > 0, both
 * in mag: the star's predicted magnitudes are pred_f + delta k_f with delta ~ N(0, tau^2).  Predicted magnitudes are linear in
 * the modulus (k_f = 1) and in A_V (k_f = the pack's absorption coefficients), so those two offsets are exact.  For star i let
 * c_f = k_f / sigma_if for the filters it uses (sigma_if > 0), else 0;  C = sum_f c_f^2 (f ascending);  V = 1 / (C + tau^-2).  For a
 * node with dd_f = fma(sw_f, pred_f, -so_f), the scaled pair its chi^2 is formed from:  B~ = -sum_f c_f dd_f (one fma chain, f
 * ascending),  mu = V B~ (the node-conditional posterior mean of delta),  g = V B~^2 / 2,  t' = t + g: delta integrated out of
 * the node analytically.  In the WD stage the same from d_f = pred_f - obs_f and wgt_f:  B = -sum k_f (wgt_f d_f),  C = sum k_f^2
 * wgt_f.  L' = logsumexp t' -- the populations mixed by that direction's own weights --, w' = exp(t' - L').  Row r adds to star i
 * the 2 + 3 n_dir columns
 *     x[0] = 1 (ROWS),  x[1] = p (MEMBER),  x[2 + 3j] = p sum w' mu,  x[3 + 3j] = p sum w' mu^2,
 *     x[4 + 3j] = p ((L' - L) - log1p(C tau^2) / 2)
 * the last being p times the log Bayes factor of "this star has an offset of its own" against "it has none", Occam term
 * included.  A star with C = 0 for a direction has exact zeros in that direction's three columns.  Where b9_star_moments adds
 * nothing this call adds nothing either, ROWS included.  A direction's columns do not depend on which other directions are in
 * the call.
 *
 * Pruning.  A node may be left out of direction j's sums only when t' lies more than 40 e-folds below a data-only lower bound
 * of max t': the star's seed (valid because t' >= t), then that direction's own running maximum.  A chunk's or unit's box is
 * skipped only when the full-data sum may skip it and every direction may: X - 2 g >= (1 - C V) lb + nbmin (Cauchy-Schwarz).  What
 * is dropped is below N_nodes e^-40 of that sum's weight; b9_tuning.marg_no_pruning: nothing is.  x[0] and x[1] are
 * b9_phot_resid's bits.
 *
 * star_off (host, [n_stars][2 + 3 n_dir], the caller's star order, in/out, nullable): acc + x_r, one plain add per row in
 * ascending row order; flags = 0 starts from zeros, B9_OFF_CONTINUE from the caller's values.  E[delta] = acc[2 + 3j] / acc[1],
 * Var[delta] = acc[3 + 3j] / acc[1] - E[delta]^2 + V, the mean log Bayes factor acc[4 + 3j] / acc[1].
 *
 * row_off (host, [n_rows][1 + 4 n_dir], out, nullable): column 0 is sum_i p_i over all stars.  For direction j, over the stars
 * with C > 0 only, in the caller's ascending star order, one plain add each:  N = sum p,  M1 = sum x[2 + 3j],
 * M2 = sum (x[3 + 3j] + p V_i),  E = sum x[4 + 3j]  at [1 + 4j .. 4 + 4j]  (V_i = 1 / (sum_f (k_f / sigma_if)^2 + tau^-2)).
 *
 * The same bits for the call's own chunking (at most 32 rows at a time, fewer while the per-(row, star) scratch would exceed
 * 64 MiB), any split of the rows over continued calls, a repeated call, any history of the context, any other stars in the
 * catalogue, and either output being NULL.  Synchronous; host pointers.  B9_ERR_INVALID (outputs untouched) for n_rows < 1, NULL
 * params, k or tau, both outputs NULL, n_dir outside 1 .. B9_OFF_MAX_DIRECTIONS, a tau that is not positive and finite or a k
 * that is not finite; B9_ERR_STATE while a sampler block is outstanding; B9_ERR_CAPACITY as its siblings.  The call uses buffers
 * of its own: a B9_BLOCK_CONTINUE block enqueued after it gives the same bits as one enqueued without it.
 */
#define B9_OFF_CONTINUE 1
#define B9_OFF_MAX_DIRECTIONS 4
int b9_star_offset(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t flags, int32_t n_dir,
                   const double *k   /* host [n_dir][n_filt], mag per unit offset */,
                   const double *tau /* host [n_dir], mag, > 0 */,
                   double *star_off  /* host [n_stars][2 + 3 n_dir], in/out, may be NULL */,
                   double *row_off   /* host [n_rows][1 + 4 n_dir], out,    may be NULL */);

/*
 * Exact pointwise predictive densities over a saved chain (the modelScore counterpart): what WAIC, PSIS-LOO and the paired
 * comparison of two fits need.  Added in ABI 6 without a version change, as its siblings were: purely additive.
 *
 * Definition.  Grid, terms and pruning are exactly b9_star_moments': marg_iso_increm x marg_n_q nodes per EEP interval; WD-stage
 * stars 8 * marg_iso_increm steps above the AGB tip at mass ratio 0; n_pops honoured, mode ignored; terms that are not finite do
 * not take part; terms more than 40 e-folds below a data-only lower bound may be dropped (b9_tuning.marg_no_pruning: none are).
 * The value of (row r, star i) is v = logaddexp(la_i, l) with l the lambda-mixed c0m_i + logsumexp(t) and la_i = log(1 - p_i) +
 * log fs: the per-star value b9_logpost reports in marginalised mode.  A star with no live node under a row has v = la_i, the
 * field term (-inf at membership prior 1), and -- unlike b9_star_moments -- that (row, star) COUNTS.  A row outside the grid
 * contributes nothing to any star.
 *
 * acc (host, [n_stars][B9_PW_N], the caller's star order, in/out, nullable): updated one row at a time in ascending row order;
 * with k = the finite rows the star has taken so far and the row's value v:
 *     B9_PW_ROWS + 1 for every row inside the grid;  B9_PW_NINF + 1 if v = -inf, and such a row touches nothing else;
 *     k = 0:  (VMAX, SPOS, RMAX, SNEG, MEAN, M2) = (v, 1, -v, 1, v, 0);
 *     k > 0:  v > VMAX ? (SPOS = fma(SPOS, exp(VMAX - v), 1), VMAX = v) : SPOS += exp(v - VMAX);  the same rule on
 *             (RMAX, SNEG) with r = -v;  d = v - MEAN, MEAN += d / (k + 1), M2 = fma(d, v - MEAN, M2)      (Welford).
 * One exp; contractions only where written.  The state is carried whole, so the bits are the same for the call's own chunking
 * (at most 32 rows at a time) and for any split of the rows over B9_PW_CONTINUE calls; flags = 0 starts from zeros.  A star is
 * empty when ROWS - NINF = 0.  lppd_i = VMAX + log SPOS - log ROWS;  the variance of v is M2 / (ROWS - NINF - 1).
 *
 * tail (host, [n_stars][tail_len], in/out, nullable, 0 <= tail_len <= B9_PW_MAX_TAIL; requires acc): the tail_len largest values
 * of r = -v among the star's finite rows, descending, padded with -inf: a function of the multiset of values only, so identical
 * for any row order, chunking or split.  flags = 0 starts from -inf.
 *
 * row_lpd (host, [n_rows], out, nullable): sum_i v_ri over the caller's star order, ascending, one plain add per star; -inf for
 * a row outside the grid; a row's value depends on that row alone.
 *
 * Synchronous; host pointers.  B9_ERR_INVALID (outputs untouched) for n_rows < 1, NULL params, both acc and row_lpd NULL,
 * tail_len outside [0, B9_PW_MAX_TAIL] or tail without acc; B9_ERR_STATE while a sampler block is outstanding; B9_ERR_CAPACITY as
 * its siblings.  The call uses buffers of its own: a B9_BLOCK_CONTINUE block enqueued after it gives the same bits as one
 * enqueued without it.
 */
#define B9_PW_ROWS 0
#define B9_PW_NINF 1
#define B9_PW_VMAX 2
#define B9_PW_SPOS 3
#define B9_PW_RMAX 4
#define B9_PW_SNEG 5
#define B9_PW_MEAN 6
#define B9_PW_M2 7
#define B9_PW_N 8
#define B9_PW_MAX_TAIL 256
#define B9_PW_CONTINUE 1
int b9_pointwise(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t flags, int32_t tail_len,
                 double *acc     /* host [n_stars][B9_PW_N],   in/out, may be NULL */,
                 double *tail    /* host [n_stars][tail_len],  in/out, may be NULL */,
                 double *row_lpd /* host [n_rows],             out,    may be NULL */);

/*
 * Star influence over a saved chain (the starInfluence counterpart): which stars and which groups of stars drive the cluster
 * parameters.  Added in ABI 6 without a version change, as its siblings were: purely additive.  Stars are independent given the
 * cluster parameters, so the posterior without star i is the chain reweighted by exp(-v_ri), and the posterior without a group G
 * of stars is the chain reweighted by exp(-sum_{i in G} v_ri): the call reduces both on the device.
 *
 * Definition.  The grid, the terms, the pruning (b9_tuning.marg_no_pruning), the treatment of n_pops / mode and the value
 * v = logaddexp(la_i, l) of (row r, star i) are exactly b9_pointwise's.  A row outside the grid touches no star.  q (host,
 * [n_rows][n_q], 1 <= n_q <= B9_INF_MAX_Q, finite) holds the caller's own per-row scalars; the library gives them no meaning.
 *
 * acc (host, [n_stars][B9_INF_N(n_q)], the caller's star order, in/out, nullable): updated one row at a time in ascending row
 * order; with k = ROWS - NINF before the row, the row's value v and r = -v:
 *     ROWS + 1 for every row inside the grid;  NINF + 1 if v = -inf, and such a row touches nothing else;
 *     k = 0:  RMAX = r, SNEG = 1, SNEG2 = 1, MEANV = v;  per j: WQ = q_j, WQ2 = q_j q_j, MQ = q_j, CVQ = 0;
 *     k > 0, r > RMAX, f = exp(RMAX - r), ff = f f:  SNEG = fma(SNEG, f, 1), SNEG2 = fma(SNEG2, ff, 1), WQ_j = fma(WQ_j, f, q_j),
 *             WQ2_j = fma(WQ2_j, f, q_j q_j), RMAX = r;
 *     k > 0 otherwise, e = exp(r - RMAX):  SNEG = SNEG + e, SNEG2 = fma(e, e, SNEG2), WQ_j = fma(e, q_j, WQ_j),
 *             WQ2_j = fma(e q_j, q_j, WQ2_j);
 *     k > 0, after either:  dv = v - MEANV, MEANV += dv / (k + 1);  per j: dq = q_j - MQ_j, MQ_j += dq / (k + 1),
 *             CVQ_j = fma(dv, q_j - MQ_j, CVQ_j) with the new MQ_j                                           (Welford).
 * One exp; contractions only where written.  (ROWS, NINF, RMAX, SNEG) are b9_pointwise's words, bit for bit.  The state is
 * carried whole, so the bits are the same for the call's own chunking (b9_pointwise's: at most 32 rows, the same 16 MiB rule) and
 * for any split of the rows over B9_INF_CONTINUE calls; flags = 0 starts from zeros.  A quantity's four columns depend on that
 * quantity alone: not on n_q, its position or the other quantities.  SNEG^2 / SNEG2 is the effective sample size of the chain
 * without star i; WQ / SNEG the mean of q_j without it; -CVQ / (ROWS - NINF - 1) the first-order move of that mean.
 *
 * tail / tail_len: exactly b9_pointwise's (the tail_len largest -v per star, descending, padded with -inf; requires acc).
 *
 * group_lpd (host, [n_rows][n_groups], out, nullable; 1 <= n_groups <= B9_INF_MAX_GROUPS): group (host, [n_stars]) gives every
 * star's group, -1 for none.  group_lpd[r][g] = sum of v_ri over the stars with group[i] == g, in ascending caller order from
 * +0.0, one plain add per star; -inf propagates; an empty group inside the grid gives 0.0; a row outside the grid gives -inf for
 * every group.  A row's sums depend on that row alone and a group's sums do not depend on the other groups.  An empty catalogue
 * gives all-zero group_lpd.
 *
 * Synchronous; host pointers.  B9_ERR_INVALID (every output untouched) for NULL ctx or params, n_rows < 1, both acc and
 * group_lpd NULL, acc with n_q outside 1 .. B9_INF_MAX_Q or NULL q, a q that is not finite, tail_len outside
 * [0, B9_PW_MAX_TAIL], tail without acc, group_lpd with n_groups outside 1 .. B9_INF_MAX_GROUPS, NULL group or an id outside
 * -1 .. n_groups - 1; B9_ERR_STATE while a sampler block is outstanding; B9_ERR_CAPACITY as its siblings.  The call uses buffers
 * of its own: a B9_BLOCK_CONTINUE block enqueued after it gives the same bits as one enqueued without it.
 */
#define B9_INF_ROWS 0
#define B9_INF_NINF 1
#define B9_INF_RMAX 2
#define B9_INF_SNEG 3
#define B9_INF_SNEG2 4
#define B9_INF_MEANV 5
#define B9_INF_HEAD 6
#define B9_INF_WQ(j)  (6 + 4 * (j))      /* then WQ2, MQ, CVQ at +1, +2, +3 */
#define B9_INF_N(Q)   (6 + 4 * (Q))
#define B9_INF_MAX_Q 12
#define B9_INF_MAX_GROUPS 8
#define B9_INF_CONTINUE 1
int b9_star_influence(b9_ctx *ctx, const double *params, int32_t n_rows, int32_t flags,
                      int32_t n_q, const double *q   /* host [n_rows][n_q] */,
                      double *acc                    /* host [n_stars][B9_INF_N(n_q)], in/out, may be NULL */,
                      int32_t tail_len, double *tail /* host [n_stars][tail_len], in/out, may be NULL */,
                      int32_t n_groups, const int32_t *group /* host [n_stars], -1 or 0 .. n_groups-1 */,
                      double *group_lpd              /* host [n_rows][n_groups], out, may be NULL */);

/*
 * Isochrone and WD-sequence bands over a saved chain (the cmdBand counterpart): the model locus the posterior implies in the
 * CMD, with what a credible band needs.  Added in ABI 6 without a version change, as its siblings were: purely additive.  Needs a
 * loaded pack and no stars, like b9_predict_mags; honours b9_options.n_pops and ignores everything else in the options.
 *
 * Lines.  Each population k has P = n_ratio n_eep + n_types n_wd_nodes points: MS/RGB point (s, e) at p = s n_eep + (e - eep0),
 * WD point (t, j) at p = n_ratio n_eep + t n_wd_nodes + (j - 1), t counting the set bits of wd_types in ascending order,
 * j = 1 .. n_wd_nodes.  Each point has C = 1 + n_filt + n_colour columns: its ZAMS mass, one apparent magnitude per filter, the
 * colours.  Line (k P + p) C + c; n_lines = n_pops P C.
 *
 * Values.  MS/RGB point (k, s, e) exists in row r when b9_derive_isochrone(row, k) reports n > 0 and first <= e < first + n.  Its
 * mass and primary magnitudes are that isochrone's point, the same bits; for q_s > 0 the secondary is the MS/RGB rule at q_s m_e
 * on the same isochrone (below the first mass: no flux), combined by b9_predict_mags' expression under its rule that a filter in
 * which neither component gives flux stays B9_MAG_NOFLUX; the apparent magnitude is x + (mod + (A_f / A_V - 1) A_V).  WD point
 * (k, t, j) exists when population k is inside the grid, dM_k = (M_wd_up - tip_k) / n_wd_nodes > 0 and the node is COOLED
 * (b9_wd_moments); its mass is tip_k + dM_k (double)j and its magnitudes are b9_wd_moments' node table's for type t.  A magnitude
 * column enters only when its value is finite and not B9_MAG_NOFLUX; a colour only when both its filters enter, as one rounded
 * subtraction of the two apparent magnitudes; a point that does not exist adds nothing to any column.
 *
 * Increments.  With v the value and d = v - pivot[line] (one rounded subtraction; pivot NULL: 0), row r updates mom[line] by
 * N += 1, SUM += d, SUMSQ += d d, MIN = fmin(MIN, v), MAX = fmax(MAX, v), each one plain IEEE operation, rows ascending; and adds
 * 1.0 to one word of bins[line] on the line's own finite edges e_0 < ... < e_B (B = n_bins): [0] below, [1 + b] e_b <= v < e_(b+1)
 * decided on the value's bits, [B + 1] at or above, and 1.0 to [B + 2], the total -- b9_star_bins' layout, so
 * b9h_refine_star_edges serves the lines with n_stars = n_lines.  flags = 0 starts from N = SUM = SUMSQ = 0, MIN = +inf,
 * MAX = -inf and zero bins, B9_BAND_CONTINUE from the caller's arrays.  Either of mom and bins may be NULL, not both; edges and
 * n_bins matter only with bins.
 *
 * The same bits for the call's own chunking (at most 256 rows, fewer while the chunk's value table or its WD node table would
 * exceed 64 MiB, down to one row at a time; beyond 8 GiB per row, or for the lines' pivots, moments, bins and edges together,
 * B9_ERR_CAPACITY), for any split of the rows over continued
 * calls, a repeated call, any history of the context and any other lines in the spec.  Synchronous; host pointers.
 * B9_ERR_INVALID (outputs untouched; checked on the host before anything is launched) for n_rows < 1, NULL params or spec, both
 * outputs NULL, no lines, n_eep < 0, n_ratio outside 0 .. B9_BAND_MAX_RATIOS, a ratio outside [0, 1] or not finite, n_eep > 0
 * with n_ratio = 0, n_wd_nodes < 0, n_wd_nodes > 0 with wd_types outside 1 .. 3, n_colour outside 0 .. B9_BAND_MAX_COLOURS, a
 * colour with a filter out of range or f1 == f2, bins without edges, n_bins outside 1 .. B9_BAND_MAX_BINS, any line's edges not
 * finite or not strictly ascending.  B9_ERR_STATE without a pack or while a sampler block is outstanding.  The call uses a
 * buffer of its own: a B9_BLOCK_CONTINUE block enqueued after it gives the same bits as one enqueued without it.
 */
#define B9_BAND_MAX_RATIOS 4
#define B9_BAND_MAX_COLOURS 8
#define B9_BAND_MAX_BINS 30
#define B9_BAND_CONTINUE 1
enum { B9_BAND_N = 0, B9_BAND_SUM = 1, B9_BAND_SUMSQ = 2, B9_BAND_MIN = 3, B9_BAND_MAX = 4, B9_BAND_NMOM = 5 };
typedef struct b9_band_spec {
    int32_t eep0, n_eep;        /* MS/RGB points: EEP ids eep0 .. eep0 + n_eep - 1 (n_eep may be 0)   */
    int32_t n_ratio;            /* 0 .. B9_BAND_MAX_RATIOS loci: mass ratio q_s in [0, 1], 0 = single */
    const double *ratio;        /* [n_ratio]                                                          */
    int32_t n_wd_nodes;         /* WD points per atmosphere type (0: none)                            */
    int32_t wd_types;           /* bit 0 DA, bit 1 DB                                                 */
    int32_t n_colour;           /* 0 .. B9_BAND_MAX_COLOURS                                           */
    const int32_t *colour;      /* [n_colour][2]: filters f1 != f2, column = app_f1 - app_f2          */
} b9_band_spec;
int b9_cmd_band(b9_ctx *ctx, const double *params, int32_t n_rows, const b9_band_spec *spec, int32_t flags,
                const double *pivot /* [n_lines], nullable: 0 */, double *mom /* [n_lines][5], in/out, nullable */,
                const double *edges /* [n_lines][n_bins + 1] */, int32_t n_bins, double *bins /* [n_lines][n_bins + 3], in/out, nullable */);

/* ---- introspection (used by bench/tests; no compute) --------------------------------- */
int b9_max_eep(const b9_ctx *ctx);           /* longest isochrone in the loaded pack        */
int b9_device_id(const b9_ctx *ctx);
/* Algorithmic bytes one star-eval moves in the loaded layout ("bytes per unit"). */
int b9_bytes_per_star_eval(const b9_ctx *ctx);
/* Star tiles per hot workgroup the fused sampler step would use for n_walkers local walkers with the loaded pack, stars
 * and tuning (> 0), or a negative b9_status.  The summation grouping of a walker's log-posterior follows from it (see
 * b9_tuning.tiles_per_block). */
int b9_step_tiles_per_block(b9_ctx *ctx, int32_t n_walkers);
/* Metropolis steps one launch of a given-mass sampler block advances n_walkers local chains by (b9_tuning.tree_depth). */
int b9_step_depth(b9_ctx *ctx, int32_t n_walkers);
/* Elapsed ms of the dominant (star-likelihood) kernel over the TIMED launches since the last
 * call with reset != 0, measured with HIP events on the launch stream; *n_launches receives
 * their count.  b9_enable_timing(ctx, n): n = 0 off, n > 0 opens an event bracket at every n-th
 * launch.  In the sampler's fused step a bracket spans 8 consecutive launches of the kernel (never
 * past the block's end; B9_TIMING_GROUP), so that the two event records cost an eighth of what a
 * bracket around a single launch adds (~2-3 us): total_ms / n_launches is the kernel's launch period. */
int b9_enable_timing(b9_ctx *ctx, int on);
int b9_kernel_time_ms(b9_ctx *ctx, int reset, double *total_ms, int32_t *n_launches);
/* Mean elapsed ms of the same event bracket around an EMPTY kernel: what the bracket adds to a
 * kernel's own duration (one dispatch boundary + event processing).  Reported, never applied. */
int b9_calibrate_timing(b9_ctx *ctx, double *bracket_overhead_ms);
/* Shader clock observed over a stretch of the context's stream (ABI 5).  b9_clock_stamp(ctx, 0) / (ctx, 1) enqueue a small
 * kernel that records, per compute unit, the shader-cycle counter (s_memtime) and the 100 MHz reference counter
 * (s_memrealtime); b9_clock_mhz waits for the stream and returns delta(shader cycles) / delta(reference) x 100 MHz between
 * the two stamps: the median over the compute units both stamps reached (differences are formed per CU: the cycle counters
 * of different CUs are offset against each other) and, when the pointers are not NULL, the extremes and the length of the
 * stretch in seconds of the reference clock.  What a roofline's clock-dependent peak should be read against. */
int b9_clock_stamp(b9_ctx *ctx, int32_t which);
int b9_clock_mhz(b9_ctx *ctx, double *mhz, double *mhz_min, double *mhz_max, double *ref_seconds);

#ifdef __cplusplus
}
#endif
#endif /* BASE9_HIP_H */
