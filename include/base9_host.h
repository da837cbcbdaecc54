/*
 * base9_host.h -- C surface of libbase9host.so: the C++ host side above the hot path's C ABI (base9_hip.h) --
 * the walker-parallel adaptive-Metropolis driver and its RCCL exchange (SURVEY.md section 8 rows e, f-1) plus the
 * file parsers (rows f-2, f-3) -- for callers that are not C++ (bench.py and the tests bind it with ctypes; a
 * reference-side binding would use the C++ classes in base_amd/host/ directly).
 *
 * The reference has no counterpart of the multi-GPU part: it runs one adaptive chain on CPU threads [RECALL]; walkers,
 * their sharding over GPUs and the RCCL all-gather are constructs of BASELINE.json's north_star.
 *
 * Every function returns 0 on success and -1 on failure (b9h_last_error() gives the text) unless stated otherwise.
 * Nothing here evaluates a likelihood: every number comes from libbase9hip.so on the GPU, or -- in the callback
 * variants, a seam for testing this library's own logic on a machine without a GPU -- from the caller.
 */
#ifndef BASE9_HOST_H
#define BASE9_HOST_H

#include "base9_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *b9h_last_error(void);

/* ---- ranks --------------------------------------------------------------------------------------------------- */
/* RANK / WORLD_SIZE / LOCAL_RANK of this process as the launchers export them (B9_RANK ... first); 0 / 1 / 0 if absent */
void b9h_rank_from_env(int *rank, int *world, int *local_rank);
int b9h_device_synchronize(void);                       /* hipDeviceSynchronize of the current device */

/* ---- exchange of block summary rows between ranks --------------------------------------------------------------- */
typedef int (*b9h_gather_fn)(void *user, const double *mine, size_t count, double *all);
int b9h_exchange_local(void **out);                     /* one rank */
/* RCCL over xGMI, one process per GPU; dir NULL = the launch's default bootstrap directory (b9dist.hpp) */
int b9h_exchange_rccl(int rank, int world, const char *dir, int device, void **out);
int b9h_exchange_callback(b9h_gather_fn gather, void *user, int rank, int world, void **out);   /* tests */
void b9h_exchange_free(void *exchange);
int b9h_exchange_barrier(void *exchange);
int b9h_exchange_max(void *exchange, double value, double *max_over_ranks);
int b9h_exchange_world(void *exchange);                 /* returns the number of ranks */
const char *b9h_exchange_name(void *exchange);
/* What the communicator itself reports: its rank count (ncclCommCount; 0 for an exchange without a communicator) ...  */
int b9h_exchange_comm_ranks(void *exchange);
/* ... and the PCI bus ids of the ranks' GPUs in rank order, comma-separated, all-gathered through the communicator
 * ("" without one).  Returns 0, or -1 when `cap` is too small. */
int b9h_exchange_devices(void *exchange, char *out, int cap);
/* 0 when a communicator of `comm_ranks` ranks on the GPUs `devices_csv` (as b9h_exchange_devices returns them) is what a launch
 * of `world` ranks must have -- that many ranks on that many DISTINCT devices -- else 1 with the reason in msg[cap].  The RCCL
 * exchange refuses such a group itself (b9h_exchange_rccl fails); launchers check their own report with it. */
int b9h_group_check(int world, int comm_ranks, const char *devices_csv, char *msg, int cap);
/* 1 when this process is a rank of a --forceRanks / --force-ranks launch (B9_FORCE_RANKS): one GPU, full multi-rank route */
int b9h_forced_ranks(void);
/* Test hook of the launchers' deadlines: parks the calling rank for ever when B9_TEST_STALL == "<where>:<rank>". */
void b9h_test_stall(const char *where, int rank);

/* ---- the sampler ------------------------------------------------------------------------------------------------ */
typedef int (*b9h_block_fn)(void *user, const double *params_in, const double *logpost_in, const int32_t *walker_ids, int n_local,
                            const int32_t *free_idx, int d, const double *chol, uint64_t seed, int64_t step0, int n_steps,
                            double *params_out, double *logpost_out, double *samples, double *lps, int64_t *n_accept);
typedef int (*b9h_logpost_fn)(void *user, const double *params, int n, double *out);
/* n_walkers: all ranks together; free_idx / step: [d]; mode: the B9_MODE_* of the context's options */
int b9h_sampler_create(b9_ctx *ctx, int mode, int n_walkers, const int32_t *free_idx, const double *step, int d,
                       uint64_t seed, int block, void *exchange, void **out);
int b9h_sampler_create_callback(b9h_block_fn run, b9h_logpost_fn eval, void *user, int n_walkers, const int32_t *free_idx,
                                const double *step, int d, uint64_t seed, int block, void *exchange, void **out);   /* tests */
void b9h_sampler_free(void *sampler);
int b9h_sampler_initialise(void *sampler, const double *start /* [n_walkers][B9_NPARAM], the same on every rank */);
/* n_steps in blocks; adapt = 0 freezes the proposal.  samples [n_steps][n_local][d] / lps [n_steps][n_local]: nullable */
int b9h_sampler_run(void *sampler, int64_t n_steps, int adapt, double *samples, double *lps);
int b9h_sampler_n_local(void *sampler);                 /* returns the number of local walkers */
/* any output may be NULL; chol [d*d]; all_params [n_walkers][B9_NPARAM] / all_logpost [n_walkers] as of the last exchange */
int b9h_sampler_state(void *sampler, int64_t *steps, int64_t *accepted_local, double *scale, double *chol,
                      double *all_params, double *all_logpost);
/* the host statement of the device's block summary rows (b9_mcmc_block::rows) */
int b9h_summary_rows(const double *samples, const double *params_end, const double *logpost_end, int n_steps, int n_local, int d,
                     const double *origin, double *rows);

/* ---- file parsers (docs/FORMATS.md) ---------------------------------------------------------------------------------- */
int b9h_load_pack(const char *dir, const char *ms_model, const char *wd_model, const char *filters_csv, void **handle, b9_pack *view);
void b9h_free_pack(void *handle);
int b9h_read_phot(const char *path, double min_mag, double max_mag, int index, void **handle, b9_stars *view,
                  char *filters_out, int filters_cap);
void b9h_free_phot(void *handle);
int b9h_settings_dump(int argc, char **argv, char *out, int cap);
/* ---- simCluster / scatterCluster draws (docs/FORMATS.md "Simulation draws"; libbase9host's one definition of them) -------- */
/* Counter-based Philox4x32-10, key = (seed lo, seed hi), counter = (i lo, i hi, purpose, j): every value of system i is a
 * function of (seed, i, settings) alone.  Systems i0 .. i0+n-1: primary mass (purpose 0), mass ratio (1; 0 above tip[pop]),
 * DB atmosphere (2), population (3; n_pops == 2: 1 when u >= lambda).  tip: [2] AGB-tip masses of the populations'
 * isochrones (tip[1] is read only when n_pops == 2).  Settings are checked as simCluster checks them. */
int b9h_sim_draw_systems(uint64_t seed, int64_t i0, int64_t n, double min_mass, double max_mass, double percent_binary,
                         double min_mass_ratio, double percent_db, int n_pops, double lambda, const double *tip,
                         double *mass1, double *mass_ratio, int32_t *wd_type, int32_t *pop);
/* field-star magnitudes of systems i0 .. i0+n-1 (purpose 4): mags[k][f] uniform in [lo[f], hi[f]] */
int b9h_sim_field_mags(uint64_t seed, int64_t i0, int64_t n, int n_filt, const double *lo, const double *hi, double *mags);
/* scatterCluster's noise (purpose 5) of the systems ids[0 .. n): sigma = sqrt(floor^2 + (at_limit 10^(0.2 (m - faint)))^2),
 * obs = m + sigma z; mags / sigma / obs [n][n_filt] */
int b9h_scatter(uint64_t seed, const int64_t *ids, int64_t n, int n_filt, const double *mags, double sigma_floor,
                double sigma_at_limit, double faint_limit, double *sigma, double *obs);
/* the resolved and checked simCluster (program 0) / scatterCluster (program 1) settings of a command line, "key = value" lines */
int b9h_sim_settings(int program, int argc, char **argv, char *out, int cap);
/* the rows of a chain file (.res) whose stage column equals `stage`, as full parameter rows (b9h::read_res_rows, what sampleMass
 * and sampleWDMass read; exposed for tests): start_row [B9_NPARAM] with the file's sampled columns written over it.  *n_rows
 * receives their number; rows (nullable: count only) receives the first min(*n_rows, cap_rows) of them, [row][B9_NPARAM] */
int b9h_read_res_rows(const char *path, const double *start_row, int stage, double *rows, long cap_rows, long *n_rows);
/* starSummary.  b9h_star_table: b9_star_moments' accumulators [n_stars][B9_MOM_N] -> the derived columns [n_stars][8]:
 * rows = acc0, member = acc1 / acc0, mass = acc2 / acc1, massSd = sqrt(max(0, acc3 / acc1 - mass^2)), massRatio and massRatioSd
 * likewise from acc4 and acc5, pBinary = acc6 / acc1, pPop2 = acc7 / acc1; with acc1 == 0 every derived value is 0.
 * b9h_write_star_summary: the file <base>.starSummary (docs/FORMATS.md) -- one header line, then per star
 * "id rows member mass massSd massRatio massRatioSd pBinary [pPop2]" (the last column with n_pops == 2 only), in the order of ids. */
int b9h_star_table(const double *acc, long n_stars, double *table);
int b9h_write_star_summary(const char *path, const char *const *ids, long n_stars, const double *acc, int n_pops);
/* wdSummary.  b9h_wd_table: b9_wd_moments' accumulators [n_wd][B9_WDM_N] -> the derived columns [n_wd][16]: rows = ROWS,
 * member = MEMBER / ROWS, pCooled = COOLED / MEMBER, zamsMass = M1 / MEMBER, zamsMassSd = sqrt(max(0, M1SQ / MEMBER - zamsMass^2)),
 * then a mean V / COOLED and an sd sqrt(max(0, V_SQ / COOLED - mean^2)) of wdMass, precLogAge, logCoolAge, logTeff and logg, and
 * pPop2 = POP1 / MEMBER; a derived column is 0 where its denominator is 0.
 * b9h_write_wd_summary: the file <base>.wdSummary (docs/FORMATS.md) -- one header line, then per WD-stage star "id rows member
 * pCooled zamsMass zamsMassSd wdMass wdMassSd precLogAge precLogAgeSd logCoolAge logCoolAgeSd logTeff logTeffSd logg loggSd
 * [pPop2]" (the last column with n_pops == 2 only), in the order of ids. */
int b9h_wd_table(const double *acc, long n_wd, double *table);
int b9h_write_wd_summary(const char *path, const char *const *ids, long n_wd, const double *acc, int n_pops);
/* massFunction.  b9h_mass_function_table: b9_mass_hist's row_hist [n_rows][n_bins + 1] -> the per-bin table [n_bins][8]:
 * lo, hi, then over the rows whose member column (the last) is > 0 the mean, the population standard deviation, the 16th, 50th
 * and 84th percentiles of the bin's expected count (linear interpolation between order statistics, numpy's default) and
 * dN/dlog10 m = mean / log10(hi / lo) (0 where lo <= 0); without such a row every statistic is 0.
 * b9h_write_mass_function: the file <base>.massFunction (docs/FORMATS.md), "lo hi mean sd p16 p50 p84 dNdlogM" per bin.
 * b9h_write_star_mass_hist: the file <base>.starMassHist, per star "id rows member bin0 .. bin<n-1>" with member =
 * star_hist[i][n_bins] / n_rows and bin b = star_hist[i][b] / star_hist[i][n_bins] (0 without membership weight).
 * b9h_mass_function_settings: massFunction's command line (argv[0] is skipped) and YAML parsed as the program parses them --
 * "key = value" lines of nBins, minMass, maxMass, linearBins, quantity (0 / 1 / 2), perStar, margIsoIncrem, nMassRatios, nPops
 * into out, and the nBins + 1 bin edges into edges (nullable); m_wd_up is the default maxMass. */
int b9h_mass_function_table(const double *row_hist, long n_rows, const double *edges, int n_bins, double *table);
int b9h_write_mass_function(const char *path, const double *table, int n_bins);
int b9h_write_star_mass_hist(const char *path, const char *const *ids, long n_stars, const double *star_hist, int n_bins, long n_rows);
int b9h_mass_function_settings(int argc, char **argv, double m_wd_up, char *out, int cap, double *edges);
/* binaryStats.  The tables of b9_ratio_hist's outputs, host arithmetic only.  A LINE is a mass bin b < n_mbins or, last, "all": its
 * cells per row are cell[j] = row_cells[r][b Q + j], for "all" the bins' cells added in ascending b.  Per row N = sum_j cell[j]
 * (ascending j), B = sum of the cell[j] with j >= 1 and (double)j / (double)Q >= q_min (ascending j; q_min exactly on a node counts
 * it), f = B / N.  A line's rows are those with member column (the last) > 0 and N > 0; the statistics are the mean, the population
 * standard deviation and the 16th / 50th / 84th percentiles by b9h_mass_function_table's rule, every one 0 without such a row.
 * b9h_binary_table: row_cells [n_rows][n_mbins Q + 1] -> [n_mbins + 1][13]: lo, hi (the line's edges; "all": the first and the last),
 * the number of rows, the five statistics of N, the five of f.
 * b9h_ratio_dist_table: -> [n_mbins + 1][Q][8]: j, q = j / Q, the number of rows, the five statistics of cell[j] / N.
 * b9h_star_ratio_table: star_cells [n_stars][n_mbins Q + 1] -> [n_stars][4 + Q]: rows = n_rows_in_grid (b9_ratio_hist does not count
 * rows: the caller passes the number it summed), member = total / rows, then with S_j = sum_b cell(b, j) (ascending b): inRange =
 * (sum_j S_j) / total, pBinaryAbove = (sum of the S_j that pass q_min) / total, and q<j> = S_j / total for every j; total == 0: every
 * derived value is 0.
 * Each fails (-1, b9h_last_error) for n_mbins < 1, Q < 1, q_min outside 0 .. 1 or a NULL pointer.
 * b9h_write_binary_fraction / b9h_write_ratio_dist / b9h_write_star_ratio: the files <base>.binaryFraction, <base>.ratioDist and
 * <base>.starRatio (docs/FORMATS.md) of those tables, 17 significant digits. */
int b9h_binary_table(const double *row_cells, long n_rows, const double *mass_edges, int n_mbins, int Q, double q_min, double *table);
int b9h_ratio_dist_table(const double *row_cells, long n_rows, int n_mbins, int Q, double *table);
int b9h_star_ratio_table(const double *star_cells, long n_stars, int n_mbins, int Q, double q_min, long n_rows_in_grid, double *table);
int b9h_write_binary_fraction(const char *path, const double *table, int n_mbins);
int b9h_write_ratio_dist(const char *path, const double *table, int n_mbins, int Q);
int b9h_write_star_ratio(const char *path, const char *const *ids, long n_stars, const double *table, int Q);
/* starIntervals.  b9h_refine_star_edges: one pass of the per-star refinement, a pure function of that pass's edges
 * [n_stars][n_bins + 1], b9_star_bins' acc [n_stars][n_bins + 3] and the levels 0 < a_1 < .. < a_m < 1 (3 m <= n_bins + 1), taken on
 * the counted mass C = below + sum bins + above.  Per star and level ([n_stars][n_levels]): the bracket [lo, hi) of the column in
 * which the cumulative sum first reaches a C, within 1e-13 C: the rounding of the sums, so that a level exactly between two nodes
 * goes to the lower one in every pass (-inf / +inf where that is `below` / `above`), the mass below lo and inside the
 * bracket, value = the linear interpolation inside it (an open bracket: its finite end), and is_final: hi - lo <= tol max(|lo|,
 * |hi|) or hi the next double after lo.  flags [n_stars]: 1 = C is 0 (values NaN), 2 = some bracket is not final.  next_edges
 * [n_stars][n_bins + 1], strictly ascending: a finished star keeps its edges; else every distinct bracket keeps its ends (an
 * open one widened) and the unfinished ones share the remaining edges evenly.
 * b9h_star_intervals_table: -> [n_stars][3 n_levels + 3]: member, then value, lo, hi per level, passes, flags.
 * b9h_write_star_intervals: the file <base>.starIntervals (docs/FORMATS.md) of that table, 17 significant digits.
 * b9h_star_intervals_settings: starIntervals' command line (argv[0] is skipped) and YAML parsed as the program parses them --
 * "key = value" lines of quantity (0 / 1 / 2), levels (comma-separated), tol, maxPasses, margIsoIncrem, nMassRatios, nPops. */
int b9h_refine_star_edges(const double *edges, const double *acc, long n_stars, int n_bins, const double *levels, int n_levels, double tol,
                          double *lo, double *hi, double *below, double *inside, double *value, int32_t *is_final, int32_t *flags, double *next_edges);
int b9h_star_intervals_table(long n_stars, int n_levels, const double *member, const double *value, const double *lo, const double *hi,
                             const int32_t *passes, const int32_t *flags, double *table);
int b9h_write_star_intervals(const char *path, const char *const *ids, long n_stars, const double *levels, int n_levels, const double *table);
int b9h_star_intervals_settings(int argc, char **argv, char *out, int cap);
/* wdIntervals.  The lines are [n_wd][n_sel]: WD-stage star i, s-th selected quantity of quantity_mask (bit q = enum
 * b9_wd_quantity q, ascending); b9h_refine_star_edges serves them unchanged with n_stars = n_wd n_sel.
 * b9h_wd_first_ranges: the lines' first ranges from b9_wd_moments' accumulators [n_wd][B9_WDM_N] over the same rows and nodes:
 * the quantity's mean over its counted mass (MEMBER for the ZAMS mass, COOLED for the derived ones) -/+ max(6 sd, 1e-3 |mean|)
 * (1 where that is not positive); a line with no counted mass gets [0, 1].
 * b9h_wd_intervals_table: -> [n_wd][1 + n_sel (3 n_levels + 3)]: member (of the star's first line), then per selected quantity
 * counted, {value, lo, hi} per level, passes, flags; member, counted, passes, flags are [n_wd][n_sel], the others
 * [n_wd][n_sel][n_levels].
 * b9h_write_wd_intervals: the file <base>.wdIntervals (docs/FORMATS.md) of that table, 17 significant digits.
 * b9h_wd_intervals_settings: wdIntervals' command line (argv[0] is skipped) and YAML parsed as the program parses them --
 * "key = value" lines of quantities (the mask), levels (comma-separated), tol, maxPasses, nMassNodes, nPops. */
int b9h_wd_first_ranges(const double *wd_acc, long n_wd, int quantity_mask, double *first_lo, double *first_hi);
int b9h_wd_intervals_table(long n_wd, int n_sel, int n_levels, const double *member, const double *counted, const double *value, const double *lo,
                           const double *hi, const int32_t *passes, const int32_t *flags, double *table);
int b9h_write_wd_intervals(const char *path, const char *const *ids, long n_wd, int quantity_mask, const double *levels, int n_levels, const double *table);
int b9h_wd_intervals_settings(int argc, char **argv, char *out, int cap);
/* cmdBand.  The lines are b9_cmd_band's, n_lines = n_pops P C; b9h_refine_star_edges serves them unchanged with n_stars = n_lines.
 * b9h_band_first_ranges: from b9_cmd_band's moments [n_lines][B9_BAND_NMOM], per line, the first range [lo, hi] = [MIN - pad,
 * MAX + pad], pad = max(0.01 (MAX - MIN), 1e-6 max(1, |MIN|, |MAX|)); a line with N = 0 gets [0, 1].  What the refinement loop
 * (b9h::interval_loop, hostlib.interval_loop) cuts evenly for its first pass.
 * b9h_band_first_edges: that cut, the n_bins + 1 strictly ascending edges lo + (hi - lo) (b / n_bins): e_0 < MIN and e_B > MAX.
 * b9h_band_table: -> [n_lines][5 + 3 n_levels + 2]: N, mean = pivot + SUM / N (pivot NULL: 0), sd = sqrt(max(0, SUMSQ / N -
 * (SUM / N)^2)), the population standard deviation, min, max, then value, lo, hi per level, passes, flags; N = 0: mean and sd NaN.
 * b9h_write_cmd_band: the file <base>.cmdBand (docs/FORMATS.md) of that table through the shared table writer, 17 significant
 * digits; names [n_lines]: the lines' labels.
 * b9h_cmd_band_settings: cmdBand's command line (argv[0] is skipped) and YAML parsed as the program parses them -- "key = value"
 * lines of ratios (comma-separated), wdNodes, wdTypes (the mask: 1 da, 2 db, 3 both), colours (f1-f2,..), levels, tol, maxPasses,
 * nPops. */
int b9h_band_first_ranges(const double *mom, long n_lines, double *first_lo, double *first_hi);
int b9h_band_first_edges(const double *mom, long n_lines, int n_bins, double *edges);
int b9h_band_table(const double *mom, const double *pivot, long n_lines, int n_levels, const double *value, const double *lo, const double *hi,
                   const int32_t *passes, const int32_t *flags, double *table);
int b9h_write_cmd_band(const char *path, const char *const *names, long n_lines, const double *levels, int n_levels, const double *table);
int b9h_cmd_band_settings(int argc, char **argv, char *out, int cap);
/* photResiduals.  b9h_resid_table: b9_phot_resid's star_resid [n_stars][2 + 2 n_filt] with the catalogue's obs and sigma
 * [n_stars][n_filt] (sigma <= 0: filter unused) -> the per-star table [n_stars][2 + 4 n_filt]: rows, member = acc[1] / rows,
 * then per filter predMag = c + acc[2 + 2f] / acc[1] (c = obs for a used filter, else 0), predSd = sqrt(max(0, acc[3 + 2f] / acc[1]
 * - (acc[2 + 2f] / acc[1])^2)) and, for used filters (0 otherwise), resid = obs - predMag and rmsZ = sqrt(acc[3 + 2f] / acc[1]) / sigma;
 * every derived value is 0 when acc[1] == 0.
 * b9h_filter_resid_table: row_resid [n_rows][1 + 5 n_filt] -> the per-filter table [n_filt][16]: the number of rows with
 * N_f > 0, then over them the mean, population standard deviation and 16th / 50th / 84th percentiles (b9h_mass_function_table's
 * rule) of meanZ = R_f / N_f, chi2 = C_f / N_f and offset = D_f / W_f; zeros without such a row.
 * b9h_write_phot_resid / b9h_write_filter_resid: the files <base>.photResid and <base>.filterResid (docs/FORMATS.md) of those
 * tables, 17 significant digits.  b9h_phot_resid_settings: photResiduals' command line (argv[0] is skipped) and YAML parsed
 * as the program parses them -- "key = value" lines of margIsoIncrem, nMassRatios, nPops, perStar into out. */
int b9h_resid_table(const double *star_resid, const double *obs, const double *sigma, long n_stars, int n_filt, double *table);
int b9h_filter_resid_table(const double *row_resid, long n_rows, int n_filt, double *table);
int b9h_write_phot_resid(const char *path, const char *const *ids, long n_stars, const char *const *filters, int n_filt, const double *table);
int b9h_write_filter_resid(const char *path, const char *const *filters, int n_filt, const double *table);
int b9h_phot_resid_settings(int argc, char **argv, char *out, int cap);
/* filterCheck.  b9h_loo_table: b9_filter_loo's star_loo [n_stars][2 + 3 n_filt] with the catalogue's obs and sigma
 * [n_stars][n_filt] (sigma <= 0: filter unused) -> the per-star table [n_stars][2 + 5 n_filt]: rows, member = acc[1] / rows,
 * then per filter looMag = c + acc[2 + 3f] / acc[1] (c = obs for a used filter, else 0), looSd = sqrt(var), var = max(0,
 * acc[3 + 3f] / acc[1] - (acc[2 + 3f] / acc[1])^2) the between-node variance, and, for used filters (0 otherwise), resid = obs -
 * looMag, z = resid / sqrt(sigma^2 + var) -- the predictive z, which a calibrated fit spreads like N(0, 1) -- and lpd =
 * acc[4 + 3f] / acc[1]; every derived value is 0 when acc[1] == 0.
 * b9h_filter_loo_table: row_loo [n_rows][1 + 6 n_filt] -> the per-filter table [n_filt][21]: the number of rows with N_f > 0,
 * then over them the mean, population standard deviation and 16th / 50th / 84th percentiles (b9h_mass_function_table's rule) of
 * meanZ = R_f / N_f, chi2 = C_f / N_f, offset = D_f / W_f and lpd = E_f / N_f; zeros without such a row.
 * b9h_write_star_filter_check / b9h_write_filter_check: the files <base>.starFilterCheck and <base>.filterCheck
 * (docs/FORMATS.md) of those tables, 17 significant digits.  b9h_filter_check_settings: filterCheck's command line (argv[0] is
 * skipped) and YAML parsed as the program parses them -- "key = value" lines of margIsoIncrem, nMassRatios, nPops, perStar. */
int b9h_loo_table(const double *star_loo, const double *obs, const double *sigma, long n_stars, int n_filt, double *table);
int b9h_filter_loo_table(const double *row_loo, long n_rows, int n_filt, double *table);
int b9h_write_star_filter_check(const char *path, const char *const *ids, long n_stars, const char *const *filters, int n_filt, const double *table);
int b9h_write_filter_check(const char *path, const char *const *filters, int n_filt, const double *table);
int b9h_filter_check_settings(int argc, char **argv, char *out, int cap);
/* starOffsets.  b9h_offset_direction: k [n_filt] of a direction spec -- "absorption" (abs_coeff [n_filt], the pack's absorption
 * coefficients; NULL: an error for this spec), "distance" (1 in every filter), "filter:NAME" (a unit vector) or n_filt
 * comma-separated values.
 * b9h_offset_table: b9_star_offset's star_off [n_stars][2 + 3 n_dir] with the catalogue's sigma [n_stars][n_filt] (sigma <= 0:
 * filter unused) and the call's k [n_dir][n_filt], tau [n_dir] -> the per-star table [n_stars][2 + 4 n_dir]: rows, member =
 * acc[1] / rows, then per direction mean = acc[2 + 3j] / acc[1], sd = sqrt(max(0, acc[3 + 3j] / acc[1] - mean^2) + V) with
 * V = 1 / (sum_f (k_f / sigma_f)^2 + tau^-2), z = mean / sd and logBF = acc[4 + 3j] / acc[1]; every derived value is 0 when
 * acc[1] == 0.
 * b9h_offset_dist_table: row_off [n_rows][1 + 4 n_dir] -> the per-direction table [n_dir][16]: the number of rows with N > 0,
 * then over them the mean, population standard deviation and 16th / 50th / 84th percentiles (b9h_mass_function_table's rule) of
 * mean = M1 / N, rms = sqrt(M2 / N) and logBF = E / N; zeros without such a row.
 * b9h_write_star_offsets / b9h_write_offset_dist: the files <base>.starOffsets and <base>.offsetDist (docs/FORMATS.md) of those
 * tables, 17 significant digits; `directions` names the columns / lines.  b9h_star_offsets_settings: starOffsets' command line
 * (argv[0] is skipped) and YAML parsed as the program parses them -- "key = value" lines of margIsoIncrem, nMassRatios, nPops,
 * direction, tau (the last two space-separated, one tau per direction). */
int b9h_offset_direction(const char *spec, const char *const *filters, int n_filt, const double *abs_coeff, double *k);
int b9h_offset_table(const double *star_off, const double *sigma, const double *k, const double *tau, long n_stars, int n_filt, int n_dir, double *table);
int b9h_offset_dist_table(const double *row_off, long n_rows, int n_dir, double *table);
int b9h_write_star_offsets(const char *path, const char *const *ids, long n_stars, const char *const *directions, int n_dir, const double *table);
int b9h_write_offset_dist(const char *path, const char *const *directions, int n_dir, const double *table);
int b9h_star_offsets_settings(int argc, char **argv, char *out, int cap);
/* modelScore.  b9h_pointwise_table: b9_pointwise's acc [n_stars][8] and tail [n_stars][tail_len] (NULL or tail_len 0: no PSIS
 * fit) -> the per-star table [n_stars][9]: rows, nInf, lppd, pWaic, elpdWaic, elpdIs, paretoK, elpdLoo, pLoo.  With n_f = rows -
 * nInf: lppd = VMAX + log SPOS - log rows, pWaic = M2 / (n_f - 1) (0 for n_f < 2), elpdWaic = lppd - pWaic, elpdIs = log n_f -
 * (RMAX + log SNEG); paretoK and elpdLoo by Pareto-smoothed importance sampling of the tail (Vehtari, Gelman & Gabry 2017; the
 * generalised Pareto fit of Zhang & Stephens 2009; DESIGN.md section 2 states every step), paretoK NaN and elpdLoo = elpdIs where
 * the tail is too short to fit; pLoo = lppd - elpdLoo.  nInf > 0: elpdWaic = elpdIs = elpdLoo = -inf, paretoK = pLoo = +inf.
 * rows = 0: every value 0.
 * b9h_score_totals: over the stars with rows > 0 -> totals [12]: their number N, sum and se = sqrt(N var_ddof1) of lppd, of
 * elpdWaic and of elpdLoo, sum pWaic, sum pLoo, the stars with nInf > 0, the stars with paretoK > 0.7, the largest finite paretoK.
 * b9h_score_compare: two tables of the same catalogue -> out [6]: the stars with rows > 0 in both, then sum and se of
 * elpdLoo_A - elpdLoo_B and of elpdWaic_A - elpdWaic_B, then the stars with rows > 0 in exactly one table (left out, reported); fails (-1, b9h_last_error) when the ids differ in content or order.
 * b9h_write_pointwise / b9h_write_model_score: the files <base>.pointwise and <base>.modelScore (docs/FORMATS.md).
 * b9h_model_score_settings: modelScore's command line (argv[0] is skipped) and YAML parsed as the program parses them --
 * "key = value" lines of margIsoIncrem, nMassRatios, nPops, perRow, compareTo into out. */
int b9h_pointwise_table(const double *acc, const double *tail, int tail_len, long n_stars, double *table);
int b9h_score_totals(const double *table, long n_stars, double *totals);
int b9h_score_compare(const double *table_a, const char *const *ids_a, long n_a, const double *table_b, const char *const *ids_b, long n_b, double *out);
int b9h_write_pointwise(const char *path, const char *const *ids, long n_stars, const double *table);
int b9h_write_model_score(const char *path, const double *totals);
int b9h_model_score_settings(int argc, char **argv, char *out, int cap);
/* starInfluence.  b9h_influence_table: b9_star_influence's acc [n_stars][6 + 4 n_q] and tail (NULL or tail_len 0: no PSIS fit) ->
 * the per-star table [n_stars][4 + 3 n_q]: rows, nInf, ess = SNEG^2 / SNEG2, paretoK (modelScore's fit of the tail; NaN where none is
 * made), then per quantity shift = WQ / SNEG - MQ (the move of the quantity's mean when the star is deleted), lin = -CVQ / (n_f - 1)
 * (its first-order form, 0 for n_f < 2) and looSd = sqrt(max(0, WQ2 / SNEG - (WQ / SNEG)^2)).  nInf > 0: ess = 0, the rest NaN.
 * rows = 0: every value 0.
 * b9h_group_influence_table: group_lpd [n_rows][n_groups], the call's q [n_rows][n_q] and the stars' ids [n_stars] -> the per-group
 * table [n_groups][5 + 3 n_q]: nStars, rows, nInf (the rows whose sum is -inf), ess, paretoK, then per quantity shiftRaw, shift (the M
 * largest weights Pareto-smoothed; = shiftRaw where the fit is refused) and looSd.  nInf > 0: ess = 0, the rest NaN.
 * b9h_influence_quantities / b9h_influence_groups: what the program passes to the call, from its command line (argv[0] is skipped)
 * and YAML: the quantities' names (space-joined into names), their z-scores q [n_rows][n_q] over rows [n_rows][B9_NPARAM] (log_post
 * may be NULL) with mean and sd [n_q]; the groups' names and every star's id (-1: none) from the catalogue's ids and stages.  The
 * arrays hold B9_INF_MAX_Q / B9_INF_MAX_GROUPS entries per row / in all.
 * b9h_write_star_influence / b9h_write_group_influence: the files <base>.starInfluence and <base>.groupInfluence (docs/FORMATS.md).
 * b9h_star_influence_settings: "key = value" lines of margIsoIncrem, nMassRatios, nPops, quantity, groupFile, noGroups into out. */
int b9h_influence_table(const double *acc, const double *tail, int tail_len, long n_stars, int n_q, double *table);
int b9h_group_influence_table(const double *group_lpd, long n_rows, int n_groups, const double *q, int n_q, const int32_t *group, long n_stars, double *table);
int b9h_influence_quantities(int argc, char **argv, const double *rows, const double *log_post, long n_rows, char *names, int cap, double *q, double *mean, double *sd,
                             int *n_q);
int b9h_influence_groups(int argc, char **argv, const char *const *ids, const int32_t *stage, long n_stars, char *names, int cap, int32_t *group, int *n_groups);
int b9h_write_star_influence(const char *path, const char *const *ids, long n_stars, const char *const *quantities, int n_q, const double *table);
int b9h_write_group_influence(const char *path, const char *const *groups, int n_groups, const char *const *quantities, int n_q, const double *table);
int b9h_star_influence_settings(int argc, char **argv, char *out, int cap);
/* rank 0's merge of <final_path>.part<r> into <final_path> after a --gpus N run (b9h::merge_result_parts; exposed for tests) */
int b9h_merge_parts(const char *final_path, int world, int walkers_per_rank, long rows_per_part);

#ifdef __cplusplus
}
#endif
#endif /* BASE9_HOST_H */
