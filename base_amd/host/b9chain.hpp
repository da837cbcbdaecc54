// b9chain.hpp -- what the programs over a saved chain (sampleMass, sampleWDMass, starSummary, wdSummary, wdIntervals, cmdBand, massFunction,
// binaryStats, starIntervals, photResiduals, filterCheck, starOffsets, modelScore, starInfluence) share above the C ABI and below their mains: their settings, the loop over the
// chain's rows, the tables derived from the device's sums and the files they are written to (docs/FORMATS.md).  Host arithmetic
// only: nothing here needs a context or a GPU.  b9host.hpp includes this header.
#pragma once
#include "b9host.hpp"

#include <algorithm>
#include <chrono>
#include <functional>

namespace b9h {

// ---- settings --------------------------------------------------------------------------------------
// The population count and the marginalisation grid of the program whose settings section is `section` (starSummary,
// massFunction, starIntervals, photResiduals, modelScore):
//   n_pops = <section>.nPops (1); K = <section>.margIsoIncrem, Q = <section>.nMassRatios, each defaulting to sampleMass's, then 4.
// Throws "<section>.nPops must be 1 or 2" / "margIsoIncrem and nMassRatios must be positive".
struct ChainGrid { int n_pops, K, Q; };
ChainGrid chain_grid(const Settings &st, const std::string &section);
int chain_n_pops(const Settings &st, const std::string &section);         // the first line alone (wdSummary has no grid)
ChainGrid sample_mass_grid(const Settings &st);                           // sampleMass: one population, sampleMass.* (4 each) alone
// <section>.nMassNodes of sampleWDMass / wdSummary, defaulting to sampleWDMass's, then 512; 1 .. 2147483647
long wd_mass_nodes(const Settings &st, const std::string &section);

// Each program's own spellings of shared flags (Settings::parse_args' second table): the short names belong to simCluster
// (--minMass --maxMass --nPops) and massFunction (--quantity --perStar) in the shared table.
extern const ProgramFlags kMassFunctionFlags, kStarIntervalsFlags, kPhotResidFlags, kFilterCheckFlags, kModelScoreFlags;

// massFunction.{nBins, minMass, maxMass, linearBins, quantity, perStar} (flags --nBins --minMass --maxMass --linearBins --quantity
// --perStar).  Default: 24 log-spaced bins over [0.1, M_wd_up] of the primary mass.
struct MassFunctionConfig {
    int n_bins, quantity;
    double min_mass, max_mass;
    bool linear, per_star;
    std::vector<double> edges() const;       // n_bins + 1, strictly ascending; the end points are min_mass and max_mass exactly
};
MassFunctionConfig mass_function_config(const Settings &st, double m_wd_up);
// starIntervals.{quantity, levels, tol, maxPasses} (flags --quantity --levels a,b,.. --tol --maxPasses)
struct StarIntervalsConfig {
    int quantity, max_passes;
    double tol;
    std::vector<double> levels;
};
StarIntervalsConfig star_intervals_config(const Settings &st);
// photResiduals.perStar (--perStar): the per-star file as well
struct PhotResidConfig { bool per_star; };
PhotResidConfig phot_resid_config(const Settings &st);
// filterCheck.perStar (--perStar): the per-star file as well
struct FilterCheckConfig { bool per_star; };
FilterCheckConfig filter_check_config(const Settings &st);
// modelScore.{perRow, compareTo} (--perRow, --compareTo otherBase): the per-row file as well; compare two fits instead
struct ModelScoreConfig { bool per_row; std::string compare_to; };
ModelScoreConfig model_score_config(const Settings &st);
// the tail kept per star for a chain of n_rows rows: min(256, min(floor(S / 5), ceil(3 sqrt S)) + 1)
int model_score_tail_len(long n_rows);

// ---- the loop over the chain's rows ------------------------------------------------------------------
// fn(r0, m) for r0 = 0, batch, 2 batch, .. with m = min(batch, n_rows - r0) rows each; -> the seconds it took.  A reduction
// continues the sums of the call before (its B9_*_CONTINUE flag) where r0 != 0.
constexpr long kChainBatch = 256;
template <class Fn> double for_row_batches(long n_rows, Fn &&fn, long batch = kChainBatch)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (long r0 = 0; r0 < n_rows; r0 += batch) fn(r0, std::min(batch, n_rows - r0));
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// ---- files -------------------------------------------------------------------------------------------
// One text table: a header line -- label_name (when there are labels), then the columns' names --, then n_lines lines of
// [labels[i]] and values[i * stride + c] printed with cols[c].fmt, everything separated by single spaces.  A format ending in
// 'd' ("%ld") prints the value as a long.  Throws "cannot write <path>" when the file cannot be opened or closed.
struct TableColumn { std::string name; const char *fmt; };
void write_table(const std::string &path, const char *label_name, const std::vector<std::string> *labels, const std::vector<TableColumn> &cols,
                 long n_lines, const double *values, size_t stride);

// ---- starSummary -----------------------------------------------------------------------------------
// b9_star_moments' accumulators [n_stars][B9_MOM_N] -> the derived columns [n_stars][kStarTableCols]:
//   rows = acc0, member = acc1 / acc0, mass = acc2 / acc1, massSd = sqrt(max(0, acc3 / acc1 - mass^2)), ratio and ratioSd
//   likewise from acc4, acc5, pBinary = acc6 / acc1, pPop2 = acc7 / acc1; with acc1 == 0 every derived value is 0.
// (Raw second moments in fp64 lose about 2^-52 mass^2 / var relatively: a one-node posterior comes out a few 1e-17 negative,
// hence the clamp.)
constexpr int kStarTableCols = 8;
void star_table(const double *acc, long n_stars, double *table);
// <base>.starSummary: a header line, then one line per star in the order of `ids`:
// id rows member mass massSd massRatio massRatioSd pBinary [pPop2 -- two populations only]
void write_star_summary(const std::string &path, const std::vector<std::string> &ids, const double *acc, int n_pops);

// ---- wdSummary -------------------------------------------------------------------------------------
// b9_wd_moments' accumulators [n_wd][B9_WDM_N] -> the derived columns [n_wd][kWdTableCols]:
//   rows = ROWS, member = MEMBER / ROWS, pCooled = COOLED / MEMBER, zamsMass and zamsMassSd from M1, M1SQ over MEMBER, then a
//   mean and an sd = sqrt(max(0, E[v^2] - E[v]^2)) of wdMass, precLogAge, logCoolAge, logTeff, logg over COOLED, and
//   pPop2 = POP1 / MEMBER.  A derived column is 0 where its denominator is 0.
constexpr int kWdTableCols = 16;
void wd_table(const double *acc, long n_wd, double *table);
// <base>.wdSummary: a header line, then one line per WD-stage star in the order of `ids`:
// id rows member pCooled zamsMass zamsMassSd wdMass wdMassSd precLogAge precLogAgeSd logCoolAge logCoolAgeSd logTeff logTeffSd
// logg loggSd [pPop2 -- two populations only]
void write_wd_summary(const std::string &path, const std::vector<std::string> &ids, const double *acc, int n_pops);

// ---- massFunction ----------------------------------------------------------------------------------
// b9_mass_hist's row_hist [n_rows][n_bins + 1] -> the per-bin table [n_bins][kMassFunctionCols]:
//   lo, hi, then over the rows whose member column (the last) is > 0 the mean, the population standard deviation and the 16th,
//   50th and 84th percentiles of the bin's expected count (linear interpolation between order statistics at (n - 1) q, numpy's
//   default), and dN/dlog10 m = mean / log10(hi / lo) (0 where lo <= 0).  No such row: every statistic is 0.
constexpr int kMassFunctionCols = 8;
void mass_function_table(const double *row_hist, long n_rows, const double *edges, int n_bins, double *table);
// <base>.massFunction: "lo hi mean sd p16 p50 p84 dNdlogM", one line per bin
void write_mass_function(const std::string &path, const double *table, int n_bins);
// <base>.starMassHist: "id rows member bin0 .. bin<n-1>", per star its id, the rows counted, the mean membership
// acc[total] / rows and the posterior probabilities acc[b] / acc[total] (zeros without membership weight)
void write_star_mass_hist(const std::string &path, const std::vector<std::string> &ids, const double *star_hist, int n_bins, long n_rows);

// ---- starIntervals ---------------------------------------------------------------------------------
// One pass of the per-star refinement: a pure function of that pass's edges [n_stars][n_bins + 1], b9_star_bins' acc
// [n_stars][n_bins + 3] (below, the bins, at or above, the total) and the levels 0 < a_1 < .. < a_m < 1 (3 m <= n_bins + 1).  The
// levels are taken on the counted mass C = below + sum bins + above, summed in that order.  Per star and level ([n_stars][m]):
//   lo, hi     the bracket [lo, hi) of the column in which the cumulative sum first reaches a C, within kSivSlack C (-inf / +inf:
//              the level lies in `below` / `above`, and the next pass widens the range)
//   below, inside   the mass below lo and inside the bracket
//   value      lo + (hi - lo) (a C - below) / inside, the linear interpolation inside the bracket (an open bracket: its finite end)
//   is_final   hi - lo <= tol max(|lo|, |hi|), or hi is the next double after lo (an open bracket is never final)
// flags [n_stars]: kSivNoMass: C = 0 -- every value NaN, nothing left to do; kSivOpen: some bracket is not final.
// next_edges [n_stars][n_bins + 1], strictly ascending: a star without kSivOpen keeps its edges; else every distinct bracket keeps
// its two ends, and the edges left over are shared evenly among the unfinished brackets as interior points (coinciding brackets
// share theirs).  Nothing is carried from pass to pass.
constexpr int32_t kSivNoMass = 1, kSivOpen = 2;
constexpr double kSivSlack = 1e-13;        // "reaches a C" means within this much of C: the rounding of the sums (ties go to the lower node)
void refine_star_edges(const double *edges, const double *acc, long n_stars, int n_bins, const double *levels, int n_levels, double tol,
                       double *lo, double *hi, double *below, double *inside, double *value, int32_t *is_final, int32_t *flags, double *next_edges);
// The loop: the first pass's edges are [0, 2 max_mass] cut evenly for every star; `bins` runs one b9_star_bins over all the rows
// from zeros; it ends when no star has kSivOpen or after max_passes.  passes: the pass at which the star was finished.
struct StarIntervals {
    int n_levels = 0;
    long n_stars = 0;
    std::vector<double> member, value, lo, hi;      // [n_stars], then [n_stars][n_levels]
    std::vector<int32_t> is_final, passes, flags;   // [n_stars][n_levels], [n_stars], [n_stars]
};
using StarBinsFn = std::function<void(const double *edges, int n_bins, double *acc)>;
StarIntervals star_intervals(const StarBinsFn &bins, long n_stars, long n_rows, int n_bins, double max_mass, const std::vector<double> &levels, double tol,
                             int max_passes);
// ... and the loop itself, over n_lines independent lines whose first pass cuts [first_lo[i], first_hi[i]] (finite, lo < hi)
// evenly: star_intervals is this loop with [0, 2 max_mass] for every star.  counted [n_lines] (may be null): the last pass's
// counted mass C over its total column (0 where the total is 0).
StarIntervals interval_loop(const StarBinsFn &bins, long n_lines, long n_rows, int n_bins, const double *first_lo, const double *first_hi,
                            const std::vector<double> &levels, double tol, int max_passes, std::vector<double> *counted = nullptr);
// -> [n_stars][3 m + 3]: member, then value, lo, hi per level, passes, flags
void star_intervals_table(const StarIntervals &r, double *table);
// <base>.starIntervals: "id member {q<a> q<a>_lo q<a>_hi} passes flags", one line per star in the order of ids, 17 significant digits
void write_star_intervals(const std::string &path, const std::vector<std::string> &ids, const std::vector<double> &levels, const double *table);

// ---- wdIntervals -----------------------------------------------------------------------------------
// wdIntervals.{quantities, levels, tol, maxPasses, nMassNodes} (flags --quantities zamsMass,wdMass,.. --levels a,b,.. --tol
// --maxPasses --nMassNodes).  Default: all six quantities at starIntervals' levels, 1e-4 relative, 12 passes; nMassNodes
// defaults to wdSummary's, then sampleWDMass's, then 512.
extern const ProgramFlags kWdIntervalsFlags;
extern const char *const kWdQuantityNames[B9_WQ_N];         // zamsMass wdMass precLogAge logCoolAge logTeff logg
struct WdIntervalsConfig {
    int quantity_mask, max_passes;
    long n_nodes;
    double tol;
    std::vector<double> levels;
    int n_sel() const { return __builtin_popcount((unsigned)quantity_mask); }
};
WdIntervalsConfig wd_intervals_config(const Settings &st);
// The first ranges of the lines [n_wd][n_sel] from one b9_wd_moments pass over the same rows and nodes (acc [n_wd][B9_WDM_N]):
// the quantity's mean over its counted mass (MEMBER for the ZAMS mass, COOLED for the derived ones) -/+ max(6 sd, 1e-3 |mean|)
// (1 where that is not positive); a line with no counted mass gets [0, 1].  The open columns widen a range that is too narrow.
void wd_first_ranges(const double *wd_acc, long n_wd, int quantity_mask, double *first_lo, double *first_hi);
// The loop: interval_loop over the n_wd * n_sel lines with those first ranges; `moments` runs one b9_wd_moments over all the
// rows from zeros, `bins` one b9_wd_bins.
struct WdIntervals {
    long n_wd = 0;
    int n_sel = 0;
    StarIntervals lines;                  // n_stars = n_wd * n_sel
    std::vector<double> counted;          // [n_wd][n_sel]
};
using WdMomentsFn = std::function<void(double *acc /* [n_wd][B9_WDM_N] */)>;
WdIntervals wd_intervals(const WdMomentsFn &moments, const StarBinsFn &bins, long n_wd, long n_rows, int quantity_mask, const std::vector<double> &levels,
                         double tol, int max_passes);
// -> [n_wd][1 + n_sel (3 m + 3)]: member, then per selected quantity counted, {value, lo, hi} per level, passes, flags
void wd_intervals_table(long n_wd, int n_sel, int n_levels, const double *member, const double *counted, const double *value, const double *lo,
                        const double *hi, const int32_t *passes, const int32_t *flags, double *table);
void wd_intervals_table(const WdIntervals &r, double *table);
// <base>.wdIntervals: "id member {N_counted {N_q<a> N_q<a>_lo N_q<a>_hi} N_passes N_flags}" for the selected quantities' names
// N, one line per WD-stage star in the order of ids, 17 significant digits
void write_wd_intervals(const std::string &path, const std::vector<std::string> &ids, int quantity_mask, const std::vector<double> &levels,
                        const double *table);

// ---- cmdBand ---------------------------------------------------------------------------------------
// cmdBand.{ratios, wdNodes, wdTypes, colours, levels, tol, maxPasses, nPops} (flags --ratios a,b,.. --wdNodes n --wdTypes
// da|db|both --colours f1-f2,.. --levels a,b,.. --tol --maxPasses --nPops).  Default: the loci q = 0 and q = 1, 256 WD points of
// the DA sequence, no colours, starIntervals' levels, 1e-4 relative, 12 passes, one population.
extern const ProgramFlags kCmdBandFlags;
struct CmdBandConfig {
    std::vector<double> ratios;                                   // 0 .. B9_BAND_MAX_RATIOS, each in [0, 1]
    long wd_nodes;                                                // >= 0
    int wd_types, max_passes;                                     // wd_types: bit 0 DA, bit 1 DB
    std::vector<std::pair<std::string, std::string>> colours;     // filter names (f1, f2), at most B9_BAND_MAX_COLOURS
    double tol;
    std::vector<double> levels;
};
CmdBandConfig cmd_band_config(const Settings &st);
// the colours' filter indices [n_colour][2] among `filters`; throws for a name that is none of them or a colour of one filter
std::vector<int32_t> band_colour_ids(const CmdBandConfig &c, const std::vector<std::string> &filters);
// The lines of a spec in b9_cmd_band's order, n_pops P C of them, named "p<k>.<locus>.<point>.<column>": locus q<s> with point
// eep<e>, or da / db with point n<j>; column mass, a filter's name, or <f1>-<f2>.
std::vector<std::string> band_line_names(int n_pops, int eep0, int n_eep, int n_ratio, long wd_nodes, int wd_types, const std::vector<std::string> &filters,
                                         const std::vector<int32_t> &colour_ids);
// The first pass's range of every line from b9_cmd_band's moments [n_lines][B9_BAND_NMOM]: [MIN - pad, MAX + pad] with pad =
// max(0.01 (MAX - MIN), 1e-6 max(1, |MIN|, |MAX|)); a line with N = 0 gets [0, 1].  band_first_edges: the n_bins + 1 edges
// interval_loop cuts that range into, lo + (hi - lo) (b / n_bins): strictly ascending, e_0 < MIN, e_B > MAX.
void band_first_ranges(const double *mom, long n_lines, double *first_lo, double *first_hi);
void band_first_edges(const double *mom, long n_lines, int n_bins, double *edges);
// The loop: one `moments` pass over all the rows (b9_cmd_band with the pivots, from its starting state) gives the first ranges,
// then interval_loop with `bins` (one b9_cmd_band bins pass over all the rows from zeros) over B9_BAND_MAX_BINS bins.
struct CmdBand {
    long n_lines = 0;
    std::vector<double> mom;              // [n_lines][B9_BAND_NMOM]
    StarIntervals lines;                  // n_stars = n_lines
};
using BandMomentsFn = std::function<void(double *mom /* [n_lines][B9_BAND_NMOM] */)>;
CmdBand cmd_band(const BandMomentsFn &moments, const StarBinsFn &bins, long n_lines, long n_rows, const std::vector<double> &levels, double tol, int max_passes);
// -> [n_lines][5 + 3 m + 2]: N, mean = pivot + SUM / N, sd = sqrt(max(0, SUMSQ / N - (SUM / N)^2)) (the population standard
// deviation), min, max, then value, lo, hi per level, passes, flags.  N = 0: mean and sd NaN, min +inf, max -inf as accumulated.
void band_table(const double *mom, const double *pivot, long n_lines, int n_levels, const double *value, const double *lo, const double *hi,
                const int32_t *passes, const int32_t *flags, double *table);
// <base>.cmdBand: "line N mean sd min max {q<a> q<a>_lo q<a>_hi} passes flags", one line per band line named by `names`, 17
// significant digits
void write_cmd_band(const std::string &path, const std::vector<std::string> &names, const std::vector<double> &levels, const double *table);

// ---- photResiduals ---------------------------------------------------------------------------------
// b9_phot_resid's star_resid [n_stars][2 + 2 nf] with the catalogue's obs / sigma [n_stars][nf] -> the per-star table
// [n_stars][2 + 4 nf]: rows, member (= acc[1] / rows), then per filter
//   predMag = c + acc[2 + 2f] / acc[1]        (c: obs where sigma > 0, else 0 -- the call's pivot)
//   predSd  = sqrt(max(0, acc[3 + 2f] / acc[1] - (acc[2 + 2f] / acc[1])^2))
//   resid   = obs - predMag                   (used filters; 0 for an unused one)
//   rmsZ    = sqrt(acc[3 + 2f] / acc[1]) / sigma   (likewise)
// Every derived value is 0 when acc[1] == 0.
void resid_table(const double *star_resid, const double *obs, const double *sigma, long n_stars, int nf, double *table);
// b9_phot_resid's row_resid [n_rows][1 + 5 nf] -> the per-filter table [nf][kFilterResidCols]: the number of rows with N_f > 0,
// then over those rows the mean, the population standard deviation and the 16th / 50th / 84th percentiles (mass_function_table's
// rule) of meanZ = R_f / N_f, of chi2 = C_f / N_f and of offset = D_f / W_f.  No such row: every entry 0.
constexpr int kFilterResidCols = 16;
void filter_resid_table(const double *row_resid, long n_rows, int nf, double *table);
// <base>.photResid: "id rows member {<filter>_predMag <filter>_predSd <filter>_resid <filter>_rmsZ}", one line per star in the
// order of ids; <base>.filterResid: "filter nRows {meanZ chi2 offset}_{mean sd p16 p50 p84}", one line per filter.
// Numbers are written with 17 significant digits: the files read back to the tables' bits.
void write_phot_resid(const std::string &path, const std::vector<std::string> &ids, const std::vector<std::string> &filters, const double *table);
void write_filter_resid(const std::string &path, const std::vector<std::string> &filters, const double *table);

// ---- filterCheck -----------------------------------------------------------------------------------
// b9_filter_loo's star_loo [n_stars][2 + 3 nf] with the catalogue's obs / sigma [n_stars][nf] -> the per-star table
// [n_stars][2 + 5 nf]: rows, member (acc[1] / acc[0]), then per filter
//   looMag = c + acc[2 + 3f] / acc[1]           (c = obs where sigma > 0, else 0: the magnitude the OTHER filters predict)
//   looSd  = sqrt(max(0, acc[3 + 3f] / acc[1] - (acc[2 + 3f] / acc[1])^2))       (the between-node spread of that prediction)
//   resid  = obs - looMag,   z = resid / sqrt(sigma^2 + looSd^2)   (the predictive z: a calibrated fit spreads it like N(0, 1)),
//   lpd    = acc[4 + 3f] / acc[1]               (the mean log predictive density);   resid, z, lpd are 0 for an unused filter.
// A star without membership weight (acc[1] == 0) has every derived value 0.
void loo_table(const double *star_loo, const double *obs, const double *sigma, long n_stars, int nf, double *table);
// b9_filter_loo's row_loo [n_rows][1 + 6 nf] -> the per-filter table [nf][kFilterCheckCols]: the number of rows with N_f > 0, then
// over those rows the mean, population sd and 16th / 50th / 84th percentiles of R_f / N_f, C_f / N_f, D_f / W_f and E_f / N_f
constexpr int kFilterCheckCols = 21;
void filter_loo_table(const double *row_loo, long n_rows, int nf, double *table);
// <base>.starFilterCheck: "id rows member {<filter>_looMag <filter>_looSd <filter>_resid <filter>_z <filter>_lpd}", one line per
// star in the order of ids; <base>.filterCheck: "filter nRows {meanZ chi2 offset lpd}_{mean sd p16 p50 p84}", one line per filter.
void write_star_filter_check(const std::string &path, const std::vector<std::string> &ids, const std::vector<std::string> &filters, const double *table);
void write_filter_check(const std::string &path, const std::vector<std::string> &filters, const double *table);

// ---- starOffsets -----------------------------------------------------------------------------------
// starOffsets.{direction, tau} (flags --direction spec, repeatable, --tau t, repeatable; in YAML one whitespace-separated
// scalar each).  A spec is `absorption` (k = the pack's absorption coefficients: more dust at the same true distance), `distance`
// (k = 1 in every filter), `filter:NAME` (a unit vector) or n_filt comma-separated values.  Default: absorption and distance.
// tau: one width (mag) for every direction or one per direction; default 0.1.  At most B9_OFF_MAX_DIRECTIONS directions.
extern const ProgramFlags kStarOffsetsFlags;
struct StarOffsetsConfig { std::vector<std::string> directions; std::vector<double> tau; };
StarOffsetsConfig star_offsets_config(const Settings &st);
// k [n_filt] of a spec; throws on an unknown name or filter or a list of another length
std::vector<double> offset_direction(const std::string &spec, const std::vector<std::string> &filters, const std::vector<double> &abs_coeff);
// b9_star_offset's star_off [n_stars][2 + 3 D] with the catalogue's sigma [n_stars][nf] and the call's k [D][nf], tau [D] -> the
// per-star table [n_stars][2 + 4 D]: rows, member (acc[1] / acc[0]), then per direction
//   mean  = acc[2 + 3j] / acc[1]                       (E[delta], mag)
//   sd    = sqrt(max(0, acc[3 + 3j] / acc[1] - mean^2) + V),   V = 1 / (sum_f (k_f / sigma_f)^2 + tau^-2) over the used filters
//   z     = mean / sd,   logBF = acc[4 + 3j] / acc[1]  (the mean log Bayes factor of an own offset against none).
// A star without membership weight (acc[1] == 0) has every derived value 0.
void offset_table(const double *star_off, const double *sigma, const double *k, const double *tau, long n_stars, int nf, int nd, double *table);
// b9_star_offset's row_off [n_rows][1 + 4 D] -> the per-direction table [D][kOffsetDistCols]: the number of rows with N > 0, then
// over those rows the mean, population sd and 16th / 50th / 84th percentiles of M1 / N, sqrt(M2 / N) and E / N
constexpr int kOffsetDistCols = 16;
void offset_dist_table(const double *row_off, long n_rows, int nd, double *table);
// <base>.starOffsets: "id rows member {<direction>_mean <direction>_sd <direction>_z <direction>_logBF}", one line per star in the
// order of ids; <base>.offsetDist: "direction nRows {mean rms logBF}_{mean sd p16 p50 p84}", one line per direction.
void write_star_offsets(const std::string &path, const std::vector<std::string> &ids, const std::vector<std::string> &directions, const double *table);
void write_offset_dist(const std::string &path, const std::vector<std::string> &directions, const double *table);

// ---- binaryStats -----------------------------------------------------------------------------------
// binaryStats.{massEdges, massBins, qMin} (flags --massEdges e0,e1,.. | --massBins N, --qMin q).  massEdges: the primary-mass
// edges as given; else massBins (default min(8, floor(128 / Q))) log-spaced bins over [0.1, max_mass], the end points exactly.
// 1 .. B9_RH_MAX_MBINS bins, bins x Q <= B9_RH_MAX_CELLS, finite strictly ascending edges, 0 <= qMin <= 1 (default 0).
extern const ProgramFlags kBinaryStatsFlags;
struct BinaryStatsConfig {
    std::vector<double> edges;               // n_mbins + 1
    double q_min;
    int n_mbins() const { return (int)edges.size() - 1; }
};
BinaryStatsConfig binary_stats_config(const Settings &st, double max_mass, int Q);
// The tables of b9_ratio_hist's outputs (DESIGN.md section 2 states the arithmetic).  A LINE is a mass bin b < n_mbins or, last, "all":
// its cells per row are cell[j] = row_cells[r][b Q + j], for "all" the bins' cells added in ascending b.  Per row N = sum_j cell[j]
// (ascending j), B = sum of the cell[j] with j >= 1 and (double)j / (double)Q >= q_min (ascending j), f = B / N.  A line's rows are
// those with member column (the last) > 0 and N > 0; the statistics are the mean, the population standard deviation and the 16th /
// 50th / 84th percentiles by mass_function_table's rule, every one 0 without such a row.
//   binary_table      -> [n_mbins + 1][kBinaryTableCols]: lo, hi (the line's edges; "all": e_0, e_last), the number of rows, the
//                        five statistics of N, the five of f
//   ratio_dist_table  -> [n_mbins + 1][Q][kRatioDistCols]: j, q = j / Q, the number of rows, the five statistics of cell[j] / N
//   star_ratio_table  b9_ratio_hist's star_cells [n_stars][n_mbins Q + 1] -> [n_stars][4 + Q]: rows = n_rows_in_grid (the call
//                        does not count rows: the caller passes the number it summed), member = total / rows, then with
//                        S_j = sum_b cell(b, j) (ascending b): inRange = (sum_j S_j) / total, pBinaryAbove = (sum of the S_j
//                        that pass q_min) / total (both ascending j), and q<j> = S_j / total = P(q = j / Q | member) for every
//                        j.  total == 0: every derived value is 0.
constexpr int kBinaryTableCols = 13, kRatioDistCols = 8;
void binary_table(const double *row_cells, long n_rows, const double *mass_edges, int n_mbins, int Q, double q_min, double *table);
void ratio_dist_table(const double *row_cells, long n_rows, int n_mbins, int Q, double *table);
void star_ratio_table(const double *star_cells, long n_stars, int n_mbins, int Q, double q_min, long n_rows_in_grid, double *table);
// <base>.binaryFraction ("bin lo hi nRows N_mean .. N_p84 f_mean .. f_p84", bin = 0 .. n_mbins - 1 then "all"), <base>.ratioDist
// ("bin j q nRows mean sd p16 p50 p84", Q lines per bin) and <base>.starRatio ("id rows member inRange pBinaryAbove q0 .. q<Q-1>",
// one line per star in the order of ids).  17 significant digits: the files read back to the tables' bits.
void write_binary_fraction(const std::string &path, const double *table, int n_mbins);
void write_ratio_dist(const std::string &path, const double *table, int n_mbins, int Q);
void write_star_ratio(const std::string &path, const std::vector<std::string> &ids, const double *table, int Q);

// ---- modelScore ------------------------------------------------------------------------------------
// b9_pointwise's acc [n_stars][8] and tail [n_stars][tail_len] (may be null: no PSIS fit is made) -> the per-star table
// [n_stars][kPointwiseCols]: rows, nInf, lppd, pWaic, elpdWaic, elpdIs, paretoK, elpdLoo, pLoo (DESIGN.md section 2 states the
// arithmetic).  With n_f = rows - nInf: lppd = VMAX + log SPOS - log rows; pWaic = M2 / (n_f - 1) (0 for n_f < 2); elpdWaic =
// lppd - pWaic; elpdIs = log n_f - (RMAX + log SNEG); paretoK / elpdLoo by Pareto-smoothed importance sampling of the tail
// (paretoK NaN and elpdLoo = elpdIs where the tail is too short to fit); pLoo = lppd - elpdLoo.  nInf > 0: elpdWaic = elpdIs =
// elpdLoo = -inf, paretoK = pLoo = +inf.  rows - nInf = 0 otherwise (rows = 0): every value 0.
constexpr int kPointwiseCols = 9;
void pointwise_table(const double *acc, const double *tail, int tail_len, long n_stars, double *table);
// over the stars with rows > 0 -> totals [kScoreTotals]: their number N, then sum and se = sqrt(N var_ddof1) of lppd, elpdWaic
// and elpdLoo, sum pWaic, sum pLoo, the stars with nInf > 0, the stars with paretoK > 0.7, the largest finite paretoK (NaN: none)
constexpr int kScoreTotals = 12;
void score_totals(const double *table, long n_stars, double *totals);
// two tables of the SAME catalogue (throws when the ids differ in content or order) -> out [kScoreCompare]: the number N of
// stars with rows > 0 in both, then sum and se = sqrt(N var_ddof1) of elpdLoo_A - elpdLoo_B, the same pair for elpdWaic, and
// the number of stars with rows > 0 in exactly one of the two tables (they take no part, and are reported)
constexpr int kScoreCompare = 6;
void score_compare(const double *table_a, const std::vector<std::string> &ids_a, const double *table_b, const std::vector<std::string> &ids_b,
                   double *out);
// <base>.pointwise ("id rows nInf lppd ... pLoo", one line per star), <base>.modelScore, <base>.modelCompare (one header line,
// one line of values) and <base>.rowLpd ("row lpd").  17 significant digits; inf / -inf / nan as printf writes them.
void write_pointwise(const std::string &path, const std::vector<std::string> &ids, const double *table);
void write_model_score(const std::string &path, const double *totals);
void write_model_compare(const std::string &path, const double *cmp);
void write_row_lpd(const std::string &path, const double *row_lpd, long n_rows);
void read_pointwise(const std::string &path, std::vector<std::string> &ids, std::vector<double> &table);

// ---- starInfluence ---------------------------------------------------------------------------------
// starInfluence.{quantity, groupFile, noGroups} (flags --quantity NAME, repeatable; --groupFile FILE; --noGroups; in YAML the
// quantities are one whitespace-separated scalar).  A quantity is a cluster parameter's name as the .res header spells it, or
// logPost; at most B9_INF_MAX_Q.  Default: every cluster parameter that varies over the main-run rows, in B9_P_* order.
extern const ProgramFlags kStarInfluenceFlags;
struct StarInfluenceConfig { std::vector<std::string> quantities; std::string group_file; bool no_groups = false; };
StarInfluenceConfig star_influence_config(const Settings &st);
// The quantities as the call takes them: q [n_rows][Q] = (theta - mean) / sd with a two-pass mean and the ddof-1 sd over the rows
// [n_rows][B9_NPARAM] (log_post [n_rows], may be null: no logPost).  Throws for an unknown name, a quantity that does not vary, more
// than B9_INF_MAX_Q of them or fewer than two rows.
struct InfluenceQuantities { std::vector<std::string> names; std::vector<double> q, mean, sd; };
InfluenceQuantities influence_quantities(const StarInfluenceConfig &c, const double *rows, const double *log_post, long n_rows);
// The groups: by default ms (stage 1) = 0 and wd (stage 3) = 1, every other star -1; with a group file its lines "id name" (names
// numbered in the order they first appear, at most B9_INF_MAX_GROUPS; a star the file does not list: -1; an unknown id throws);
// noGroups: no names, no ids.
struct InfluenceGroups { std::vector<std::string> names; std::vector<int32_t> id; };
InfluenceGroups influence_groups(const StarInfluenceConfig &c, const std::vector<std::string> &ids, const std::vector<int32_t> &stage);
// b9_star_influence's acc [n_stars][B9_INF_N(Q)] and tail (may be null) -> the per-star table [n_stars][kInfluenceHead + 3 Q]:
// rows, nInf, ess = SNEG^2 / SNEG2, paretoK (the PSIS fit of the tail; NaN without a tail or where the fit is refused), then per
// quantity shift = WQ / SNEG - MQ, lin = -CVQ / (n_f - 1) (0 for n_f < 2), looSd = sqrt(max(0, WQ2 / SNEG - (WQ / SNEG)^2)).
// nInf > 0: ess = 0, paretoK and every per-quantity value NaN.  rows = 0: every value 0.
constexpr int kInfluenceHead = 4, kGroupInfluenceHead = 5;
void influence_table(const double *acc, const double *tail, int tail_len, long n_stars, int n_q, double *table);
// b9_star_influence's group_lpd [n_rows][G] with the call's q [n_rows][Q] and the stars' ids -> [G][kGroupInfluenceHead + 3 Q]:
// nStars, rows (= n_rows), nInf (the rows whose sum is -inf: a row outside the grid is one), ess, paretoK, then per quantity
// shiftRaw (self-normalised with e^(rho - max rho), rho = -group_lpd), shift (the M largest weights replaced by the smoothed ones;
// = shiftRaw where the fit is refused) and looSd (with shift's weights).  nInf > 0: ess = 0, the rest NaN.
void group_influence_table(const double *group_lpd, long n_rows, int n_groups, const double *q, int n_q, const int32_t *group, long n_stars, double *table);
// <base>.starInfluence ("id rows nInf ess paretoK {shift_<q> lin_<q> looSd_<q>}"), <base>.groupInfluence ("group nStars rows nInf
// ess paretoK {shiftRaw_<q> shift_<q> looSd_<q>}") and <base>.influenceScale ("name mean sd").  17 significant digits.
void write_star_influence(const std::string &path, const std::vector<std::string> &ids, const std::vector<std::string> &quantities, const double *table);
void write_group_influence(const std::string &path, const std::vector<std::string> &groups, const std::vector<std::string> &quantities, const double *table);
void write_influence_scale(const std::string &path, const std::vector<std::string> &quantities, const double *mean, const double *sd);

}  // namespace b9h
