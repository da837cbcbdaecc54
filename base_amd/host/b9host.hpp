// b9host.hpp -- C++ host side above the C ABI: settings, model-pack loaders, photometry reader,
// result writer and the adaptive-MCMC driver behind the singlePopMcmc / multiPopMcmc / makeCMD
// command-line surface.
//
// The reference's sources are not mounted (/root/reference/README.md:4); names, flags and file
// formats below follow the public BASE-9 conventions as [RECALL]ed and are documented in
// docs/FORMATS.md.  Nothing here computes a likelihood: every number comes from libbase9hip.so.
#pragma once
#include "../../include/base9_hip.h"

#include <cstdint>
#include <map>
#include <functional>
#include <string>
#include <vector>

namespace b9h {

// ---- settings: "section.key" -> value, from a YAML subset plus --flag overrides -------------
class Settings {
  public:
    void load_yaml(const std::string &path);              // nested maps by indentation, scalars only
    void parse_args(int argc, char **argv);               // --key value | --key=value
    bool has(const std::string &key) const { return kv.count(key) != 0; }
    std::string str(const std::string &key, const std::string &def = "") const;
    double num(const std::string &key, double def) const;
    long integer(const std::string &key, long def) const;
    void set(const std::string &key, const std::string &value) { kv[key] = value; }
    std::string dump() const;
    // flag name ([RECALL] BASE-9 long options) -> settings key
    static const std::map<std::string, std::string> &flag_map();

  private:
    std::map<std::string, std::string> kv;
};

// ---- model pack in host memory (owns the arrays a b9_pack points to) ------------------------
struct ModelPack {
    std::vector<std::string> filters;                     // columns, in photometry order
    std::vector<double> feh, y, log_age;
    std::vector<int32_t> iso_first_eep, iso_n_eep;
    std::vector<int64_t> iso_offset;
    std::vector<double> mass, mags, abs_coeff;
    // WD cooling tracks, one per (carbonicity, mass) node in that order, each with its own age axis (ragged)
    std::vector<double> wc_carb, wc_mass, wc_log_age, wc_log_teff, wc_log_radius;   // the last three: all tracks, concatenated
    std::vector<int32_t> wc_n_age;
    std::vector<int64_t> wc_offset;
    std::vector<double> at_logg, at_log_teff, at_mags;
    int n_at_type = 0;
    int ifmr_id = B9_IFMR_WILLIAMS;
    double m_wd_up = 8.0;
    b9_pack view() const;                                 // plain-pointer view for b9_load_pack
};

// Loads <dir>/msrgb/<ms_model>.model (+ absorption.dat, wd/cooling_<wd_model>.dat,
// wd/atmos_DA.dat, wd/atmos_DB.dat when present), keeping the filter columns named in `filters`
// (in that order).  Throws std::runtime_error with a message on malformed input.
ModelPack load_model_pack(const std::string &dir, const std::string &ms_model,
                          const std::string &wd_model, const std::vector<std::string> &filters);
// The filter names a .model file provides (its %f line).
std::vector<std::string> model_filters(const std::string &dir, const std::string &ms_model);

// ---- photometry -------------------------------------------------------------------------------
struct Photometry {
    std::vector<std::string> ids, filters;
    std::vector<double> obs, sigma, mass1, mass_ratio, clust_prior;
    std::vector<int32_t> stage, wd_type, use_dbi;
    std::vector<double> filter_prior_min, filter_prior_max;
    int n_stars() const { return (int)mass1.size(); }
    b9_stars view() const;
};
// [RECALL] .phot: header "id <filters> sig<filters> mass1 massRatio stage CMprior useDBI", one
// whitespace-separated row per star; sigma < 0 marks an unused filter.  Stars outside
// [min_mag, max_mag] in filter `index` are dropped, as the reference's minMag/maxMag/index do.
Photometry read_photometry(const std::string &path, double min_mag = -1e300, double max_mag = 1e300, int index = 0);

// ---- results ------------------------------------------------------------------------------------
// [RECALL] .res: header naming the sampled columns + logPost + stage, one row per kept iteration.  [OWN] a first line
// "# <comment>" (when given) says which posterior the file holds: evaluation mode, ABI version, populations, walkers.
class ResultWriter {
  public:
    ResultWriter(const std::string &path, const std::vector<std::string> &columns, const std::string &comment = "");
    ~ResultWriter();
    void row(const std::vector<double> &values, double logpost, int stage);
  private:
    void *fp;
};

// ---- starSummary -----------------------------------------------------------------------------------
// b9_star_moments' accumulators [n_stars][B9_MOM_N] -> the derived columns [n_stars][kStarTableCols]:
//   rows = acc0, member = acc1 / acc0, mass = acc2 / acc1, massSd = sqrt(max(0, acc3 / acc1 - mass^2)), ratio and ratioSd
//   likewise from acc4, acc5, pBinary = acc6 / acc1, pPop2 = acc7 / acc1; with acc1 == 0 every derived value is 0.
// (Raw second moments in fp64 lose about 2^-52 mass^2 / var relatively: a one-node posterior comes out a few 1e-17 negative,
// hence the clamp.)  Host arithmetic only.
constexpr int kStarTableCols = 8;
void star_table(const double *acc, long n_stars, double *table);
// <base>.starSummary (docs/FORMATS.md): a header line, then one line per star in the order of `ids`:
// id rows member mass massSd massRatio massRatioSd pBinary [pPop2 -- two populations only]
void write_star_summary(const std::string &path, const std::vector<std::string> &ids, const double *acc, int n_pops);

// ---- wdSummary -------------------------------------------------------------------------------------
// b9_wd_moments' accumulators [n_wd][B9_WDM_N] -> the derived columns [n_wd][kWdTableCols]:
//   rows = ROWS, member = MEMBER / ROWS, pCooled = COOLED / MEMBER, zamsMass and zamsMassSd from M1, M1SQ over MEMBER, then a
//   mean and an sd = sqrt(max(0, E[v^2] - E[v]^2)) of wdMass, precLogAge, logCoolAge, logTeff, logg over COOLED, and
//   pPop2 = POP1 / MEMBER.  A derived column is 0 where its denominator is 0.  Host arithmetic only.
constexpr int kWdTableCols = 16;
void wd_table(const double *acc, long n_wd, double *table);
// <base>.wdSummary (docs/FORMATS.md): a header line, then one line per WD-stage star in the order of `ids`:
// id rows member pCooled zamsMass zamsMassSd wdMass wdMassSd precLogAge precLogAgeSd logCoolAge logCoolAgeSd logTeff logTeffSd
// logg loggSd [pPop2 -- two populations only]
void write_wd_summary(const std::string &path, const std::vector<std::string> &ids, const double *acc, int n_pops);

// ---- massFunction ----------------------------------------------------------------------------------
// b9_mass_hist's row_hist [n_rows][n_bins + 1] -> the per-bin table [n_bins][kMassFunctionCols]:
//   lo, hi, then over the rows whose member column (the last) is > 0 the mean, the population standard deviation and the 16th,
//   50th and 84th percentiles of the bin's expected count (linear interpolation between order statistics at (n - 1) q, numpy's
//   default), and dN/dlog10 m = mean / log10(hi / lo) (0 where lo <= 0).  No such row: every statistic is 0.  Host arithmetic only.
constexpr int kMassFunctionCols = 8;
void mass_function_table(const double *row_hist, long n_rows, const double *edges, int n_bins, double *table);
// <base>.massFunction (docs/FORMATS.md): "lo hi mean sd p16 p50 p84 dNdlogM", one line per bin
void write_mass_function(const std::string &path, const double *table, int n_bins);
// <base>.starMassHist: "id rows member bin0 .. bin<n-1>", per star its id, the rows counted, the mean membership
// acc[total] / rows and the posterior probabilities acc[b] / acc[total] (zeros without membership weight)
void write_star_mass_hist(const std::string &path, const std::vector<std::string> &ids, const double *star_hist, int n_bins, long n_rows);

// massFunction's own settings: massFunction.{nBins, minMass, maxMass, linearBins, quantity, perStar, margIsoIncrem, nMassRatios,
// nPops} (flags --nBins --minMass --maxMass --linearBins --quantity --perStar; --margIsoIncrem / --nMassRatios as sampleMass).
// Default: 24 log-spaced bins over [0.1, M_wd_up] of the primary mass.
struct MassFunctionConfig {
    int n_bins, quantity, K, Q, n_pops;
    double min_mass, max_mass;
    bool linear, per_star;
    std::vector<double> edges() const;       // n_bins + 1, strictly ascending; the end points are min_mass and max_mass exactly
};
MassFunctionConfig mass_function_config(const Settings &st, double m_wd_up);
// --minMass / --maxMass belong to simCluster in the shared flag table: massFunction's command line has them renamed to the
// flags of its own keys (--massFunctionMinMass / --massFunctionMaxMass) before Settings::parse_args sees it
std::vector<std::string> mass_function_args(int argc, char **argv);

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
// share theirs).  Nothing is carried from pass to pass.  Host arithmetic only.
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
// -> [n_stars][3 m + 3]: member, then value, lo, hi per level, passes, flags
void star_intervals_table(const StarIntervals &r, double *table);
// <base>.starIntervals (docs/FORMATS.md): "id member {q<a> q<a>_lo q<a>_hi} passes flags", one line per star in the order of ids,
// 17 significant digits
void write_star_intervals(const std::string &path, const std::vector<std::string> &ids, const std::vector<double> &levels, const double *table);
// starIntervals' own settings: starIntervals.{quantity, levels, tol, maxPasses, margIsoIncrem, nMassRatios, nPops} (flags --quantity
// --levels a,b,.. --tol --maxPasses --nPops; --margIsoIncrem / --nMassRatios as sampleMass).
struct StarIntervalsConfig {
    int quantity, K, Q, n_pops, max_passes;
    double tol;
    std::vector<double> levels;
};
StarIntervalsConfig star_intervals_config(const Settings &st);
// --quantity and --nPops belong to massFunction and simCluster in the shared flag table: they are renamed to starIntervals' own
std::vector<std::string> star_intervals_args(int argc, char **argv);

// ---- photResiduals ---------------------------------------------------------------------------------
// b9_phot_resid's star_resid [n_stars][2 + 2 nf] with the catalogue's obs / sigma [n_stars][nf] -> the per-star table
// [n_stars][2 + 4 nf]: rows, member (= acc[1] / rows), then per filter
//   predMag = c + acc[2 + 2f] / acc[1]        (c: obs where sigma > 0, else 0 -- the call's pivot)
//   predSd  = sqrt(max(0, acc[3 + 2f] / acc[1] - (acc[2 + 2f] / acc[1])^2))
//   resid   = obs - predMag                   (used filters; 0 for an unused one)
//   rmsZ    = sqrt(acc[3 + 2f] / acc[1]) / sigma   (likewise)
// Every derived value is 0 when acc[1] == 0.  Host arithmetic only.
void resid_table(const double *star_resid, const double *obs, const double *sigma, long n_stars, int nf, double *table);
// b9_phot_resid's row_resid [n_rows][1 + 5 nf] -> the per-filter table [nf][kFilterResidCols]: the number of rows with N_f > 0,
// then over those rows the mean, the population standard deviation and the 16th / 50th / 84th percentiles (mass_function_table's
// rule) of meanZ = R_f / N_f, of chi2 = C_f / N_f and of offset = D_f / W_f.  No such row: every entry 0.
constexpr int kFilterResidCols = 16;
void filter_resid_table(const double *row_resid, long n_rows, int nf, double *table);
// <base>.photResid (docs/FORMATS.md): "id rows member {<filter>_predMag <filter>_predSd <filter>_resid <filter>_rmsZ}", one line
// per star in the order of ids; <base>.filterResid: "filter nRows {meanZ chi2 offset}_{mean sd p16 p50 p84}", one line per filter.
// Numbers are written with 17 significant digits: the files read back to the tables' bits.
void write_phot_resid(const std::string &path, const std::vector<std::string> &ids, const std::vector<std::string> &filters, const double *table);
void write_filter_resid(const std::string &path, const std::vector<std::string> &filters, const double *table);

// ---- modelScore ------------------------------------------------------------------------------------
// b9_pointwise's acc [n_stars][8] and tail [n_stars][tail_len] (may be null: no PSIS fit is made) -> the per-star table
// [n_stars][kPointwiseCols]: rows, nInf, lppd, pWaic, elpdWaic, elpdIs, paretoK, elpdLoo, pLoo (DESIGN.md section 2 states the
// arithmetic).  With n_f = rows - nInf: lppd = VMAX + log SPOS - log rows; pWaic = M2 / (n_f - 1) (0 for n_f < 2); elpdWaic =
// lppd - pWaic; elpdIs = log n_f - (RMAX + log SNEG); paretoK / elpdLoo by Pareto-smoothed importance sampling of the tail
// (paretoK NaN and elpdLoo = elpdIs where the tail is too short to fit); pLoo = lppd - elpdLoo.  nInf > 0: elpdWaic = elpdIs =
// elpdLoo = -inf, paretoK = pLoo = +inf.  rows - nInf = 0 otherwise (rows = 0): every value 0.  Host arithmetic only.
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
// one line of values) and <base>.rowLpd ("row lpd"); docs/FORMATS.md.  17 significant digits; inf / -inf / nan as printf writes them.
void write_pointwise(const std::string &path, const std::vector<std::string> &ids, const double *table);
void write_model_score(const std::string &path, const double *totals);
void write_model_compare(const std::string &path, const double *cmp);
void write_row_lpd(const std::string &path, const double *row_lpd, long n_rows);
void read_pointwise(const std::string &path, std::vector<std::string> &ids, std::vector<double> &table);

const char *param_name(int idx);          // "logAge", "Y", "FeH", "modulus", "absorption", ...

}  // namespace b9h
