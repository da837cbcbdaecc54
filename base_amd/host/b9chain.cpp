// b9chain.cpp -- see b9chain.hpp.  File formats: docs/FORMATS.md.
#include "b9chain.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>
#include <stdexcept>

namespace b9h {

namespace {

[[noreturn]] void fail(const std::string &msg) { throw std::runtime_error(msg); }

// B9_HQ_* of a <section>.quantity
int quantity_id(const Settings &st, const std::string &section)
{
    const std::string q = st.str(section + ".quantity", "primary");
    if (q == "primary") return B9_HQ_PRIMARY;
    if (q == "secondary") return B9_HQ_SECONDARY;
    if (q == "system") return B9_HQ_SYSTEM;
    fail(section + ".quantity must be primary, secondary or system, not '" + q + "'");
}

ChainGrid checked(ChainGrid g)
{
    if (g.K < 1 || g.Q < 1) fail("margIsoIncrem and nMassRatios must be positive");
    return g;
}

// names, all printed with one format
std::vector<TableColumn> columns(std::initializer_list<const char *> names, const char *fmt)
{
    std::vector<TableColumn> c;
    for (const char *n : names) c.push_back({n, fmt});
    return c;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// settings
// ---------------------------------------------------------------------------------------------
int chain_n_pops(const Settings &st, const std::string &section)
{
    const long n_pops = st.integer(section + ".nPops", 1);
    if (n_pops != 1 && n_pops != 2) fail(section + ".nPops must be 1 or 2");
    return (int)n_pops;
}

ChainGrid chain_grid(const Settings &st, const std::string &section)
{
    const int n_pops = chain_n_pops(st, section);
    return checked({n_pops, (int)st.integer(section + ".margIsoIncrem", st.integer("sampleMass.margIsoIncrem", 4)),
                    (int)st.integer(section + ".nMassRatios", st.integer("sampleMass.nMassRatios", 4))});
}

ChainGrid sample_mass_grid(const Settings &st)
{
    return checked({1, (int)st.integer("sampleMass.margIsoIncrem", 4), (int)st.integer("sampleMass.nMassRatios", 4)});
}

long wd_mass_nodes(const Settings &st, const std::string &section)
{
    const long nodes = st.integer(section + ".nMassNodes", st.integer("sampleWDMass.nMassNodes", 512));
    if (nodes < 1 || nodes > 2147483647l) fail("nMassNodes must be a positive 32-bit number");
    return nodes;
}

const ProgramFlags kMassFunctionFlags = {{"minMass", "massFunctionMinMass", false}, {"maxMass", "massFunctionMaxMass", false}};
const ProgramFlags kStarIntervalsFlags = {{"quantity", "starIntervalsQuantity", false}, {"nPops", "starIntervalsNPops", false}};
const ProgramFlags kWdIntervalsFlags = {{"levels", "wdIntervalsLevels", false}, {"tol", "wdIntervalsTol", false}, {"maxPasses", "wdIntervalsMaxPasses", false},
                                        {"nMassNodes", "wdIntervalsNMassNodes", false}, {"nPops", "wdIntervalsNPops", false}};
const ProgramFlags kCmdBandFlags = {{"ratios", "cmdBandRatios", false}, {"wdNodes", "cmdBandWdNodes", false}, {"wdTypes", "cmdBandWdTypes", false},
                                    {"colours", "cmdBandColours", false}, {"levels", "cmdBandLevels", false}, {"tol", "cmdBandTol", false},
                                    {"maxPasses", "cmdBandMaxPasses", false}, {"nPops", "cmdBandNPops", false}};
const ProgramFlags kPhotResidFlags = {{"perStar", "photResidualsPerStar", true}, {"nPops", "photResidualsNPops", false}};
const ProgramFlags kFilterCheckFlags = {{"perStar", "filterCheckPerStar", true}, {"nPops", "filterCheckNPops", false}};
const ProgramFlags kStarOffsetsFlags = {{"nPops", "starOffsetsNPops", false}};
const ProgramFlags kModelScoreFlags = {{"perRow", "modelScorePerRow", true}, {"nPops", "modelScoreNPops", false}};
const ProgramFlags kStarInfluenceFlags = {{"quantity", "starInfluenceQuantity", false}, {"noGroups", "noGroups", true}, {"nPops", "starInfluenceNPops", false}};

PhotResidConfig phot_resid_config(const Settings &st) { return {st.integer("photResiduals.perStar", 0) != 0}; }

FilterCheckConfig filter_check_config(const Settings &st) { return {st.integer("filterCheck.perStar", 0) != 0}; }

ModelScoreConfig model_score_config(const Settings &st) { return {st.integer("modelScore.perRow", 0) != 0, st.str("modelScore.compareTo", "")}; }

int model_score_tail_len(long n_rows)
{
    const double s = (double)n_rows;
    return (int)std::min(256.0, std::min(std::floor(s / 5.0), std::ceil(3.0 * std::sqrt(s))) + 1.0);
}

// ---------------------------------------------------------------------------------------------
// files
// ---------------------------------------------------------------------------------------------
void write_table(const std::string &path, const char *label_name, const std::vector<std::string> *labels, const std::vector<TableColumn> &cols,
                 long n_lines, const double *values, size_t stride)
{
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) fail("cannot write " + path);
    const char *first = labels ? " " : "";                   // what stands before a line's first column
    if (labels) std::fprintf(f, "%s", label_name);
    for (size_t c = 0; c < cols.size(); ++c) std::fprintf(f, "%s%s", c ? " " : first, cols[c].name.c_str());
    std::fprintf(f, "\n");
    for (long i = 0; i < n_lines; ++i) {
        if (labels) std::fprintf(f, "%s", (*labels)[(size_t)i].c_str());
        for (size_t c = 0; c < cols.size(); ++c) {
            const char *fmt = cols[c].fmt;
            const double v = values[(size_t)i * stride + c];
            std::fputs(c ? " " : first, f);
            if (fmt[std::strlen(fmt) - 1] == 'd') std::fprintf(f, fmt, (long)v);
            else std::fprintf(f, fmt, v);
        }
        std::fprintf(f, "\n");
    }
    if (std::fclose(f) != 0) fail("cannot write " + path);
}

// ---------------------------------------------------------------------------------------------
// starSummary
// ---------------------------------------------------------------------------------------------
void star_table(const double *acc, long n_stars, double *table)
{
    for (long i = 0; i < n_stars; ++i) {
        const double *a = acc + (size_t)i * B9_MOM_N;
        double *t = table + (size_t)i * kStarTableCols;
        for (int c = 0; c < kStarTableCols; ++c) t[c] = 0.0;
        t[0] = a[B9_MOM_ROWS];
        if (a[B9_MOM_ROWS] > 0.0) t[1] = a[B9_MOM_MEMBER] / a[B9_MOM_ROWS];
        if (!(a[B9_MOM_MEMBER] > 0.0)) continue;             // no membership weight: every derived value is 0
        const double w = a[B9_MOM_MEMBER];
        t[2] = a[B9_MOM_M1] / w;
        t[3] = std::sqrt(std::max(0.0, a[B9_MOM_M1SQ] / w - t[2] * t[2]));
        t[4] = a[B9_MOM_Q] / w;
        t[5] = std::sqrt(std::max(0.0, a[B9_MOM_QSQ] / w - t[4] * t[4]));
        t[6] = a[B9_MOM_BINARY] / w;
        t[7] = a[B9_MOM_POP1] / w;
    }
}

void write_star_summary(const std::string &path, const std::vector<std::string> &ids, const double *acc, int n_pops)
{
    const long n = (long)ids.size();
    std::vector<double> table((size_t)n * kStarTableCols);
    star_table(acc, n, table.data());
    std::vector<TableColumn> cols = columns({"rows", "member", "mass", "massSd", "massRatio", "massRatioSd", "pBinary", "pPop2"}, "%.6f");
    cols[0].fmt = "%.0f";
    if (n_pops != 2) cols.pop_back();
    write_table(path, "id", &ids, cols, n, table.data(), kStarTableCols);
}

// ---------------------------------------------------------------------------------------------
// wdSummary
// ---------------------------------------------------------------------------------------------
void wd_table(const double *acc, long n_wd, double *table)
{
    for (long i = 0; i < n_wd; ++i) {
        const double *a = acc + (size_t)i * B9_WDM_N;
        double *t = table + (size_t)i * kWdTableCols;
        for (int c = 0; c < kWdTableCols; ++c) t[c] = 0.0;
        t[0] = a[B9_WDM_ROWS];
        if (a[B9_WDM_ROWS] > 0.0) t[1] = a[B9_WDM_MEMBER] / a[B9_WDM_ROWS];
        if (!(a[B9_WDM_MEMBER] > 0.0)) continue;             // no membership weight: every further value is 0
        const double w = a[B9_WDM_MEMBER], wc = a[B9_WDM_COOLED];
        t[2] = wc / w;
        t[3] = a[B9_WDM_M1] / w;
        t[4] = std::sqrt(std::max(0.0, a[B9_WDM_M1SQ] / w - t[3] * t[3]));
        t[15] = a[B9_WDM_POP1] / w;
        if (!(wc > 0.0)) continue;                           // no cooled weight: the derived values' columns are 0
        for (int q = 0; q < 5; ++q) {
            const double mean = a[B9_WDM_WDMASS + 2 * q] / wc;
            t[5 + 2 * q] = mean;
            t[6 + 2 * q] = std::sqrt(std::max(0.0, a[B9_WDM_WDMASS_SQ + 2 * q] / wc - mean * mean));
        }
    }
}

void write_wd_summary(const std::string &path, const std::vector<std::string> &ids, const double *acc, int n_pops)
{
    const long n = (long)ids.size();
    std::vector<double> table((size_t)n * kWdTableCols);
    wd_table(acc, n, table.data());
    std::vector<TableColumn> cols = columns({"rows", "member", "pCooled", "zamsMass", "zamsMassSd", "wdMass", "wdMassSd", "precLogAge", "precLogAgeSd",
                                             "logCoolAge", "logCoolAgeSd", "logTeff", "logTeffSd", "logg", "loggSd", "pPop2"}, "%.6f");
    cols[0].fmt = "%.0f";
    if (n_pops != 2) cols.pop_back();
    write_table(path, "id", &ids, cols, n, table.data(), kWdTableCols);
}

// ---------------------------------------------------------------------------------------------
// massFunction
// ---------------------------------------------------------------------------------------------
namespace {
// numpy's default percentile of an ascending sample: linear interpolation between the order statistics around (n - 1) q
double percentile_sorted(const std::vector<double> &v, double q)
{
    const double pos = (double)(v.size() - 1) * q;
    const size_t lo = (size_t)std::floor(pos), hi = std::min(lo + 1, v.size() - 1);
    const double t = pos - (double)lo;
    return v[lo] + (v[hi] - v[lo]) * t;
}
}  // namespace

void mass_function_table(const double *row_hist, long n_rows, const double *edges, int n_bins, double *table)
{
    const size_t ncol = (size_t)n_bins + 1;
    std::vector<long> use;
    for (long r = 0; r < n_rows; ++r)
        if (row_hist[(size_t)r * ncol + n_bins] > 0.0) use.push_back(r);
    std::vector<double> v(use.size());
    for (int b = 0; b < n_bins; ++b) {
        double *t = table + (size_t)b * kMassFunctionCols;
        for (int c = 0; c < kMassFunctionCols; ++c) t[c] = 0.0;
        t[0] = edges[b]; t[1] = edges[b + 1];
        if (use.empty()) continue;
        double sum = 0.0;
        for (size_t k = 0; k < use.size(); ++k) { v[k] = row_hist[(size_t)use[k] * ncol + b]; sum += v[k]; }
        const double mean = sum / (double)use.size();
        double ss = 0.0;
        for (double x : v) ss += (x - mean) * (x - mean);
        std::sort(v.begin(), v.end());
        t[2] = mean;
        t[3] = std::sqrt(ss / (double)use.size());
        t[4] = percentile_sorted(v, 0.16); t[5] = percentile_sorted(v, 0.50); t[6] = percentile_sorted(v, 0.84);
        if (edges[b] > 0.0) t[7] = mean / std::log10(edges[b + 1] / edges[b]);
    }
}

void write_mass_function(const std::string &path, const double *table, int n_bins)
{
    write_table(path, nullptr, nullptr, columns({"lo", "hi", "mean", "sd", "p16", "p50", "p84", "dNdlogM"}, "%.6f"), n_bins, table, kMassFunctionCols);
}

void write_star_mass_hist(const std::string &path, const std::vector<std::string> &ids, const double *star_hist, int n_bins, long n_rows)
{
    std::vector<TableColumn> cols = {{"rows", "%ld"}, {"member", "%.6f"}};
    for (int b = 0; b < n_bins; ++b) cols.push_back({"bin" + std::to_string(b), "%.6f"});
    const size_t ncol = (size_t)n_bins + 1, tcol = cols.size();
    std::vector<double> table(ids.size() * tcol);
    for (size_t i = 0; i < ids.size(); ++i) {
        const double *a = star_hist + i * ncol, tot = a[n_bins];
        double *t = table.data() + i * tcol;
        t[0] = (double)n_rows;
        t[1] = n_rows > 0 ? tot / (double)n_rows : 0.0;
        for (int b = 0; b < n_bins; ++b) t[2 + b] = tot > 0.0 ? a[b] / tot : 0.0;
    }
    write_table(path, "id", &ids, cols, (long)ids.size(), table.data(), tcol);
}

std::vector<double> MassFunctionConfig::edges() const
{
    std::vector<double> e((size_t)n_bins + 1);
    for (int b = 0; b <= n_bins; ++b) {
        const double t = (double)b / (double)n_bins;
        e[b] = linear ? min_mass + (max_mass - min_mass) * t : min_mass * std::pow(max_mass / min_mass, t);
    }
    e[0] = min_mass; e[n_bins] = max_mass;
    for (int b = 0; b < n_bins; ++b)
        if (!(e[b + 1] > e[b])) fail("massFunction: the bins are too narrow to tell their edges apart");
    return e;
}

MassFunctionConfig mass_function_config(const Settings &st, double m_wd_up)
{
    MassFunctionConfig c;
    c.n_bins = (int)st.integer("massFunction.nBins", 24);
    c.min_mass = st.num("massFunction.minMass", 0.1);
    c.max_mass = st.num("massFunction.maxMass", m_wd_up);
    c.linear = st.integer("massFunction.linearBins", 0) != 0;
    c.per_star = st.integer("massFunction.perStar", 0) != 0;
    c.quantity = quantity_id(st, "massFunction");
    if (c.n_bins < 1 || c.n_bins > B9_HIST_MAX_BINS) fail("massFunction.nBins must lie in 1 .. " + std::to_string(B9_HIST_MAX_BINS));
    if (!std::isfinite(c.min_mass) || !std::isfinite(c.max_mass) || !(c.max_mass > c.min_mass)) fail("massFunction: maxMass must exceed minMass");
    if (!c.linear && !(c.min_mass > 0.0)) fail("massFunction: log-spaced bins need minMass > 0 (or --linearBins)");
    return c;
}

// ---------------------------------------------------------------------------------------------
// starIntervals
// ---------------------------------------------------------------------------------------------
namespace {
void check_levels(const double *levels, int m, int n_bins, const char *who)
{
    if (m < 1 || 3 * m > n_bins + 1) fail(std::string(who) + ": the levels need 3 edges each: at most (n_bins + 1) / 3 of them, at least one");
    for (int l = 0; l < m; ++l)
        if (!(levels[l] > 0.0 && levels[l] < 1.0) || (l > 0 && !(levels[l] > levels[l - 1])))
            fail(std::string(who) + ": the levels must lie strictly inside (0, 1) and ascend strictly");
}
}  // namespace

void refine_star_edges(const double *edges, const double *acc, long n_stars, int n_bins, const double *levels, int n_levels, double tol,
                       double *lo, double *hi, double *below, double *inside, double *value, int32_t *is_final, int32_t *flags, double *next_edges)
{
    const int B = n_bins, m = n_levels;
    if (B < 1) fail("refine_star_edges: n_bins must be positive");
    check_levels(levels, m, B, "refine_star_edges");
    if (!(tol >= 0.0)) fail("refine_star_edges: tol must not be negative");
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> cum((size_t)B + 2), pts, out;
    std::vector<int> col(m);
    for (long i = 0; i < n_stars; ++i) {
        const double *e = edges + (size_t)i * (B + 1), *a = acc + (size_t)i * (B + 3);
        double *ne = next_edges + (size_t)i * (B + 1);
        std::copy(e, e + B + 1, ne);                         // a finished star keeps its edges
        // the counted mass: below, the bins, at or above, summed in that order (the total column may hold more: B9_HQ_SECONDARY)
        double c = 0.0;
        for (int k = 0; k < B + 2; ++k) { c = c + a[k]; cum[k] = c; }
        const double C = cum[B + 1];
        flags[i] = 0;
        if (!(C > 0.0)) {
            flags[i] = kSivNoMass;
            for (int l = 0; l < m; ++l) {
                const size_t o = (size_t)i * m + l;
                lo[o] = hi[o] = value[o] = nan; below[o] = inside[o] = 0.0; is_final[o] = 1;
            }
            continue;
        }
        auto col_final = [&](int k) {
            if (k < 1 || k > B) return false;
            const double L = e[k - 1], H = e[k];
            return H - L <= tol * std::max(std::fabs(L), std::fabs(H)) || H == std::nextafter(L, inf);
        };
        bool open = false;
        for (int l = 0; l < m; ++l) {
            const size_t o = (size_t)i * m + l;
            const double target = levels[l] * C;
            // the column in which the cumulative sum first reaches the level -- within kSivSlack C, the rounding of the sums: a
            // level that falls exactly between two nodes (whole rows on either side: 17 of 34 at the median) is a tie that rounding
            // would decide one way in one pass and the other way in the next; with the slack every pass takes the lower node
            int k = 0;
            while (k < B + 1 && !(cum[k] >= target - kSivSlack * C)) ++k;
            col[l] = k;
            lo[o] = k == 0 ? -inf : e[k - 1];
            hi[o] = k == B + 1 ? inf : e[k];
            below[o] = k == 0 ? 0.0 : cum[k - 1];
            inside[o] = a[k];
            is_final[o] = col_final(k);
            open = open || !is_final[o];
            if (k == 0) value[o] = e[0];
            else if (k == B + 1) value[o] = e[B];
            else {
                const double t = a[k] > 0.0 ? std::min(1.0, std::max(0.0, (target - below[o]) / a[k])) : 0.0;
                value[o] = std::min(hi[o], std::max(lo[o], lo[o] + (hi[o] - lo[o]) * t));
            }
        }
        if (!open) continue;
        flags[i] = kSivOpen;
        // the next pass's edges: every distinct bracket keeps its two ends (an open one is widened to twice the range), the
        // unfinished ones share the remaining edges evenly as interior points
        const double range = e[B] - e[0];
        struct Iv { double L, H; bool todo; int extra; };
        std::vector<Iv> iv;
        for (int l = 0; l < m; ++l) {
            if (l > 0 && col[l] == col[l - 1]) continue;    // coinciding brackets share their sub-bins
            const int k = col[l];
            if (k == 0) iv.push_back({e[0] - 2.0 * range, e[0], true, 0});
            else if (k == B + 1) iv.push_back({e[B], e[B] + 2.0 * range, true, 0});
            else iv.push_back({e[k - 1], e[k], !col_final(k), 0});
        }
        int mandatory = 0, todo = 0;
        for (size_t j = 0; j < iv.size(); ++j) {
            mandatory += (j > 0 && iv[j].L == iv[j - 1].H) ? 1 : 2;
            todo += iv[j].todo;
        }
        int spare = B + 1 - mandatory;
        if (spare < todo) fail("refine_star_edges: too few bins for the levels");
        for (int j = 0, t = 0; j < (int)iv.size(); ++j)
            if (iv[j].todo) { iv[j].extra = spare / todo + (t < spare % todo); ++t; }
        out.clear();
        int left_over = 0;
        for (size_t j = 0; j < iv.size(); ++j) {
            if (out.empty() || out.back() != iv[j].L) out.push_back(iv[j].L);
            const int q = iv[j].extra;
            for (int s = 1; s <= q; ++s) {
                double x = iv[j].L + (iv[j].H - iv[j].L) * ((double)s / (double)(q + 1));
                if (!(x > out.back())) x = std::nextafter(out.back(), inf);
                if (!(x < iv[j].H)) { left_over += q - s + 1; break; }      // no double left inside the bracket
                out.push_back(x);
            }
            out.push_back(iv[j].H);
        }
        // (edges a bracket could not take go above the top one, a range apart: they cut nothing that matters)
        for (int s = 0; s < left_over; ++s) out.push_back(out.back() + std::max(range, std::fabs(out.back())));
        if ((int)out.size() != B + 1) fail("refine_star_edges: internal error: edge count");
        for (int b = 0; b <= B; ++b) {
            if (!std::isfinite(out[b]) || (b > 0 && !(out[b] > out[b - 1]))) fail("refine_star_edges: the next edges of star " + std::to_string(i) + " do not ascend");
            ne[b] = out[b];
        }
    }
}

StarIntervals interval_loop(const StarBinsFn &bins, long n_lines, long n_rows, int n_bins, const double *first_lo, const double *first_hi,
                            const std::vector<double> &levels, double tol, int max_passes, std::vector<double> *counted)
{
    const int B = n_bins, m = (int)levels.size();
    const long n_stars = n_lines;
    check_levels(levels.data(), m, B, "interval_loop");
    if (max_passes < 1) fail("interval_loop: maxPasses must be positive");
    StarIntervals r;
    r.n_levels = m; r.n_stars = n_stars;
    const size_t nm = (size_t)n_stars * m;
    r.member.assign(n_stars, 0.0); r.value.assign(nm, 0.0); r.lo.assign(nm, 0.0); r.hi.assign(nm, 0.0);
    r.is_final.assign(nm, 0); r.passes.assign(n_stars, 0); r.flags.assign(n_stars, 0);
    std::vector<double> edges((size_t)n_stars * (B + 1)), next(edges.size()), acc((size_t)n_stars * (B + 3)), below(nm), inside(nm);
    for (long i = 0; i < n_stars; ++i) {
        const double lo = first_lo[i], hi = first_hi[i];
        if (!std::isfinite(lo) || !std::isfinite(hi) || !(hi > lo)) fail("interval_loop: line " + std::to_string(i) + ": the first range must be finite and not empty");
        for (int b = 0; b <= B; ++b) edges[(size_t)i * (B + 1) + b] = lo + (hi - lo) * ((double)b / (double)B);
        for (int b = 1; b <= B; ++b)
            if (!(edges[(size_t)i * (B + 1) + b] > edges[(size_t)i * (B + 1) + b - 1])) fail("interval_loop: line " + std::to_string(i) + ": the first range is too narrow to cut");
    }
    for (int pass = 1; pass <= max_passes; ++pass) {
        bins(edges.data(), B, acc.data());
        refine_star_edges(edges.data(), acc.data(), n_stars, B, levels.data(), m, tol, r.lo.data(), r.hi.data(), below.data(), inside.data(), r.value.data(),
                          r.is_final.data(), r.flags.data(), next.data());
        bool all = true;
        for (long i = 0; i < n_stars; ++i) {
            const bool done = !(r.flags[i] & kSivOpen);
            if (r.passes[i] == 0 && (done || pass == max_passes)) r.passes[i] = pass;
            all = all && done;
            r.member[i] = n_rows > 0 ? acc[(size_t)i * (B + 3) + B + 2] / (double)n_rows : 0.0;
        }
        if (all) break;
        edges.swap(next);
    }
    if (counted) {
        counted->assign(n_stars, 0.0);
        for (long i = 0; i < n_stars; ++i) {
            const double *a = acc.data() + (size_t)i * (B + 3);
            double c = 0.0;
            for (int k = 0; k < B + 2; ++k) c = c + a[k];       // (refine_star_edges' order)
            if (a[B + 2] > 0.0) (*counted)[i] = c / a[B + 2];
        }
    }
    return r;
}

StarIntervals star_intervals(const StarBinsFn &bins, long n_stars, long n_rows, int n_bins, double max_mass, const std::vector<double> &levels, double tol,
                             int max_passes)
{
    check_levels(levels.data(), (int)levels.size(), n_bins, "star_intervals");
    if (max_passes < 1) fail("star_intervals: maxPasses must be positive");
    if (!(max_mass > 0.0) || !std::isfinite(max_mass)) fail("star_intervals: the largest mass must be positive");
    // (0 + (2 max_mass - 0) (b / B) is (2 max_mass) (b / B) bit for bit)
    const std::vector<double> lo(n_stars, 0.0), hi(n_stars, 2.0 * max_mass);
    return interval_loop(bins, n_stars, n_rows, n_bins, lo.data(), hi.data(), levels, tol, max_passes);
}

void star_intervals_table(const StarIntervals &r, double *table)
{
    const int m = r.n_levels;
    const size_t tcol = 3 * (size_t)m + 3;
    for (long i = 0; i < r.n_stars; ++i) {
        double *t = table + (size_t)i * tcol;
        t[0] = r.member[i];
        for (int l = 0; l < m; ++l) {
            const size_t o = (size_t)i * m + l;
            t[1 + 3 * l] = r.value[o]; t[2 + 3 * l] = r.lo[o]; t[3 + 3 * l] = r.hi[o];
        }
        t[tcol - 2] = (double)r.passes[i]; t[tcol - 1] = (double)r.flags[i];
    }
}

void write_star_intervals(const std::string &path, const std::vector<std::string> &ids, const std::vector<double> &levels, const double *table)
{
    std::vector<TableColumn> cols = {{"member", "%.17g"}};
    for (double a : levels) {
        char q[40];
        std::snprintf(q, sizeof q, "q%.12g", a);
        for (const char *end : {"", "_lo", "_hi"}) cols.push_back({std::string(q) + end, "%.17g"});
    }
    cols.push_back({"passes", "%.0f"});
    cols.push_back({"flags", "%.0f"});
    write_table(path, "id", &ids, cols, (long)ids.size(), table, cols.size());
}

namespace {
// "a,b,.." or "[a, b, ..]" -> the numbers
std::vector<double> parse_levels(const Settings &st, const std::string &key)
{
    std::vector<double> levels;
    std::string lv = st.str(key, "0.025,0.16,0.5,0.84,0.975");
    for (char &ch : lv) if (ch == ',' || ch == '[' || ch == ']') ch = ' ';
    std::istringstream ls(lv);
    std::string tok;
    while (ls >> tok) {
        char *end = nullptr;
        const double v = std::strtod(tok.c_str(), &end);
        if (end == tok.c_str() || *end) fail(key + ": '" + tok + "' is not a number");
        levels.push_back(v);
    }
    return levels;
}
}  // namespace

StarIntervalsConfig star_intervals_config(const Settings &st)
{
    StarIntervalsConfig c;
    c.quantity = quantity_id(st, "starIntervals");
    c.levels = parse_levels(st, "starIntervals.levels");
    c.tol = st.num("starIntervals.tol", 1e-4);
    c.max_passes = (int)st.integer("starIntervals.maxPasses", 12);
    check_levels(c.levels.data(), (int)c.levels.size(), B9_SBIN_MAX_BINS, "starIntervals.levels");
    if (!(c.tol >= 0.0)) fail("starIntervals.tol must not be negative");
    if (c.max_passes < 1) fail("starIntervals.maxPasses must be positive");
    return c;
}

// ---------------------------------------------------------------------------------------------
// wdIntervals
// ---------------------------------------------------------------------------------------------
const char *const kWdQuantityNames[B9_WQ_N] = {"zamsMass", "wdMass", "precLogAge", "logCoolAge", "logTeff", "logg"};

WdIntervalsConfig wd_intervals_config(const Settings &st)
{
    WdIntervalsConfig c;
    c.quantity_mask = 0;
    std::string qs = st.str("wdIntervals.quantities", "zamsMass,wdMass,precLogAge,logCoolAge,logTeff,logg");
    for (char &ch : qs) if (ch == ',' || ch == '[' || ch == ']') ch = ' ';
    std::istringstream is(qs);
    std::string tok;
    while (is >> tok) {
        int q = 0;
        while (q < B9_WQ_N && tok != kWdQuantityNames[q]) ++q;
        if (q == B9_WQ_N) fail("wdIntervals.quantities: '" + tok + "' is none of zamsMass, wdMass, precLogAge, logCoolAge, logTeff, logg");
        c.quantity_mask |= 1 << q;
    }
    if (c.quantity_mask == 0) fail("wdIntervals.quantities: at least one quantity");
    c.levels = parse_levels(st, "wdIntervals.levels");
    c.tol = st.num("wdIntervals.tol", 1e-4);
    c.max_passes = (int)st.integer("wdIntervals.maxPasses", 12);
    c.n_nodes = st.integer("wdIntervals.nMassNodes", st.integer("wdSummary.nMassNodes", st.integer("sampleWDMass.nMassNodes", 512)));
    check_levels(c.levels.data(), (int)c.levels.size(), B9_WBIN_MAX_BINS, "wdIntervals.levels");
    if (!(c.tol >= 0.0)) fail("wdIntervals.tol must not be negative");
    if (c.max_passes < 1) fail("wdIntervals.maxPasses must be positive");
    if (c.n_nodes < 1 || c.n_nodes > 2147483647l) fail("nMassNodes must be a positive 32-bit number");
    return c;
}

void wd_first_ranges(const double *wd_acc, long n_wd, int quantity_mask, double *first_lo, double *first_hi)
{
    if (quantity_mask < 1 || quantity_mask >= (1 << B9_WQ_N)) fail("wd_first_ranges: the quantity mask selects nothing, or something unknown");
    size_t o = 0;
    for (long i = 0; i < n_wd; ++i) {
        const double *a = wd_acc + (size_t)i * B9_WDM_N;
        for (int q = 0; q < B9_WQ_N; ++q) {
            if (!(quantity_mask >> q & 1)) continue;
            const double w = q == B9_WQ_ZAMS ? a[B9_WDM_MEMBER] : a[B9_WDM_COOLED];
            const double s1 = q == B9_WQ_ZAMS ? a[B9_WDM_M1] : a[B9_WDM_WDMASS + 2 * (q - 1)];
            const double s2 = q == B9_WQ_ZAMS ? a[B9_WDM_M1SQ] : a[B9_WDM_WDMASS_SQ + 2 * (q - 1)];
            double lo = 0.0, hi = 1.0;
            if (w > 0.0) {
                const double mean = s1 / w, sd = std::sqrt(std::max(0.0, s2 / w - mean * mean));
                double half = std::max(6.0 * sd, 1e-3 * std::fabs(mean));
                if (!(half > 0.0) || !std::isfinite(half)) half = 1.0;
                if (std::isfinite(mean)) { lo = mean - half; hi = mean + half; }
            }
            first_lo[o] = lo; first_hi[o] = hi;
            ++o;
        }
    }
}

WdIntervals wd_intervals(const WdMomentsFn &moments, const StarBinsFn &bins, long n_wd, long n_rows, int quantity_mask, const std::vector<double> &levels,
                         double tol, int max_passes)
{
    WdIntervals r;
    r.n_wd = n_wd; r.n_sel = __builtin_popcount((unsigned)quantity_mask);
    const long n_lines = n_wd * r.n_sel;
    std::vector<double> wd_acc((size_t)n_wd * B9_WDM_N, 0.0), lo(n_lines), hi(n_lines);
    moments(wd_acc.data());
    wd_first_ranges(wd_acc.data(), n_wd, quantity_mask, lo.data(), hi.data());
    r.lines = interval_loop(bins, n_lines, n_rows, B9_WBIN_MAX_BINS, lo.data(), hi.data(), levels, tol, max_passes, &r.counted);
    return r;
}

void wd_intervals_table(long n_wd, int n_sel, int n_levels, const double *member, const double *counted, const double *value, const double *lo,
                        const double *hi, const int32_t *passes, const int32_t *flags, double *table)
{
    const int m = n_levels;
    const size_t per = 3 * (size_t)m + 3, tcol = 1 + (size_t)n_sel * per;
    for (long i = 0; i < n_wd; ++i) {
        double *t = table + (size_t)i * tcol;
        t[0] = member[(size_t)i * n_sel];
        for (int s = 0; s < n_sel; ++s) {
            const size_t line = (size_t)i * n_sel + s;
            double *ts = t + 1 + (size_t)s * per;
            ts[0] = counted[line];
            for (int l = 0; l < m; ++l) {
                const size_t o = line * m + l;
                ts[1 + 3 * l] = value[o]; ts[2 + 3 * l] = lo[o]; ts[3 + 3 * l] = hi[o];
            }
            ts[per - 2] = (double)passes[line]; ts[per - 1] = (double)flags[line];
        }
    }
}

void wd_intervals_table(const WdIntervals &r, double *table)
{
    const StarIntervals &l = r.lines;
    wd_intervals_table(r.n_wd, r.n_sel, l.n_levels, l.member.data(), r.counted.data(), l.value.data(), l.lo.data(), l.hi.data(), l.passes.data(),
                       l.flags.data(), table);
}

void write_wd_intervals(const std::string &path, const std::vector<std::string> &ids, int quantity_mask, const std::vector<double> &levels,
                        const double *table)
{
    std::vector<TableColumn> cols = {{"member", "%.17g"}};
    for (int q = 0; q < B9_WQ_N; ++q) {
        if (!(quantity_mask >> q & 1)) continue;
        const std::string n = kWdQuantityNames[q];
        cols.push_back({n + "_counted", "%.17g"});
        for (double a : levels) {
            char lv[40];
            std::snprintf(lv, sizeof lv, "q%.12g", a);
            for (const char *end : {"", "_lo", "_hi"}) cols.push_back({n + "_" + lv + end, "%.17g"});
        }
        cols.push_back({n + "_passes", "%.0f"});
        cols.push_back({n + "_flags", "%.0f"});
    }
    write_table(path, "id", &ids, cols, (long)ids.size(), table, cols.size());
}

// ---------------------------------------------------------------------------------------------
// cmdBand
// ---------------------------------------------------------------------------------------------
CmdBandConfig cmd_band_config(const Settings &st)
{
    CmdBandConfig c;
    {
        std::string rs = st.str("cmdBand.ratios", "0,1");
        for (char &ch : rs) if (ch == ',' || ch == '[' || ch == ']') ch = ' ';
        std::istringstream is(rs);
        std::string tok;
        while (is >> tok) {
            char *end = nullptr;
            const double v = std::strtod(tok.c_str(), &end);
            if (end == tok.c_str() || *end) fail("cmdBand.ratios: '" + tok + "' is not a number");
            if (!std::isfinite(v) || v < 0.0 || v > 1.0) fail("cmdBand.ratios: a mass ratio lies in [0, 1]");
            c.ratios.push_back(v);
        }
        if (c.ratios.size() > B9_BAND_MAX_RATIOS) fail("cmdBand.ratios: at most " + std::to_string(B9_BAND_MAX_RATIOS) + " loci");
    }
    c.wd_nodes = st.integer("cmdBand.wdNodes", 256);
    if (c.wd_nodes < 0 || c.wd_nodes > 2147483647l) fail("cmdBand.wdNodes must be a 32-bit number that is not negative");
    {
        std::string t = st.str("cmdBand.wdTypes", "da");
        std::transform(t.begin(), t.end(), t.begin(), ::tolower);
        c.wd_types = t == "da" ? 1 : (t == "db" ? 2 : (t == "both" ? 3 : 0));
        if (!c.wd_types) fail("cmdBand.wdTypes must be da, db or both");
    }
    {
        std::string cs = st.str("cmdBand.colours", "");
        for (char &ch : cs) if (ch == ',' || ch == '[' || ch == ']') ch = ' ';
        std::istringstream is(cs);
        std::string tok;
        while (is >> tok) {
            const size_t dash = tok.find('-');
            if (dash == std::string::npos || dash == 0 || dash + 1 == tok.size()) fail("cmdBand.colours: '" + tok + "' is not <filter>-<filter>");
            c.colours.emplace_back(tok.substr(0, dash), tok.substr(dash + 1));
        }
        if (c.colours.size() > B9_BAND_MAX_COLOURS) fail("cmdBand.colours: at most " + std::to_string(B9_BAND_MAX_COLOURS) + " colours");
    }
    c.levels = parse_levels(st, "cmdBand.levels");
    c.tol = st.num("cmdBand.tol", 1e-4);
    c.max_passes = (int)st.integer("cmdBand.maxPasses", 12);
    check_levels(c.levels.data(), (int)c.levels.size(), B9_BAND_MAX_BINS, "cmdBand.levels");
    if (!(c.tol >= 0.0)) fail("cmdBand.tol must not be negative");
    if (c.max_passes < 1) fail("cmdBand.maxPasses must be positive");
    if (c.ratios.empty() && c.wd_nodes == 0) fail("cmdBand: no ratios and no WD nodes: nothing to do");
    return c;
}

std::vector<int32_t> band_colour_ids(const CmdBandConfig &c, const std::vector<std::string> &filters)
{
    std::vector<int32_t> ids;
    for (const auto &col : c.colours) {
        for (const std::string &name : {col.first, col.second}) {
            const auto it = std::find(filters.begin(), filters.end(), name);
            if (it == filters.end()) fail("cmdBand.colours: '" + name + "' is not a filter of the model set");
            ids.push_back((int32_t)(it - filters.begin()));
        }
        if (ids[ids.size() - 1] == ids[ids.size() - 2]) fail("cmdBand.colours: '" + col.first + "-" + col.second + "' takes one filter twice");
    }
    return ids;
}

std::vector<std::string> band_line_names(int n_pops, int eep0, int n_eep, int n_ratio, long wd_nodes, int wd_types, const std::vector<std::string> &filters,
                                         const std::vector<int32_t> &colour_ids)
{
    std::vector<std::string> cols = {"mass"};
    for (const std::string &f : filters) cols.push_back(f);
    for (size_t c = 0; c + 1 < colour_ids.size(); c += 2) cols.push_back(filters[(size_t)colour_ids[c]] + "-" + filters[(size_t)colour_ids[c + 1]]);
    std::vector<std::string> names;
    for (int k = 0; k < n_pops; ++k) {
        const std::string pop = "p" + std::to_string(k) + ".";
        for (int s = 0; s < n_ratio; ++s)
            for (int e = 0; e < n_eep; ++e)
                for (const std::string &c : cols) names.push_back(pop + "q" + std::to_string(s) + ".eep" + std::to_string(eep0 + e) + "." + c);
        for (int t = 0; t < 2; ++t) {
            if (wd_nodes < 1 || !(wd_types >> t & 1)) continue;
            for (long j = 1; j <= wd_nodes; ++j)
                for (const std::string &c : cols) names.push_back(pop + (t ? "db" : "da") + ".n" + std::to_string(j) + "." + c);
        }
    }
    return names;
}

void band_first_ranges(const double *mom, long n_lines, double *first_lo, double *first_hi)
{
    for (long l = 0; l < n_lines; ++l) {
        const double *m = mom + (size_t)l * B9_BAND_NMOM;
        double lo = 0.0, hi = 1.0;
        if (m[B9_BAND_N] > 0.0 && std::isfinite(m[B9_BAND_MIN]) && std::isfinite(m[B9_BAND_MAX])) {
            const double mn = m[B9_BAND_MIN], mx = m[B9_BAND_MAX];
            const double pad = std::max(0.01 * (mx - mn), 1e-6 * std::max({1.0, std::fabs(mn), std::fabs(mx)}));
            lo = mn - pad; hi = mx + pad;
        }
        first_lo[l] = lo; first_hi[l] = hi;
    }
}

void band_first_edges(const double *mom, long n_lines, int n_bins, double *edges)
{
    if (n_bins < 1 || n_bins > B9_BAND_MAX_BINS) fail("band_first_edges: n_bins must lie in 1 .. B9_BAND_MAX_BINS");
    std::vector<double> lo(n_lines), hi(n_lines);
    band_first_ranges(mom, n_lines, lo.data(), hi.data());
    for (long l = 0; l < n_lines; ++l)       // (interval_loop's cut)
        for (int b = 0; b <= n_bins; ++b) edges[(size_t)l * (n_bins + 1) + b] = lo[l] + (hi[l] - lo[l]) * ((double)b / (double)n_bins);
}

CmdBand cmd_band(const BandMomentsFn &moments, const StarBinsFn &bins, long n_lines, long n_rows, const std::vector<double> &levels, double tol, int max_passes)
{
    CmdBand r;
    r.n_lines = n_lines;
    r.mom.assign((size_t)n_lines * B9_BAND_NMOM, 0.0);
    std::vector<double> lo(n_lines), hi(n_lines);
    moments(r.mom.data());
    band_first_ranges(r.mom.data(), n_lines, lo.data(), hi.data());
    r.lines = interval_loop(bins, n_lines, n_rows, B9_BAND_MAX_BINS, lo.data(), hi.data(), levels, tol, max_passes);
    return r;
}

void band_table(const double *mom, const double *pivot, long n_lines, int n_levels, const double *value, const double *lo, const double *hi,
                const int32_t *passes, const int32_t *flags, double *table)
{
    const int m = n_levels;
    const size_t tcol = 5 + 3 * (size_t)m + 2;
    for (long l = 0; l < n_lines; ++l) {
        const double *a = mom + (size_t)l * B9_BAND_NMOM;
        double *t = table + (size_t)l * tcol;
        const double n = a[B9_BAND_N];
        t[0] = n; t[1] = t[2] = std::nan(""); t[3] = a[B9_BAND_MIN]; t[4] = a[B9_BAND_MAX];
        if (n > 0.0) {
            const double d = a[B9_BAND_SUM] / n;
            t[1] = (pivot ? pivot[l] : 0.0) + d;
            t[2] = std::sqrt(std::max(0.0, a[B9_BAND_SUMSQ] / n - d * d));
        }
        for (int k = 0; k < m; ++k) {
            const size_t o = (size_t)l * m + k;
            t[5 + 3 * k] = value[o]; t[6 + 3 * k] = lo[o]; t[7 + 3 * k] = hi[o];
        }
        t[tcol - 2] = (double)passes[l]; t[tcol - 1] = (double)flags[l];
    }
}

void write_cmd_band(const std::string &path, const std::vector<std::string> &names, const std::vector<double> &levels, const double *table)
{
    std::vector<TableColumn> cols = {{"N", "%.0f"}, {"mean", "%.17g"}, {"sd", "%.17g"}, {"min", "%.17g"}, {"max", "%.17g"}};
    for (double a : levels) {
        char q[40];
        std::snprintf(q, sizeof q, "q%.12g", a);
        for (const char *end : {"", "_lo", "_hi"}) cols.push_back({std::string(q) + end, "%.17g"});
    }
    cols.push_back({"passes", "%.0f"});
    cols.push_back({"flags", "%.0f"});
    write_table(path, "line", &names, cols, (long)names.size(), table, cols.size());
}

// ---------------------------------------------------------------------------------------------
// photResiduals
// ---------------------------------------------------------------------------------------------
void resid_table(const double *star_resid, const double *obs, const double *sigma, long n_stars, int nf, double *table)
{
    const size_t ncol = 2 + 2 * (size_t)nf, tcol = 2 + 4 * (size_t)nf;
    for (long i = 0; i < n_stars; ++i) {
        const double *a = star_resid + (size_t)i * ncol;
        double *t = table + (size_t)i * tcol;
        for (size_t c = 0; c < tcol; ++c) t[c] = 0.0;
        t[0] = a[0];
        if (a[0] > 0.0) t[1] = a[1] / a[0];
        if (!(a[1] > 0.0)) continue;                         // no membership weight: every derived value is 0
        for (int f = 0; f < nf; ++f) {
            const double sg = sigma[(size_t)i * nf + f], o = obs[(size_t)i * nf + f];
            const bool used = sg > 0.0;
            const double m1 = a[2 + 2 * f] / a[1], m2 = a[3 + 2 * f] / a[1];
            double *tf = t + 2 + 4 * (size_t)f;
            tf[0] = (used ? o : 0.0) + m1;
            tf[1] = std::sqrt(std::max(0.0, m2 - m1 * m1));
            if (used) { tf[2] = o - tf[0]; tf[3] = std::sqrt(m2) / sg; }
        }
    }
}

void filter_resid_table(const double *row_resid, long n_rows, int nf, double *table)
{
    const size_t ncol = 1 + 5 * (size_t)nf;
    std::vector<double> v;
    for (int f = 0; f < nf; ++f) {
        double *t = table + (size_t)f * kFilterResidCols;
        for (int c = 0; c < kFilterResidCols; ++c) t[c] = 0.0;
        std::vector<long> use;
        for (long r = 0; r < n_rows; ++r)
            if (row_resid[(size_t)r * ncol + 1 + 5 * f] > 0.0) use.push_back(r);
        t[0] = (double)use.size();
        if (use.empty()) continue;
        for (int q = 0; q < 3; ++q) {
            v.resize(use.size());
            double sum = 0.0;
            for (size_t k = 0; k < use.size(); ++k) {
                const double *x = row_resid + (size_t)use[k] * ncol + 1 + 5 * f;          // N, R, C, W, D
                v[k] = q == 0 ? x[1] / x[0] : q == 1 ? x[2] / x[0] : (x[3] > 0.0 ? x[4] / x[3] : 0.0);
                sum += v[k];
            }
            const double mean = sum / (double)use.size();
            double ss = 0.0;
            for (double x : v) ss += (x - mean) * (x - mean);
            std::sort(v.begin(), v.end());
            double *tq = t + 1 + 5 * q;
            tq[0] = mean;
            tq[1] = std::sqrt(ss / (double)use.size());
            tq[2] = percentile_sorted(v, 0.16); tq[3] = percentile_sorted(v, 0.50); tq[4] = percentile_sorted(v, 0.84);
        }
    }
}

void write_phot_resid(const std::string &path, const std::vector<std::string> &ids, const std::vector<std::string> &filters, const double *table)
{
    std::vector<TableColumn> cols = columns({"rows", "member"}, "%.17g");
    for (const std::string &n : filters)
        for (const char *what : {"_predMag", "_predSd", "_resid", "_rmsZ"}) cols.push_back({n + what, "%.17g"});
    write_table(path, "id", &ids, cols, (long)ids.size(), table, cols.size());
}

void write_filter_resid(const std::string &path, const std::vector<std::string> &filters, const double *table)
{
    std::vector<TableColumn> cols = {{"nRows", "%.17g"}};
    for (const char *q : {"meanZ", "chi2", "offset"})
        for (const char *s : {"mean", "sd", "p16", "p50", "p84"}) cols.push_back({std::string(q) + "_" + s, "%.17g"});
    write_table(path, "filter", &filters, cols, (long)filters.size(), table, kFilterResidCols);
}

// ---------------------------------------------------------------------------------------------
// filterCheck
// ---------------------------------------------------------------------------------------------
void loo_table(const double *star_loo, const double *obs, const double *sigma, long n_stars, int nf, double *table)
{
    const size_t ncol = 2 + 3 * (size_t)nf, tcol = 2 + 5 * (size_t)nf;
    for (long i = 0; i < n_stars; ++i) {
        const double *a = star_loo + (size_t)i * ncol;
        double *t = table + (size_t)i * tcol;
        for (size_t c = 0; c < tcol; ++c) t[c] = 0.0;
        t[0] = a[0];
        if (a[0] > 0.0) t[1] = a[1] / a[0];
        if (!(a[1] > 0.0)) continue;                         // no membership weight: every derived value is 0
        for (int f = 0; f < nf; ++f) {
            const double sg = sigma[(size_t)i * nf + f], o = obs[(size_t)i * nf + f];
            const bool used = sg > 0.0;
            const double m1 = a[2 + 3 * f] / a[1], m2 = a[3 + 3 * f] / a[1], var = std::max(0.0, m2 - m1 * m1);
            double *tf = t + 2 + 5 * (size_t)f;
            tf[0] = (used ? o : 0.0) + m1;
            tf[1] = std::sqrt(var);
            if (used) { tf[2] = o - tf[0]; tf[3] = tf[2] / std::sqrt(sg * sg + var); tf[4] = a[4 + 3 * f] / a[1]; }
        }
    }
}

void filter_loo_table(const double *row_loo, long n_rows, int nf, double *table)
{
    const size_t ncol = 1 + 6 * (size_t)nf;
    std::vector<double> v;
    for (int f = 0; f < nf; ++f) {
        double *t = table + (size_t)f * kFilterCheckCols;
        for (int c = 0; c < kFilterCheckCols; ++c) t[c] = 0.0;
        std::vector<long> use;
        for (long r = 0; r < n_rows; ++r)
            if (row_loo[(size_t)r * ncol + 1 + 6 * f] > 0.0) use.push_back(r);
        t[0] = (double)use.size();
        if (use.empty()) continue;
        for (int q = 0; q < 4; ++q) {
            v.resize(use.size());
            double sum = 0.0;
            for (size_t k = 0; k < use.size(); ++k) {
                const double *x = row_loo + (size_t)use[k] * ncol + 1 + 6 * f;            // N, R, C, W, D, E
                v[k] = q == 0 ? x[1] / x[0] : q == 1 ? x[2] / x[0] : q == 2 ? (x[3] > 0.0 ? x[4] / x[3] : 0.0) : x[5] / x[0];
                sum += v[k];
            }
            const double mean = sum / (double)use.size();
            double ss = 0.0;
            for (double x : v) ss += (x - mean) * (x - mean);
            std::sort(v.begin(), v.end());
            double *tq = t + 1 + 5 * q;
            tq[0] = mean;
            tq[1] = std::sqrt(ss / (double)use.size());
            tq[2] = percentile_sorted(v, 0.16); tq[3] = percentile_sorted(v, 0.50); tq[4] = percentile_sorted(v, 0.84);
        }
    }
}

void write_star_filter_check(const std::string &path, const std::vector<std::string> &ids, const std::vector<std::string> &filters, const double *table)
{
    std::vector<TableColumn> cols = columns({"rows", "member"}, "%.17g");
    for (const std::string &n : filters)
        for (const char *what : {"_looMag", "_looSd", "_resid", "_z", "_lpd"}) cols.push_back({n + what, "%.17g"});
    write_table(path, "id", &ids, cols, (long)ids.size(), table, cols.size());
}

void write_filter_check(const std::string &path, const std::vector<std::string> &filters, const double *table)
{
    std::vector<TableColumn> cols = {{"nRows", "%.17g"}};
    for (const char *q : {"meanZ", "chi2", "offset", "lpd"})
        for (const char *s : {"mean", "sd", "p16", "p50", "p84"}) cols.push_back({std::string(q) + "_" + s, "%.17g"});
    write_table(path, "filter", &filters, cols, (long)filters.size(), table, kFilterCheckCols);
}

// ---------------------------------------------------------------------------------------------
// starOffsets
// ---------------------------------------------------------------------------------------------
StarOffsetsConfig star_offsets_config(const Settings &st)
{
    StarOffsetsConfig c;
    std::istringstream ds(st.str("starOffsets.direction", "absorption distance"));
    std::string tok;
    while (ds >> tok) c.directions.push_back(tok);
    if (c.directions.empty() || c.directions.size() > B9_OFF_MAX_DIRECTIONS)
        fail("starOffsets.direction: between 1 and " + std::to_string(B9_OFF_MAX_DIRECTIONS) + " directions");
    std::istringstream ts(st.str("starOffsets.tau", "0.1"));
    while (ts >> tok) {
        char *end = nullptr;
        const double v = std::strtod(tok.c_str(), &end);
        if (end == tok.c_str() || *end || !(v > 0.0) || !std::isfinite(v)) fail("starOffsets.tau: '" + tok + "' is not a positive number");
        c.tau.push_back(v);
    }
    if (c.tau.size() == 1) c.tau.assign(c.directions.size(), c.tau[0]);
    if (c.tau.size() != c.directions.size()) fail("starOffsets.tau: one width, or one per direction");
    return c;
}

std::vector<double> offset_direction(const std::string &spec, const std::vector<std::string> &filters, const std::vector<double> &abs_coeff)
{
    const size_t nf = filters.size();
    std::vector<double> k(nf, 0.0);
    if (spec == "absorption") {
        if (abs_coeff.size() < nf) fail("starOffsets.direction: the model pack has no absorption coefficients");
        for (size_t f = 0; f < nf; ++f) k[f] = abs_coeff[f];
    } else if (spec == "distance") {
        for (size_t f = 0; f < nf; ++f) k[f] = 1.0;
    } else if (spec.rfind("filter:", 0) == 0) {
        const auto it = std::find(filters.begin(), filters.end(), spec.substr(7));
        if (it == filters.end()) fail("starOffsets.direction: no filter '" + spec.substr(7) + "'");
        k[(size_t)(it - filters.begin())] = 1.0;
    } else {
        std::string lv = spec;
        for (char &ch : lv) if (ch == ',') ch = ' ';
        std::istringstream ls(lv);
        std::string tok;
        size_t f = 0;
        while (ls >> tok) {
            char *end = nullptr;
            const double v = std::strtod(tok.c_str(), &end);
            if (end == tok.c_str() || *end || !std::isfinite(v)) fail("starOffsets.direction: '" + spec + "' is neither a named direction nor a list of numbers");
            if (f < nf) k[f] = v;
            ++f;
        }
        if (f != nf) fail("starOffsets.direction: '" + spec + "' must hold one value per filter (" + std::to_string(nf) + ")");
    }
    return k;
}

void offset_table(const double *star_off, const double *sigma, const double *k, const double *tau, long n_stars, int nf, int nd, double *table)
{
    const size_t ncol = 2 + 3 * (size_t)nd, tcol = 2 + 4 * (size_t)nd;
    for (long i = 0; i < n_stars; ++i) {
        const double *a = star_off + (size_t)i * ncol;
        double *t = table + (size_t)i * tcol;
        for (size_t c = 0; c < tcol; ++c) t[c] = 0.0;
        t[0] = a[0];
        if (a[0] > 0.0) t[1] = a[1] / a[0];
        if (!(a[1] > 0.0)) continue;                         // no membership weight: every derived value is 0
        for (int j = 0; j < nd; ++j) {
            double C = 0.0;
            for (int f = 0; f < nf; ++f) {
                const double sg = sigma[(size_t)i * nf + f];
                if (sg > 0.0) { const double c = k[(size_t)j * nf + f] / sg; C += c * c; }
            }
            const double V = 1.0 / (C + 1.0 / (tau[j] * tau[j]));
            const double m1 = a[2 + 3 * j] / a[1], m2 = a[3 + 3 * j] / a[1];
            double *tj = t + 2 + 4 * (size_t)j;
            tj[0] = m1;
            tj[1] = std::sqrt(std::max(0.0, m2 - m1 * m1) + V);
            tj[2] = m1 / tj[1];
            tj[3] = a[4 + 3 * j] / a[1];
        }
    }
}

void offset_dist_table(const double *row_off, long n_rows, int nd, double *table)
{
    const size_t ncol = 1 + 4 * (size_t)nd;
    std::vector<double> v;
    for (int j = 0; j < nd; ++j) {
        double *t = table + (size_t)j * kOffsetDistCols;
        for (int c = 0; c < kOffsetDistCols; ++c) t[c] = 0.0;
        std::vector<long> use;
        for (long r = 0; r < n_rows; ++r)
            if (row_off[(size_t)r * ncol + 1 + 4 * j] > 0.0) use.push_back(r);
        t[0] = (double)use.size();
        if (use.empty()) continue;
        for (int q = 0; q < 3; ++q) {
            v.resize(use.size());
            double sum = 0.0;
            for (size_t u = 0; u < use.size(); ++u) {
                const double *x = row_off + (size_t)use[u] * ncol + 1 + 4 * j;            // N, M1, M2, E
                v[u] = q == 0 ? x[1] / x[0] : q == 1 ? std::sqrt(x[2] / x[0]) : x[3] / x[0];
                sum += v[u];
            }
            const double mean = sum / (double)use.size();
            double ss = 0.0;
            for (double x : v) ss += (x - mean) * (x - mean);
            std::sort(v.begin(), v.end());
            double *tq = t + 1 + 5 * q;
            tq[0] = mean;
            tq[1] = std::sqrt(ss / (double)use.size());
            tq[2] = percentile_sorted(v, 0.16); tq[3] = percentile_sorted(v, 0.50); tq[4] = percentile_sorted(v, 0.84);
        }
    }
}

void write_star_offsets(const std::string &path, const std::vector<std::string> &ids, const std::vector<std::string> &directions, const double *table)
{
    std::vector<TableColumn> cols = columns({"rows", "member"}, "%.17g");
    for (const std::string &n : directions)
        for (const char *what : {"_mean", "_sd", "_z", "_logBF"}) cols.push_back({n + what, "%.17g"});
    write_table(path, "id", &ids, cols, (long)ids.size(), table, cols.size());
}

void write_offset_dist(const std::string &path, const std::vector<std::string> &directions, const double *table)
{
    std::vector<TableColumn> cols = {{"nRows", "%.17g"}};
    for (const char *q : {"mean", "rms", "logBF"})
        for (const char *s : {"mean", "sd", "p16", "p50", "p84"}) cols.push_back({std::string(q) + "_" + s, "%.17g"});
    write_table(path, "direction", &directions, cols, (long)directions.size(), table, kOffsetDistCols);
}

// ---------------------------------------------------------------------------------------------
// modelScore
// ---------------------------------------------------------------------------------------------
namespace {
const double kInf = std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();

// Steps (1) - (6) of the PSIS statement on r[0 .. n_t), finite and descending: the tail's length M,
// rho[0 .. M] = r - r[0], paretoK and w[j - 1], the smoothed weight of the j-th SMALLEST of the M tail values.  false: no fit.
struct PsisFit { long M = 0; double k_hat = 0.0; std::vector<double> rho, w; };
bool psis_fit(const double *r, long n_t, double n_f, PsisFit &fit)
{
    const long M = std::min({(long)std::floor(n_f / 5.0), (long)std::ceil(3.0 * std::sqrt(n_f)), n_t - 1});
    if (M < 5) return false;
    const long N = M;
    std::vector<double> &rho = fit.rho, x((size_t)M);
    rho.assign((size_t)M + 1, 0.0);
    for (long j = 0; j <= M; ++j) rho[(size_t)j] = r[j] - r[0];
    const double ec = std::exp(rho[(size_t)M]);
    for (long j = 0; j < M; ++j) x[(size_t)(M - 1 - j)] = std::exp(rho[(size_t)j]) - ec;          // ascending: rho descends
    const double x_n = x[(size_t)N - 1], x_star = x[(size_t)std::floor((double)N / 4.0 + 0.5) - 1];
    if (x_n == 0.0 || !(x_star > 0.0)) return false;
    // Zhang & Stephens' profile fit of the generalised Pareto distribution, with the weakly informative prior on k
    const long m = 30 + (long)std::floor(std::sqrt((double)N));
    std::vector<double> theta((size_t)m), ell((size_t)m);
    auto mean_log1p = [&](double th) { double sum = 0.0; for (long i = 0; i < N; ++i) sum += std::log1p(-th * x[(size_t)i]); return sum / (double)N; };
    for (long j = 1; j <= m; ++j) {
        const double th = 1.0 / x_n + (1.0 - std::sqrt((double)m / ((double)j - 0.5))) / (3.0 * x_star);
        const double k = mean_log1p(th);
        theta[(size_t)j - 1] = th;
        ell[(size_t)j - 1] = (double)N * (std::log(-th / k) - k - 1.0);
    }
    double theta_hat = 0.0;
    for (long j = 0; j < m; ++j) {
        double den = 0.0;
        for (long l = 0; l < m; ++l) den += std::exp(ell[(size_t)l] - ell[(size_t)j]);
        theta_hat += theta[(size_t)j] * (1.0 / den);
    }
    double k_hat = mean_log1p(theta_hat);
    const double sigma = -k_hat / theta_hat;
    k_hat = ((double)N * k_hat + 5.0) / ((double)N + 10.0);
    // the smoothed weights, by rank: the j-th smallest tail value takes the quantile at p_j = (j - 1/2) / M
    fit.w.assign((size_t)M, 0.0);
    for (long j = 1; j <= M; ++j) {
        const double p = ((double)j - 0.5) / (double)M, lp = std::log1p(-p);
        const double q = k_hat == 0.0 ? -sigma * lp : sigma * std::expm1(-k_hat * lp) / k_hat;
        fit.w[(size_t)j - 1] = std::min(1.0, ec + q);
    }
    fit.M = M; fit.k_hat = k_hat;
    return true;
}

// PSIS of one star: r[0 .. n_t) the finite tail values, descending (r[0] = RMAX); -> paretoK, elpdLoo (elpd_is where no fit is made)
void psis_star(const double *r, long n_t, double n_f, double rmax, double sneg, double elpd_is, double &pareto_k, double &elpd_loo)
{
    pareto_k = kNaN;
    elpd_loo = elpd_is;
    PsisFit fit;
    if (!psis_fit(r, n_t, n_f, fit)) return;
    const long M = fit.M;
    double num = n_f - (double)M, tail_raw = 0.0, tail_smooth = 0.0;
    for (long j = 1; j <= M; ++j) {                       // step (7), paired by rank
        const double w = fit.w[(size_t)j - 1], rh = fit.rho[(size_t)(M - j)];
        num += std::exp(std::log(w) - rh);
        tail_smooth += w;
        tail_raw += std::exp(rh);
    }
    const double den = std::max(0.0, sneg - tail_raw) + tail_smooth;
    pareto_k = fit.k_hat;
    elpd_loo = std::log(num) - std::log(den) - rmax;
}

// sum and sqrt(N var_ddof1) of v
void sum_se(const std::vector<double> &v, double &sum, double &se)
{
    sum = 0.0; se = 0.0;
    for (double x : v) sum += x;
    const size_t n = v.size();
    if (n < 2) return;
    const double mean = sum / (double)n;
    double ss = 0.0;
    for (double x : v) ss += (x - mean) * (x - mean);
    se = std::sqrt((double)n * (ss / (double)(n - 1)));
}
}  // namespace

void pointwise_table(const double *acc, const double *tail, int tail_len, long n_stars, double *table)
{
    for (long i = 0; i < n_stars; ++i) {
        const double *a = acc + (size_t)i * 8;
        double *t = table + (size_t)i * kPointwiseCols;
        for (int c = 0; c < kPointwiseCols; ++c) t[c] = 0.0;
        const double rows = a[0], n_inf = a[1], n_f = rows - n_inf;
        t[0] = rows; t[1] = n_inf;
        if (n_inf > 0.0) {                               // a row gives the star no likelihood at all: no finite score
            t[2] = n_f > 0.0 ? a[2] + std::log(a[3]) - std::log(rows) : -kInf;
            t[3] = n_f >= 2.0 ? a[7] / (n_f - 1.0) : 0.0;
            t[4] = t[5] = t[7] = -kInf; t[6] = kInf; t[8] = kInf;
            continue;
        }
        if (!(n_f > 0.0)) continue;
        const double lppd = a[2] + std::log(a[3]) - std::log(rows);
        const double p_waic = n_f >= 2.0 ? a[7] / (n_f - 1.0) : 0.0;
        const double elpd_is = std::log(n_f) - (a[4] + std::log(a[5]));
        long n_t = 0;
        const double *r = tail ? tail + (size_t)i * (size_t)tail_len : nullptr;
        while (r && n_t < tail_len && std::isfinite(r[n_t])) ++n_t;
        double k, loo;
        psis_star(r, n_t, n_f, a[4], a[5], elpd_is, k, loo);
        t[2] = lppd; t[3] = p_waic; t[4] = lppd - p_waic; t[5] = elpd_is; t[6] = k; t[7] = loo; t[8] = lppd - loo;
    }
}

void score_totals(const double *table, long n_stars, double *totals)
{
    std::vector<double> lppd, waic, loo;
    double p_waic = 0.0, p_loo = 0.0, n_infs = 0.0, n_high = 0.0, k_max = kNaN;
    for (long i = 0; i < n_stars; ++i) {
        const double *t = table + (size_t)i * kPointwiseCols;
        if (!(t[0] > 0.0)) continue;
        lppd.push_back(t[2]); waic.push_back(t[4]); loo.push_back(t[7]);
        p_waic += t[3]; p_loo += t[8];
        if (t[1] > 0.0) n_infs += 1.0;
        if (t[6] > 0.7) n_high += 1.0;
        if (std::isfinite(t[6]) && !(k_max >= t[6])) k_max = t[6];
    }
    totals[0] = (double)lppd.size();
    sum_se(lppd, totals[1], totals[2]);
    sum_se(waic, totals[3], totals[4]);
    sum_se(loo, totals[5], totals[6]);
    totals[7] = p_waic; totals[8] = p_loo; totals[9] = n_infs; totals[10] = n_high; totals[11] = k_max;
}

void score_compare(const double *table_a, const std::vector<std::string> &ids_a, const double *table_b, const std::vector<std::string> &ids_b,
                   double *out)
{
    if (ids_a.size() != ids_b.size()) fail("modelScore: the two catalogues differ in their number of stars");
    for (size_t i = 0; i < ids_a.size(); ++i)
        if (ids_a[i] != ids_b[i]) fail("modelScore: the two catalogues differ at star " + std::to_string(i) + " ('" + ids_a[i] + "' against '" + ids_b[i] + "')");
    std::vector<double> d_loo, d_waic;
    double dropped = 0.0;
    for (size_t i = 0; i < ids_a.size(); ++i) {
        const double *a = table_a + i * kPointwiseCols, *b = table_b + i * kPointwiseCols;
        if ((a[0] > 0.0) != (b[0] > 0.0)) dropped += 1.0;                  // scored by one fit only
        if (!(a[0] > 0.0) || !(b[0] > 0.0)) continue;
        d_loo.push_back(a[7] - b[7]);
        d_waic.push_back(a[4] - b[4]);
    }
    out[0] = (double)d_loo.size();
    sum_se(d_loo, out[1], out[2]);
    sum_se(d_waic, out[3], out[4]);
    out[5] = dropped;
}

static const char *const kPointwiseNames[kPointwiseCols] = {"rows", "nInf", "lppd", "pWaic", "elpdWaic", "elpdIs", "paretoK", "elpdLoo", "pLoo"};
static const char *const kScoreNames[kScoreTotals] = {"nStars", "lppd", "lppdSe", "elpdWaic", "elpdWaicSe", "elpdLoo", "elpdLooSe", "pWaic", "pLoo",
                                                      "nInfStars", "nHighK", "maxK"};
static const char *const kCompareNames[kScoreCompare] = {"nStars", "dElpdLoo", "dElpdLooSe", "dElpdWaic", "dElpdWaicSe", "nDropped"};

namespace {
std::vector<TableColumn> columns17(const char *const *names, int n)
{
    std::vector<TableColumn> c;
    for (int k = 0; k < n; ++k) c.push_back({names[k], "%.17g"});
    return c;
}
}  // namespace

void write_pointwise(const std::string &path, const std::vector<std::string> &ids, const double *table)
{
    write_table(path, "id", &ids, columns17(kPointwiseNames, kPointwiseCols), (long)ids.size(), table, kPointwiseCols);
}
void write_model_score(const std::string &path, const double *totals)
{
    write_table(path, nullptr, nullptr, columns17(kScoreNames, kScoreTotals), 1, totals, kScoreTotals);
}
void write_model_compare(const std::string &path, const double *cmp)
{
    write_table(path, nullptr, nullptr, columns17(kCompareNames, kScoreCompare), 1, cmp, kScoreCompare);
}

void write_row_lpd(const std::string &path, const double *row_lpd, long n_rows)
{
    std::vector<double> table(2 * (size_t)n_rows);
    for (long r = 0; r < n_rows; ++r) { table[2 * (size_t)r] = (double)r; table[2 * (size_t)r + 1] = row_lpd[r]; }
    write_table(path, nullptr, nullptr, {{"row", "%ld"}, {"lpd", "%.17g"}}, n_rows, table.data(), 2);
}

void read_pointwise(const std::string &path, std::vector<std::string> &ids, std::vector<double> &table)
{
    std::ifstream in(path);
    if (!in) fail("cannot read " + path);
    std::string line, word;
    if (!std::getline(in, line)) fail(path + ": empty file");
    {
        std::istringstream hs(line);
        hs >> word;
        if (word != "id") fail(path + ": not a .pointwise file (the header starts with '" + word + "')");
        for (const char *n : kPointwiseNames)
            if (!(hs >> word) || word != n) fail(path + ": column '" + std::string(n) + "' missing from the header");
    }
    ids.clear(); table.clear();
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        if (!(ls >> word)) continue;
        ids.push_back(word);
        for (int c = 0; c < kPointwiseCols; ++c) {
            if (!(ls >> word)) fail(path + ": short line for star '" + ids.back() + "'");
            table.push_back(std::strtod(word.c_str(), nullptr));         // (strtod reads inf / -inf / nan as printf wrote them)
        }
    }
}

// ---------------------------------------------------------------------------------------------
// starInfluence
// ---------------------------------------------------------------------------------------------
StarInfluenceConfig star_influence_config(const Settings &st)
{
    StarInfluenceConfig c;
    std::istringstream qs(st.str("starInfluence.quantity", ""));
    std::string tok;
    while (qs >> tok) c.quantities.push_back(tok);
    if (c.quantities.size() > B9_INF_MAX_Q) fail("starInfluence.quantity: at most " + std::to_string(B9_INF_MAX_Q) + " quantities");
    c.group_file = st.str("starInfluence.groupFile", "");
    c.no_groups = st.integer("starInfluence.noGroups", 0) != 0;
    if (c.no_groups && !c.group_file.empty()) fail("starInfluence: give groupFile or noGroups, not both");
    return c;
}

InfluenceQuantities influence_quantities(const StarInfluenceConfig &c, const double *rows, const double *log_post, long n_rows)
{
    if (n_rows < 2) fail("starInfluence: the chain needs at least two main-run rows");
    InfluenceQuantities out;
    std::vector<int> col;                                 // B9_P_* index, or -1: logPost
    auto column = [&](int k, long r) { return k < 0 ? log_post[r] : rows[(size_t)r * B9_NPARAM + k]; };
    if (c.quantities.empty()) {
        for (int k = 0; k < B9_NPARAM; ++k) {
            bool varies = false;
            for (long r = 1; r < n_rows && !varies; ++r) varies = column(k, r) != column(k, 0);
            if (varies) col.push_back(k);
        }
        if (col.empty()) fail("starInfluence: no cluster parameter varies over the main-run rows");
        if (col.size() > B9_INF_MAX_Q) fail("starInfluence: more than " + std::to_string(B9_INF_MAX_Q) + " parameters vary: name the quantities (--quantity)");
    } else {
        for (const std::string &name : c.quantities) {
            int idx = -2;
            if (name == "logPost") idx = -1;
            for (int k = 0; k < B9_NPARAM; ++k) if (name == param_name(k)) idx = k;
            if (idx == -2) fail("starInfluence.quantity: '" + name + "' is neither a cluster parameter nor logPost");
            if (idx == -1 && !log_post) fail("starInfluence.quantity: the chain has no logPost column");
            col.push_back(idx);
        }
    }
    const size_t Q = col.size();
    out.q.assign((size_t)n_rows * Q, 0.0);
    for (size_t j = 0; j < Q; ++j) {
        const int k = col[j];
        out.names.push_back(k < 0 ? "logPost" : param_name(k));
        double sum = 0.0, ss = 0.0;                       // two passes: the mean, then the squares about it
        for (long r = 0; r < n_rows; ++r) sum += column(k, r);
        const double mean = sum / (double)n_rows;
        for (long r = 0; r < n_rows; ++r) { const double d = column(k, r) - mean; ss += d * d; }
        const double sd = std::sqrt(ss / (double)(n_rows - 1));
        if (!(sd > 0.0) || !std::isfinite(sd)) fail("starInfluence.quantity: '" + out.names.back() + "' does not vary over the main-run rows");
        out.mean.push_back(mean); out.sd.push_back(sd);
        for (long r = 0; r < n_rows; ++r) out.q[(size_t)r * Q + j] = (column(k, r) - mean) / sd;
    }
    return out;
}

InfluenceGroups influence_groups(const StarInfluenceConfig &c, const std::vector<std::string> &ids, const std::vector<int32_t> &stage)
{
    InfluenceGroups g;
    if (c.no_groups) return g;
    g.id.assign(ids.size(), -1);
    if (c.group_file.empty()) {
        g.names = {"ms", "wd"};
        for (size_t i = 0; i < ids.size(); ++i) g.id[i] = stage[i] == B9_STAGE_WD ? 1 : stage[i] == B9_STAGE_MSRG ? 0 : -1;
        return g;
    }
    std::ifstream in(c.group_file);
    if (!in) fail("cannot read " + c.group_file);
    std::string line, id, name;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        if (!(ls >> id) || id[0] == '#') continue;
        if (!(ls >> name)) fail(c.group_file + ": no group name for star '" + id + "'");
        const auto it = std::find(ids.begin(), ids.end(), id);
        if (it == ids.end()) fail(c.group_file + ": unknown star id '" + id + "'");
        auto gt = std::find(g.names.begin(), g.names.end(), name);
        if (gt == g.names.end()) {
            if (g.names.size() >= B9_INF_MAX_GROUPS) fail(c.group_file + ": at most " + std::to_string(B9_INF_MAX_GROUPS) + " groups");
            g.names.push_back(name);
            gt = g.names.end() - 1;
        }
        g.id[(size_t)(it - ids.begin())] = (int32_t)(gt - g.names.begin());
    }
    if (g.names.empty()) fail(c.group_file + ": no group");
    return g;
}

void influence_table(const double *acc, const double *tail, int tail_len, long n_stars, int n_q, double *table)
{
    const size_t n_acc = (size_t)B9_INF_N(n_q), n_col = (size_t)kInfluenceHead + 3 * (size_t)n_q;
    for (long i = 0; i < n_stars; ++i) {
        const double *a = acc + (size_t)i * n_acc;
        double *t = table + (size_t)i * n_col;
        for (size_t c = 0; c < n_col; ++c) t[c] = 0.0;
        const double rows = a[B9_INF_ROWS], n_inf = a[B9_INF_NINF], n_f = rows - n_inf;
        t[0] = rows; t[1] = n_inf;
        if (n_inf > 0.0) {                               // a row gives the star no likelihood at all: no finite weight there
            for (size_t c = 3; c < n_col; ++c) t[c] = kNaN;
            continue;
        }
        if (!(n_f > 0.0)) continue;
        const double sneg = a[B9_INF_SNEG];
        t[2] = sneg * sneg / a[B9_INF_SNEG2];
        t[3] = kNaN;
        const double *r = tail ? tail + (size_t)i * (size_t)tail_len : nullptr;
        long n_t = 0;
        while (r && n_t < tail_len && std::isfinite(r[n_t])) ++n_t;
        PsisFit fit;
        if (psis_fit(r, n_t, n_f, fit)) t[3] = fit.k_hat;
        for (int j = 0; j < n_q; ++j) {
            const double *w = a + B9_INF_WQ(j);
            const double m = w[0] / sneg;
            t[kInfluenceHead + 3 * j] = m - w[2];
            t[kInfluenceHead + 3 * j + 1] = n_f >= 2.0 ? -w[3] / (n_f - 1.0) : 0.0;
            t[kInfluenceHead + 3 * j + 2] = std::sqrt(std::max(0.0, w[1] / sneg - m * m));
        }
    }
}

void group_influence_table(const double *group_lpd, long n_rows, int n_groups, const double *q, int n_q, const int32_t *group, long n_stars, double *table)
{
    const size_t n_col = (size_t)kGroupInfluenceHead + 3 * (size_t)n_q;
    for (int g = 0; g < n_groups; ++g) {
        double *t = table + (size_t)g * n_col;
        for (size_t c = 0; c < n_col; ++c) t[c] = 0.0;
        for (long i = 0; i < n_stars; ++i) t[0] += group[i] == g ? 1.0 : 0.0;
        t[1] = (double)n_rows;
        for (long r = 0; r < n_rows; ++r) t[2] += std::isfinite(group_lpd[(size_t)r * n_groups + g]) ? 0.0 : 1.0;
        if (n_rows == 0) continue;
        if (t[2] > 0.0) {
            for (size_t c = 4; c < n_col; ++c) t[c] = kNaN;
            continue;
        }
        // rho = -group_lpd, descending (ties: the earlier row first), the raw weights e^(rho - max rho) and the smoothed ones
        std::vector<long> order((size_t)n_rows);
        for (long r = 0; r < n_rows; ++r) order[(size_t)r] = r;
        auto rho = [&](long r) { return -group_lpd[(size_t)r * n_groups + g]; };
        std::stable_sort(order.begin(), order.end(), [&](long a, long b) { return rho(a) > rho(b); });
        const double top = rho(order[0]);
        std::vector<double> raw((size_t)n_rows), w, sorted((size_t)n_rows);
        for (long r = 0; r < n_rows; ++r) raw[(size_t)r] = std::exp(rho(r) - top);
        for (long k = 0; k < n_rows; ++k) sorted[(size_t)k] = rho(order[(size_t)k]);
        w = raw;
        PsisFit fit;
        t[4] = kNaN;
        if (psis_fit(sorted.data(), n_rows, (double)n_rows, fit)) {
            t[4] = fit.k_hat;
            for (long j = 1; j <= fit.M; ++j) w[(size_t)order[(size_t)(fit.M - j)]] = fit.w[(size_t)j - 1];
        }
        double s1 = 0.0, s2 = 0.0;
        for (double x : raw) { s1 += x; s2 += x * x; }
        t[3] = s1 * s1 / s2;
        for (int j = 0; j < n_q; ++j) {
            double mq = 0.0;
            for (long r = 0; r < n_rows; ++r) mq += q[(size_t)r * n_q + j];
            mq /= (double)n_rows;
            auto mean_of = [&](const std::vector<double> &wt, double &m, double &sd) {
                double sw = 0.0, a = 0.0, b = 0.0;
                for (long r = 0; r < n_rows; ++r) { const double y = q[(size_t)r * n_q + j]; sw += wt[(size_t)r]; a += wt[(size_t)r] * y; b += wt[(size_t)r] * y * y; }
                m = a / sw;
                sd = std::sqrt(std::max(0.0, b / sw - m * m));
            };
            double m_raw, sd_raw, m, sd;
            mean_of(raw, m_raw, sd_raw);
            mean_of(w, m, sd);
            t[kGroupInfluenceHead + 3 * j] = m_raw - mq;
            t[kGroupInfluenceHead + 3 * j + 1] = m - mq;
            t[kGroupInfluenceHead + 3 * j + 2] = sd;
        }
    }
}

void write_star_influence(const std::string &path, const std::vector<std::string> &ids, const std::vector<std::string> &quantities, const double *table)
{
    std::vector<TableColumn> cols = columns({"rows", "nInf", "ess", "paretoK"}, "%.17g");
    for (const std::string &n : quantities)
        for (const char *what : {"shift_", "lin_", "looSd_"}) cols.push_back({what + n, "%.17g"});
    write_table(path, "id", &ids, cols, (long)ids.size(), table, cols.size());
}

void write_group_influence(const std::string &path, const std::vector<std::string> &groups, const std::vector<std::string> &quantities, const double *table)
{
    std::vector<TableColumn> cols = columns({"nStars", "rows", "nInf", "ess", "paretoK"}, "%.17g");
    for (const std::string &n : quantities)
        for (const char *what : {"shiftRaw_", "shift_", "looSd_"}) cols.push_back({what + n, "%.17g"});
    write_table(path, "group", &groups, cols, (long)groups.size(), table, cols.size());
}

void write_influence_scale(const std::string &path, const std::vector<std::string> &quantities, const double *mean, const double *sd)
{
    std::vector<double> table;
    for (size_t j = 0; j < quantities.size(); ++j) { table.push_back(mean[j]); table.push_back(sd[j]); }
    write_table(path, "name", &quantities, columns({"mean", "sd"}, "%.17g"), (long)quantities.size(), table.data(), 2);
}

// ---------------------------------------------------------------------------------------------
// binaryStats
// ---------------------------------------------------------------------------------------------
const ProgramFlags kBinaryStatsFlags = {{"nPops", "binaryStatsNPops", false}};

BinaryStatsConfig binary_stats_config(const Settings &st, double max_mass, int Q)
{
    BinaryStatsConfig c;
    c.q_min = st.num("binaryStats.qMin", 0.0);
    if (!(c.q_min >= 0.0 && c.q_min <= 1.0)) fail("binaryStats.qMin must lie in 0 .. 1");
    if (st.has("binaryStats.massEdges")) {
        if (st.has("binaryStats.massBins")) fail("binaryStats: give massEdges or massBins, not both");
        std::string ev = st.str("binaryStats.massEdges");
        for (char &ch : ev) if (ch == ',' || ch == '[' || ch == ']') ch = ' ';
        std::istringstream es(ev);
        std::string tok;
        while (es >> tok) {
            char *end = nullptr;
            const double v = std::strtod(tok.c_str(), &end);
            if (end == tok.c_str() || *end) fail("binaryStats.massEdges: '" + tok + "' is not a number");
            c.edges.push_back(v);
        }
    } else {
        const long n = st.integer("binaryStats.massBins", std::max(1, std::min(8, B9_RH_MAX_CELLS / std::max(1, Q))));
        if (n < 1 || n > B9_RH_MAX_MBINS) fail("binaryStats.massBins must lie in 1 .. " + std::to_string(B9_RH_MAX_MBINS));
        const double lo = 0.1;
        if (!std::isfinite(max_mass) || !(max_mass > lo)) fail("binaryStats: the models' largest mass must exceed 0.1");
        c.edges.resize((size_t)n + 1);
        for (long b = 0; b <= n; ++b) c.edges[(size_t)b] = lo * std::pow(max_mass / lo, (double)b / (double)n);
        c.edges[0] = lo; c.edges[(size_t)n] = max_mass;
    }
    const long n_mbins = (long)c.edges.size() - 1;
    if (n_mbins < 1 || n_mbins > B9_RH_MAX_MBINS) fail("binaryStats: 1 .. " + std::to_string(B9_RH_MAX_MBINS) + " mass bins (2 .. 17 edges) are allowed");
    if (n_mbins * Q > B9_RH_MAX_CELLS) fail("binaryStats: mass bins x nMassRatios must not exceed " + std::to_string(B9_RH_MAX_CELLS));
    for (long b = 0; b <= n_mbins; ++b)
        if (!std::isfinite(c.edges[(size_t)b]) || (b > 0 && !(c.edges[(size_t)b] > c.edges[(size_t)b - 1])))
            fail("binaryStats: the mass edges must be finite and strictly ascending");
    return c;
}

namespace {
// mean, population standard deviation and 16th / 50th / 84th percentiles of v (mass_function_table's arithmetic) -> t[0 .. 4]; v is sorted
void five_stats(std::vector<double> &v, double *t)
{
    double sum = 0.0;
    for (double x : v) sum += x;
    const double mean = sum / (double)v.size();
    double ss = 0.0;
    for (double x : v) ss += (x - mean) * (x - mean);
    std::sort(v.begin(), v.end());
    t[0] = mean;
    t[1] = std::sqrt(ss / (double)v.size());
    t[2] = percentile_sorted(v, 0.16); t[3] = percentile_sorted(v, 0.50); t[4] = percentile_sorted(v, 0.84);
}

void check_ratio_grid(const char *who, int n_mbins, int Q, double q_min)
{
    if (n_mbins < 1 || Q < 1) fail(std::string(who) + ": n_mbins and Q must be positive");
    if (!(q_min >= 0.0 && q_min <= 1.0)) fail(std::string(who) + ": q_min must lie in 0 .. 1");
}

// does ratio node j of Q count as a binary at q_min?
bool ratio_counts(int j, int Q, double q_min) { return j >= 1 && (double)j / (double)Q >= q_min; }

// The lines of b9_ratio_hist's row_cells [n_rows][n_mbins Q + 1]: line b < n_mbins is mass bin b, line n_mbins is "all" (the bins'
// cells added in ascending b).  fn(line, rows, cells): rows = the rows with member column > 0 and N > 0 of that line, cells
// [rows][Q] theirs, in row order.
template <class Fn> void for_ratio_lines(const double *row_cells, long n_rows, int n_mbins, int Q, Fn &&fn)
{
    const size_t ncol = (size_t)n_mbins * Q + 1;
    std::vector<double> line((size_t)Q), cells;
    for (int ln = 0; ln <= n_mbins; ++ln) {
        cells.clear();
        long used = 0;
        for (long r = 0; r < n_rows; ++r) {
            const double *x = row_cells + (size_t)r * ncol;
            if (!(x[ncol - 1] > 0.0)) continue;
            for (int j = 0; j < Q; ++j) {
                if (ln < n_mbins) { line[(size_t)j] = x[(size_t)ln * Q + j]; continue; }
                double a = 0.0;
                for (int b = 0; b < n_mbins; ++b) a = a + x[(size_t)b * Q + j];
                line[(size_t)j] = a;
            }
            double N = 0.0;
            for (int j = 0; j < Q; ++j) N = N + line[(size_t)j];
            if (!(N > 0.0)) continue;
            cells.insert(cells.end(), line.begin(), line.end());
            ++used;
        }
        fn(ln, used, cells.data());
    }
}
}  // namespace

void binary_table(const double *row_cells, long n_rows, const double *mass_edges, int n_mbins, int Q, double q_min, double *table)
{
    check_ratio_grid("binary_table", n_mbins, Q, q_min);
    for_ratio_lines(row_cells, n_rows, n_mbins, Q, [&](int ln, long used, const double *cells) {
        double *t = table + (size_t)ln * kBinaryTableCols;
        for (int c = 0; c < kBinaryTableCols; ++c) t[c] = 0.0;
        t[0] = ln < n_mbins ? mass_edges[ln] : mass_edges[0];
        t[1] = ln < n_mbins ? mass_edges[ln + 1] : mass_edges[n_mbins];
        t[2] = (double)used;
        if (!used) return;
        std::vector<double> vn((size_t)used), vf((size_t)used);
        for (long k = 0; k < used; ++k) {
            const double *x = cells + (size_t)k * Q;
            double N = 0.0, B = 0.0;
            for (int j = 0; j < Q; ++j) N = N + x[j];
            for (int j = 0; j < Q; ++j) if (ratio_counts(j, Q, q_min)) B = B + x[j];
            vn[(size_t)k] = N; vf[(size_t)k] = B / N;
        }
        five_stats(vn, t + 3);
        five_stats(vf, t + 8);
    });
}

void ratio_dist_table(const double *row_cells, long n_rows, int n_mbins, int Q, double *table)
{
    check_ratio_grid("ratio_dist_table", n_mbins, Q, 0.0);
    for_ratio_lines(row_cells, n_rows, n_mbins, Q, [&](int ln, long used, const double *cells) {
        std::vector<double> v((size_t)used);
        for (int j = 0; j < Q; ++j) {
            double *t = table + ((size_t)ln * Q + j) * kRatioDistCols;
            for (int c = 0; c < kRatioDistCols; ++c) t[c] = 0.0;
            t[0] = (double)j; t[1] = (double)j / (double)Q; t[2] = (double)used;
            if (!used) continue;
            for (long k = 0; k < used; ++k) {
                const double *x = cells + (size_t)k * Q;
                double N = 0.0;
                for (int i = 0; i < Q; ++i) N = N + x[i];
                v[(size_t)k] = x[j] / N;
            }
            five_stats(v, t + 3);
        }
    });
}

void star_ratio_table(const double *star_cells, long n_stars, int n_mbins, int Q, double q_min, long n_rows_in_grid, double *table)
{
    check_ratio_grid("star_ratio_table", n_mbins, Q, q_min);
    const size_t ncol = (size_t)n_mbins * Q + 1, tcol = 4 + (size_t)Q;
    for (long i = 0; i < n_stars; ++i) {
        const double *a = star_cells + (size_t)i * ncol, tot = a[ncol - 1];
        double *t = table + (size_t)i * tcol;
        for (size_t c = 0; c < tcol; ++c) t[c] = 0.0;
        t[0] = (double)n_rows_in_grid;
        if (n_rows_in_grid > 0) t[1] = tot / (double)n_rows_in_grid;
        if (!(tot > 0.0)) continue;                          // no membership weight: every derived value is 0
        double in = 0.0, above = 0.0;
        for (int j = 0; j < Q; ++j) {
            double s = 0.0;
            for (int b = 0; b < n_mbins; ++b) s = s + a[(size_t)b * Q + j];
            in = in + s;
            if (ratio_counts(j, Q, q_min)) above = above + s;
            t[4 + j] = s / tot;
        }
        t[2] = in / tot;
        t[3] = above / tot;
    }
}

namespace {
std::vector<std::string> ratio_line_labels(int n_mbins, int per_line)
{
    std::vector<std::string> labels;
    for (int ln = 0; ln <= n_mbins; ++ln)
        for (int k = 0; k < per_line; ++k) labels.push_back(ln < n_mbins ? std::to_string(ln) : "all");
    return labels;
}
}  // namespace

void write_binary_fraction(const std::string &path, const double *table, int n_mbins)
{
    std::vector<TableColumn> cols = columns({"lo", "hi", "nRows", "N_mean", "N_sd", "N_p16", "N_p50", "N_p84", "f_mean", "f_sd", "f_p16", "f_p50", "f_p84"}, "%.17g");
    cols[2].fmt = "%ld";
    const std::vector<std::string> labels = ratio_line_labels(n_mbins, 1);
    write_table(path, "bin", &labels, cols, n_mbins + 1, table, kBinaryTableCols);
}

void write_ratio_dist(const std::string &path, const double *table, int n_mbins, int Q)
{
    std::vector<TableColumn> cols = columns({"j", "q", "nRows", "mean", "sd", "p16", "p50", "p84"}, "%.17g");
    cols[0].fmt = "%ld"; cols[2].fmt = "%ld";
    const std::vector<std::string> labels = ratio_line_labels(n_mbins, Q);
    write_table(path, "bin", &labels, cols, (long)(n_mbins + 1) * Q, table, kRatioDistCols);
}

void write_star_ratio(const std::string &path, const std::vector<std::string> &ids, const double *table, int Q)
{
    std::vector<TableColumn> cols = {{"rows", "%ld"}, {"member", "%.17g"}, {"inRange", "%.17g"}, {"pBinaryAbove", "%.17g"}};
    for (int j = 0; j < Q; ++j) cols.push_back({"q" + std::to_string(j), "%.17g"});
    write_table(path, "id", &ids, cols, (long)ids.size(), table, cols.size());
}

}  // namespace b9h
