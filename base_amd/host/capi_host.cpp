// capi_host.cpp -- the C surface of libbase9host.so declared in include/base9_host.h: the walker-parallel sampler and
// its exchange for callers that are not C++ (bench.py, tests), and the host loaders so that tests can check the parsers
// against the generators without a GPU.  No numerics.
#include "../../include/base9_host.h"
#include "b9host.hpp"
#include "b9sampler.hpp"
#include "b9sim.hpp"
#include "cli_common.hpp"

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

namespace {
std::string g_err;
template <class F> int guard(F f) { try { f(); return 0; } catch (const std::exception &e) { g_err = e.what(); return -1; } }

std::string g17(double v)
{
    char b[40];
    std::snprintf(b, sizeof b, "%.17g", v);
    return b;
}

std::vector<std::string> strings(const char *const *v, long n) { return std::vector<std::string>(v, v + n); }

// What a program's main makes of a command line, as "key = value" lines: parsed with the program's own flags, then
// text(settings) copied into out.
template <class F> int settings_text(const std::string &who, int argc, char **argv, const b9h::ProgramFlags &flags, char *out, int cap, F text)
{
    return guard([&] {
        if (!out) throw std::runtime_error(who + ": NULL argument");
        b9h::Settings st;
        st.parse_args(argc, argv, flags);
        const std::string d = text(st);
        if ((int)d.size() >= cap) throw std::runtime_error(who + ": output buffer too small");
        std::memcpy(out, d.c_str(), d.size() + 1);
    });
}

std::string grid_text(const b9h::ChainGrid &g)
{
    return "margIsoIncrem = " + std::to_string(g.K) + "\nnMassRatios = " + std::to_string(g.Q) + "\nnPops = " + std::to_string(g.n_pops) + "\n";
}
}  // namespace

extern "C" {

const char *b9h_last_error(void) { return g_err.c_str(); }

// Loads a pack and hands out a b9_pack view; the storage lives until b9h_free_pack.
int b9h_load_pack(const char *dir, const char *ms_model, const char *wd_model, const char *filters_csv,
                  void **handle, b9_pack *view)
{
    return guard([&] {
        std::vector<std::string> filters;
        std::string cur;
        for (const char *p = filters_csv; ; ++p) {
            if (*p == ',' || *p == '\0') { if (!cur.empty()) filters.push_back(cur); cur.clear(); if (!*p) break; }
            else cur += *p;
        }
        auto *pk = new b9h::ModelPack(b9h::load_model_pack(dir, ms_model, wd_model, filters));
        *handle = pk;
        *view = pk->view();
    });
}
void b9h_free_pack(void *handle) { delete static_cast<b9h::ModelPack *>(handle); }

int b9h_read_phot(const char *path, double min_mag, double max_mag, int index, void **handle, b9_stars *view,
                  char *filters_out, int filters_cap)
{
    return guard([&] {
        auto *ph = new b9h::Photometry(b9h::read_photometry(path, min_mag, max_mag, index));
        *handle = ph;
        *view = ph->view();
        std::string csv;
        for (auto &f : ph->filters) csv += (csv.empty() ? "" : ",") + f;
        std::strncpy(filters_out, csv.c_str(), (size_t)filters_cap - 1);
        filters_out[filters_cap - 1] = '\0';
    });
}
void b9h_free_phot(void *handle) { delete static_cast<b9h::Photometry *>(handle); }

// Resolves settings (YAML + flags given as one string per argv entry) and returns "key = value" lines.
int b9h_settings_dump(int argc, char **argv, char *out, int cap)
{
    return guard([&] {
        b9h::Settings st;
        st.parse_args(argc, argv);
        std::string d = st.dump();
        std::strncpy(out, d.c_str(), (size_t)cap - 1);
        out[cap - 1] = '\0';
    });
}

// ---- simCluster / scatterCluster draws (b9sim.hpp) -----------------------------------------------------------------
int b9h_sim_draw_systems(uint64_t seed, int64_t i0, int64_t n, double min_mass, double max_mass, double percent_binary,
                         double min_mass_ratio, double percent_db, int n_pops, double lambda, const double *tip,
                         double *mass1, double *mass_ratio, int32_t *wd_type, int32_t *pop)
{
    return guard([&] {
        b9h::Settings st;              // through the settings, so that the values are checked as simCluster checks them
        st.set("simCluster.minMass", g17(min_mass)); st.set("simCluster.maxMass", g17(max_mass));
        st.set("simCluster.percentBinary", g17(percent_binary)); st.set("simCluster.minMassRatio", g17(min_mass_ratio));
        st.set("simCluster.percentDB", g17(percent_db)); st.set("simCluster.nPops", std::to_string(n_pops));
        b9h::SimConfig c = b9h::sim_config(st);
        c.seed = seed;
        const double tips[2] = {tip[0], n_pops == 2 ? tip[1] : tip[0]};
        b9h::sim_draw_systems(c, lambda, tips, i0, n, mass1, mass_ratio, wd_type, pop);
    });
}

int b9h_sim_field_mags(uint64_t seed, int64_t i0, int64_t n, int n_filt, const double *lo, const double *hi, double *mags)
{
    return guard([&] { b9h::sim_field_mags(seed, i0, n, n_filt, lo, hi, mags); });
}

int b9h_scatter(uint64_t seed, const int64_t *ids, int64_t n, int n_filt, const double *mags, double sigma_floor,
                double sigma_at_limit, double faint_limit, double *sigma, double *obs)
{
    return guard([&] {
        b9h::ScatterConfig c;
        c.seed = seed; c.sigma_floor = sigma_floor; c.sigma_at_limit = sigma_at_limit; c.faint_limit = faint_limit;
        b9h::scatter_noise(c, ids, n, n_filt, mags, sigma, obs);
    });
}

int b9h_sim_settings(int program, int argc, char **argv, char *out, int cap)
{
    return guard([&] {
        b9h::Settings st;
        st.parse_args(argc, argv);
        std::string d;
        if (program == 0) {
            const b9h::SimConfig c = b9h::sim_config(st);
            d = "nStars = " + std::to_string(c.n_stars) + "\nnFieldStars = " + std::to_string(c.n_field) +
                "\npercentBinary = " + g17(c.percent_binary) + "\npercentDB = " + g17(c.percent_db) + "\nminMass = " + g17(c.min_mass) +
                "\nmaxMass = " + g17(c.max_mass) + "\nminMassRatio = " + g17(c.min_mass_ratio) + "\nmemberPrior = " + g17(c.member_prior) +
                "\nnPops = " + std::to_string(c.n_pops) + "\nseed = " + std::to_string(c.seed) + "\n";
        } else {
            const b9h::ScatterConfig c = b9h::scatter_config(st);
            d = "brightLimit = " + g17(c.bright_limit) + "\nfaintLimit = " + g17(c.faint_limit) + "\nrelevantFilt = " +
                std::to_string(c.relevant_filt) + "\nlimitS2N = " + g17(c.limit_s2n) + "\nsigmaFloor = " + g17(c.sigma_floor) +
                "\nsigmaAtLimit = " + g17(c.sigma_at_limit) + "\nmemberPrior = " + g17(c.member_prior) + "\nseed = " + std::to_string(c.seed) + "\n";
        }
        if ((int)d.size() >= cap) throw std::runtime_error("b9h_sim_settings: output buffer too small");
        std::memcpy(out, d.c_str(), d.size() + 1);
    });
}

int b9h_read_res_rows(const char *path, const double *start_row, int stage, double *rows, long cap_rows, long *n_rows)
{
    return guard([&] {
        if (!path || !start_row || !n_rows) throw std::runtime_error("b9h_read_res_rows: NULL argument");
        const std::vector<double> r = b9h::read_res_rows(path, std::vector<double>(start_row, start_row + B9_NPARAM), stage);
        *n_rows = (long)(r.size() / B9_NPARAM);
        if (rows) std::memcpy(rows, r.data(), sizeof(double) * B9_NPARAM * (size_t)std::max(0l, std::min(*n_rows, cap_rows)));
    });
}

int b9h_star_table(const double *acc, long n_stars, double *table)
{
    return guard([&] {
        if (n_stars < 0 || (n_stars > 0 && (!acc || !table))) throw std::runtime_error("b9h_star_table: NULL argument");
        b9h::star_table(acc, n_stars, table);
    });
}

int b9h_write_star_summary(const char *path, const char *const *ids, long n_stars, const double *acc, int n_pops)
{
    return guard([&] {
        if (!path || n_stars < 0 || (n_stars > 0 && (!ids || !acc))) throw std::runtime_error("b9h_write_star_summary: NULL argument");
        b9h::write_star_summary(path, strings(ids, n_stars), acc, n_pops);
    });
}

int b9h_wd_table(const double *acc, long n_wd, double *table)
{
    return guard([&] {
        if (n_wd < 0 || (n_wd > 0 && (!acc || !table))) throw std::runtime_error("b9h_wd_table: NULL argument");
        b9h::wd_table(acc, n_wd, table);
    });
}

int b9h_write_wd_summary(const char *path, const char *const *ids, long n_wd, const double *acc, int n_pops)
{
    return guard([&] {
        if (!path || n_wd < 0 || (n_wd > 0 && (!ids || !acc))) throw std::runtime_error("b9h_write_wd_summary: NULL argument");
        b9h::write_wd_summary(path, strings(ids, n_wd), acc, n_pops);
    });
}

int b9h_mass_function_table(const double *row_hist, long n_rows, const double *edges, int n_bins, double *table)
{
    return guard([&] {
        if (n_rows < 0 || n_bins < 1 || !edges || !table || (n_rows > 0 && !row_hist)) throw std::runtime_error("b9h_mass_function_table: invalid argument");
        b9h::mass_function_table(row_hist, n_rows, edges, n_bins, table);
    });
}

int b9h_write_mass_function(const char *path, const double *table, int n_bins)
{
    return guard([&] {
        if (!path || !table || n_bins < 1) throw std::runtime_error("b9h_write_mass_function: invalid argument");
        b9h::write_mass_function(path, table, n_bins);
    });
}

int b9h_write_star_mass_hist(const char *path, const char *const *ids, long n_stars, const double *star_hist, int n_bins, long n_rows)
{
    return guard([&] {
        if (!path || n_stars < 0 || n_bins < 1 || (n_stars > 0 && (!ids || !star_hist))) throw std::runtime_error("b9h_write_star_mass_hist: invalid argument");
        b9h::write_star_mass_hist(path, strings(ids, n_stars), star_hist, n_bins, n_rows);
    });
}

int b9h_mass_function_settings(int argc, char **argv, double m_wd_up, char *out, int cap, double *edges /* [B9_HIST_MAX_BINS + 1], nullable */)
{
    return settings_text("b9h_mass_function_settings", argc, argv, b9h::kMassFunctionFlags, out, cap, [&](const b9h::Settings &st) {
        const b9h::MassFunctionConfig c = b9h::mass_function_config(st, m_wd_up);
        const std::string grid = grid_text(b9h::chain_grid(st, "massFunction"));
        if (edges) { const std::vector<double> e = c.edges(); std::copy(e.begin(), e.end(), edges); }
        return "nBins = " + std::to_string(c.n_bins) + "\nminMass = " + g17(c.min_mass) + "\nmaxMass = " + g17(c.max_mass) +
               "\nlinearBins = " + std::to_string((int)c.linear) + "\nquantity = " + std::to_string(c.quantity) +
               "\nperStar = " + std::to_string((int)c.per_star) + "\n" + grid;
    });
}

int b9h_binary_table(const double *row_cells, long n_rows, const double *mass_edges, int n_mbins, int Q, double q_min, double *table)
{
    return guard([&] {
        if (n_rows < 0 || !mass_edges || !table || (n_rows > 0 && !row_cells)) throw std::runtime_error("b9h_binary_table: invalid argument");
        b9h::binary_table(row_cells, n_rows, mass_edges, n_mbins, Q, q_min, table);
    });
}

int b9h_ratio_dist_table(const double *row_cells, long n_rows, int n_mbins, int Q, double *table)
{
    return guard([&] {
        if (n_rows < 0 || !table || (n_rows > 0 && !row_cells)) throw std::runtime_error("b9h_ratio_dist_table: invalid argument");
        b9h::ratio_dist_table(row_cells, n_rows, n_mbins, Q, table);
    });
}

int b9h_star_ratio_table(const double *star_cells, long n_stars, int n_mbins, int Q, double q_min, long n_rows_in_grid, double *table)
{
    return guard([&] {
        if (n_stars < 0 || n_rows_in_grid < 0 || (n_stars > 0 && (!star_cells || !table))) throw std::runtime_error("b9h_star_ratio_table: invalid argument");
        b9h::star_ratio_table(star_cells, n_stars, n_mbins, Q, q_min, n_rows_in_grid, table);
    });
}

int b9h_write_binary_fraction(const char *path, const double *table, int n_mbins)
{
    return guard([&] {
        if (!path || !table || n_mbins < 1) throw std::runtime_error("b9h_write_binary_fraction: invalid argument");
        b9h::write_binary_fraction(path, table, n_mbins);
    });
}

int b9h_write_ratio_dist(const char *path, const double *table, int n_mbins, int Q)
{
    return guard([&] {
        if (!path || !table || n_mbins < 1 || Q < 1) throw std::runtime_error("b9h_write_ratio_dist: invalid argument");
        b9h::write_ratio_dist(path, table, n_mbins, Q);
    });
}

int b9h_write_star_ratio(const char *path, const char *const *ids, long n_stars, const double *table, int Q)
{
    return guard([&] {
        if (!path || n_stars < 0 || Q < 1 || (n_stars > 0 && (!ids || !table))) throw std::runtime_error("b9h_write_star_ratio: invalid argument");
        b9h::write_star_ratio(path, strings(ids, n_stars), table, Q);
    });
}

int b9h_refine_star_edges(const double *edges, const double *acc, long n_stars, int n_bins, const double *levels, int n_levels, double tol,
                          double *lo, double *hi, double *below, double *inside, double *value, int32_t *is_final, int32_t *flags, double *next_edges)
{
    return guard([&] {
        if (n_stars < 0 || !levels || !lo || !hi || !below || !inside || !value || !is_final || (n_stars > 0 && (!edges || !acc || !flags || !next_edges)))
            throw std::runtime_error("b9h_refine_star_edges: NULL argument");
        b9h::refine_star_edges(edges, acc, n_stars, n_bins, levels, n_levels, tol, lo, hi, below, inside, value, is_final, flags, next_edges);
    });
}

int b9h_star_intervals_table(long n_stars, int n_levels, const double *member, const double *value, const double *lo, const double *hi,
                             const int32_t *passes, const int32_t *flags, double *table)
{
    return guard([&] {
        if (n_stars < 0 || n_levels < 1 || (n_stars > 0 && (!member || !value || !lo || !hi || !passes || !flags || !table)))
            throw std::runtime_error("b9h_star_intervals_table: invalid argument");
        b9h::StarIntervals r;
        r.n_levels = n_levels; r.n_stars = n_stars;
        const size_t nm = (size_t)n_stars * n_levels;
        r.member.assign(member, member + n_stars); r.value.assign(value, value + nm); r.lo.assign(lo, lo + nm); r.hi.assign(hi, hi + nm);
        r.passes.assign(passes, passes + n_stars); r.flags.assign(flags, flags + n_stars);
        b9h::star_intervals_table(r, table);
    });
}

int b9h_write_star_intervals(const char *path, const char *const *ids, long n_stars, const double *levels, int n_levels, const double *table)
{
    return guard([&] {
        if (!path || n_stars < 0 || n_levels < 1 || !levels || (n_stars > 0 && (!ids || !table))) throw std::runtime_error("b9h_write_star_intervals: invalid argument");
        b9h::write_star_intervals(path, strings(ids, n_stars), std::vector<double>(levels, levels + n_levels), table);
    });
}

int b9h_star_intervals_settings(int argc, char **argv, char *out, int cap)
{
    return settings_text("b9h_star_intervals_settings", argc, argv, b9h::kStarIntervalsFlags, out, cap, [&](const b9h::Settings &st) {
        const b9h::StarIntervalsConfig c = b9h::star_intervals_config(st);
        std::string lv;
        for (size_t l = 0; l < c.levels.size(); ++l) lv += (l ? "," : "") + g17(c.levels[l]);
        return "quantity = " + std::to_string(c.quantity) + "\nlevels = " + lv + "\ntol = " + g17(c.tol) + "\nmaxPasses = " +
               std::to_string(c.max_passes) + "\n" + grid_text(b9h::chain_grid(st, "starIntervals"));
    });
}

int b9h_wd_first_ranges(const double *wd_acc, long n_wd, int quantity_mask, double *first_lo, double *first_hi)
{
    return guard([&] {
        if (n_wd < 0 || (n_wd > 0 && (!wd_acc || !first_lo || !first_hi))) throw std::runtime_error("b9h_wd_first_ranges: NULL argument");
        b9h::wd_first_ranges(wd_acc, n_wd, quantity_mask, first_lo, first_hi);
    });
}

int b9h_wd_intervals_table(long n_wd, int n_sel, int n_levels, const double *member, const double *counted, const double *value, const double *lo,
                           const double *hi, const int32_t *passes, const int32_t *flags, double *table)
{
    return guard([&] {
        if (n_wd < 0 || n_sel < 1 || n_sel > B9_WQ_N || n_levels < 1 || (n_wd > 0 && (!member || !counted || !value || !lo || !hi || !passes || !flags || !table)))
            throw std::runtime_error("b9h_wd_intervals_table: invalid argument");
        b9h::wd_intervals_table(n_wd, n_sel, n_levels, member, counted, value, lo, hi, passes, flags, table);
    });
}

int b9h_write_wd_intervals(const char *path, const char *const *ids, long n_wd, int quantity_mask, const double *levels, int n_levels, const double *table)
{
    return guard([&] {
        if (!path || n_wd < 0 || n_levels < 1 || !levels || quantity_mask < 1 || quantity_mask >= (1 << B9_WQ_N) || (n_wd > 0 && (!ids || !table)))
            throw std::runtime_error("b9h_write_wd_intervals: invalid argument");
        b9h::write_wd_intervals(path, strings(ids, n_wd), quantity_mask, std::vector<double>(levels, levels + n_levels), table);
    });
}

int b9h_wd_intervals_settings(int argc, char **argv, char *out, int cap)
{
    return settings_text("b9h_wd_intervals_settings", argc, argv, b9h::kWdIntervalsFlags, out, cap, [&](const b9h::Settings &st) {
        const b9h::WdIntervalsConfig c = b9h::wd_intervals_config(st);
        std::string lv;
        for (size_t l = 0; l < c.levels.size(); ++l) lv += (l ? "," : "") + g17(c.levels[l]);
        return "quantities = " + std::to_string(c.quantity_mask) + "\nlevels = " + lv + "\ntol = " + g17(c.tol) + "\nmaxPasses = " +
               std::to_string(c.max_passes) + "\nnMassNodes = " + std::to_string(c.n_nodes) + "\nnPops = " +
               std::to_string(b9h::chain_n_pops(st, "wdIntervals")) + "\n";
    });
}

int b9h_band_first_ranges(const double *mom, long n_lines, double *first_lo, double *first_hi)
{
    return guard([&] {
        if (n_lines < 0 || (n_lines > 0 && (!mom || !first_lo || !first_hi))) throw std::runtime_error("b9h_band_first_ranges: NULL argument");
        b9h::band_first_ranges(mom, n_lines, first_lo, first_hi);
    });
}

int b9h_band_first_edges(const double *mom, long n_lines, int n_bins, double *edges)
{
    return guard([&] {
        if (n_lines < 0 || (n_lines > 0 && (!mom || !edges))) throw std::runtime_error("b9h_band_first_edges: NULL argument");
        b9h::band_first_edges(mom, n_lines, n_bins, edges);
    });
}

int b9h_band_table(const double *mom, const double *pivot, long n_lines, int n_levels, const double *value, const double *lo, const double *hi,
                   const int32_t *passes, const int32_t *flags, double *table)
{
    return guard([&] {
        if (n_lines < 0 || n_levels < 1 || (n_lines > 0 && (!mom || !value || !lo || !hi || !passes || !flags || !table)))
            throw std::runtime_error("b9h_band_table: invalid argument");
        b9h::band_table(mom, pivot, n_lines, n_levels, value, lo, hi, passes, flags, table);
    });
}

int b9h_write_cmd_band(const char *path, const char *const *names, long n_lines, const double *levels, int n_levels, const double *table)
{
    return guard([&] {
        if (!path || n_lines < 0 || n_levels < 1 || !levels || (n_lines > 0 && (!names || !table))) throw std::runtime_error("b9h_write_cmd_band: invalid argument");
        b9h::write_cmd_band(path, strings(names, n_lines), std::vector<double>(levels, levels + n_levels), table);
    });
}

int b9h_cmd_band_settings(int argc, char **argv, char *out, int cap)
{
    return settings_text("b9h_cmd_band_settings", argc, argv, b9h::kCmdBandFlags, out, cap, [&](const b9h::Settings &st) {
        const b9h::CmdBandConfig c = b9h::cmd_band_config(st);
        std::string rs, cs, lv;
        for (size_t s = 0; s < c.ratios.size(); ++s) rs += (s ? "," : "") + g17(c.ratios[s]);
        for (size_t k = 0; k < c.colours.size(); ++k) cs += (k ? "," : "") + c.colours[k].first + "-" + c.colours[k].second;
        for (size_t l = 0; l < c.levels.size(); ++l) lv += (l ? "," : "") + g17(c.levels[l]);
        return "ratios = " + rs + "\nwdNodes = " + std::to_string(c.wd_nodes) + "\nwdTypes = " + std::to_string(c.wd_types) + "\ncolours = " + cs +
               "\nlevels = " + lv + "\ntol = " + g17(c.tol) + "\nmaxPasses = " + std::to_string(c.max_passes) + "\nnPops = " +
               std::to_string(b9h::chain_n_pops(st, "cmdBand")) + "\n";
    });
}

int b9h_resid_table(const double *star_resid, const double *obs, const double *sigma, long n_stars, int n_filt, double *table)
{
    return guard([&] {
        if (n_stars < 0 || n_filt < 1 || !table || (n_stars > 0 && (!star_resid || !obs || !sigma))) throw std::runtime_error("b9h_resid_table: invalid argument");
        b9h::resid_table(star_resid, obs, sigma, n_stars, n_filt, table);
    });
}

int b9h_filter_resid_table(const double *row_resid, long n_rows, int n_filt, double *table)
{
    return guard([&] {
        if (n_rows < 0 || n_filt < 1 || !table || (n_rows > 0 && !row_resid)) throw std::runtime_error("b9h_filter_resid_table: invalid argument");
        b9h::filter_resid_table(row_resid, n_rows, n_filt, table);
    });
}

int b9h_write_phot_resid(const char *path, const char *const *ids, long n_stars, const char *const *filters, int n_filt, const double *table)
{
    return guard([&] {
        if (!path || n_stars < 0 || n_filt < 1 || !filters || (n_stars > 0 && (!ids || !table))) throw std::runtime_error("b9h_write_phot_resid: invalid argument");
        b9h::write_phot_resid(path, strings(ids, n_stars), strings(filters, n_filt), table);
    });
}

int b9h_write_filter_resid(const char *path, const char *const *filters, int n_filt, const double *table)
{
    return guard([&] {
        if (!path || n_filt < 1 || !filters || !table) throw std::runtime_error("b9h_write_filter_resid: invalid argument");
        b9h::write_filter_resid(path, strings(filters, n_filt), table);
    });
}

int b9h_loo_table(const double *star_loo, const double *obs, const double *sigma, long n_stars, int n_filt, double *table)
{
    return guard([&] {
        if (n_stars < 0 || n_filt < 1 || !table || (n_stars > 0 && (!star_loo || !obs || !sigma))) throw std::runtime_error("b9h_loo_table: invalid argument");
        b9h::loo_table(star_loo, obs, sigma, n_stars, n_filt, table);
    });
}

int b9h_filter_loo_table(const double *row_loo, long n_rows, int n_filt, double *table)
{
    return guard([&] {
        if (n_rows < 0 || n_filt < 1 || !table || (n_rows > 0 && !row_loo)) throw std::runtime_error("b9h_filter_loo_table: invalid argument");
        b9h::filter_loo_table(row_loo, n_rows, n_filt, table);
    });
}

int b9h_write_star_filter_check(const char *path, const char *const *ids, long n_stars, const char *const *filters, int n_filt, const double *table)
{
    return guard([&] {
        if (!path || n_stars < 0 || n_filt < 1 || !filters || (n_stars > 0 && (!ids || !table))) throw std::runtime_error("b9h_write_star_filter_check: invalid argument");
        b9h::write_star_filter_check(path, strings(ids, n_stars), strings(filters, n_filt), table);
    });
}

int b9h_write_filter_check(const char *path, const char *const *filters, int n_filt, const double *table)
{
    return guard([&] {
        if (!path || n_filt < 1 || !filters || !table) throw std::runtime_error("b9h_write_filter_check: invalid argument");
        b9h::write_filter_check(path, strings(filters, n_filt), table);
    });
}

int b9h_filter_check_settings(int argc, char **argv, char *out, int cap)
{
    return settings_text("b9h_filter_check_settings", argc, argv, b9h::kFilterCheckFlags, out, cap, [&](const b9h::Settings &st) {
        return grid_text(b9h::chain_grid(st, "filterCheck")) + "perStar = " + std::to_string((int)b9h::filter_check_config(st).per_star) + "\n";
    });
}

int b9h_offset_direction(const char *spec, const char *const *filters, int n_filt, const double *abs_coeff, double *k)
{
    return guard([&] {
        if (!spec || n_filt < 1 || !filters || !k) throw std::runtime_error("b9h_offset_direction: invalid argument");
        const std::vector<double> ac = abs_coeff ? std::vector<double>(abs_coeff, abs_coeff + n_filt) : std::vector<double>();
        const std::vector<double> v = b9h::offset_direction(spec, strings(filters, n_filt), ac);
        std::copy(v.begin(), v.end(), k);
    });
}

int b9h_offset_table(const double *star_off, const double *sigma, const double *k, const double *tau, long n_stars, int n_filt, int n_dir, double *table)
{
    return guard([&] {
        if (n_stars < 0 || n_filt < 1 || n_dir < 1 || !k || !tau || !table || (n_stars > 0 && (!star_off || !sigma)))
            throw std::runtime_error("b9h_offset_table: invalid argument");
        b9h::offset_table(star_off, sigma, k, tau, n_stars, n_filt, n_dir, table);
    });
}

int b9h_offset_dist_table(const double *row_off, long n_rows, int n_dir, double *table)
{
    return guard([&] {
        if (n_rows < 0 || n_dir < 1 || !table || (n_rows > 0 && !row_off)) throw std::runtime_error("b9h_offset_dist_table: invalid argument");
        b9h::offset_dist_table(row_off, n_rows, n_dir, table);
    });
}

int b9h_write_star_offsets(const char *path, const char *const *ids, long n_stars, const char *const *directions, int n_dir, const double *table)
{
    return guard([&] {
        if (!path || n_stars < 0 || n_dir < 1 || !directions || (n_stars > 0 && (!ids || !table))) throw std::runtime_error("b9h_write_star_offsets: invalid argument");
        b9h::write_star_offsets(path, strings(ids, n_stars), strings(directions, n_dir), table);
    });
}

int b9h_write_offset_dist(const char *path, const char *const *directions, int n_dir, const double *table)
{
    return guard([&] {
        if (!path || n_dir < 1 || !directions || !table) throw std::runtime_error("b9h_write_offset_dist: invalid argument");
        b9h::write_offset_dist(path, strings(directions, n_dir), table);
    });
}

int b9h_star_offsets_settings(int argc, char **argv, char *out, int cap)
{
    return settings_text("b9h_star_offsets_settings", argc, argv, b9h::kStarOffsetsFlags, out, cap, [&](const b9h::Settings &st) {
        const b9h::StarOffsetsConfig c = b9h::star_offsets_config(st);
        std::string dirs, taus;
        char buf[40];
        for (size_t j = 0; j < c.directions.size(); ++j) {
            std::snprintf(buf, sizeof buf, "%.17g", c.tau[j]);
            dirs += (j ? " " : "") + c.directions[j];
            taus += (j ? " " : "") + std::string(buf);
        }
        return grid_text(b9h::chain_grid(st, "starOffsets")) + "direction = " + dirs + "\ntau = " + taus + "\n";
    });
}

int b9h_phot_resid_settings(int argc, char **argv, char *out, int cap)
{
    return settings_text("b9h_phot_resid_settings", argc, argv, b9h::kPhotResidFlags, out, cap, [&](const b9h::Settings &st) {
        return grid_text(b9h::chain_grid(st, "photResiduals")) + "perStar = " + std::to_string((int)b9h::phot_resid_config(st).per_star) + "\n";
    });
}

int b9h_pointwise_table(const double *acc, const double *tail, int tail_len, long n_stars, double *table)
{
    return guard([&] {
        if (n_stars < 0 || !table || tail_len < 0 || (n_stars > 0 && !acc)) throw std::runtime_error("b9h_pointwise_table: invalid argument");
        b9h::pointwise_table(acc, tail_len > 0 ? tail : nullptr, tail_len, n_stars, table);
    });
}

int b9h_score_totals(const double *table, long n_stars, double *totals)
{
    return guard([&] {
        if (n_stars < 0 || !totals || (n_stars > 0 && !table)) throw std::runtime_error("b9h_score_totals: invalid argument");
        b9h::score_totals(table, n_stars, totals);
    });
}

int b9h_score_compare(const double *table_a, const char *const *ids_a, long n_a, const double *table_b, const char *const *ids_b, long n_b, double *out)
{
    return guard([&] {
        if (n_a < 0 || n_b < 0 || !out || (n_a > 0 && (!table_a || !ids_a)) || (n_b > 0 && (!table_b || !ids_b)))
            throw std::runtime_error("b9h_score_compare: invalid argument");
        b9h::score_compare(table_a, strings(ids_a, n_a), table_b, strings(ids_b, n_b), out);
    });
}

int b9h_write_pointwise(const char *path, const char *const *ids, long n_stars, const double *table)
{
    return guard([&] {
        if (!path || n_stars < 0 || (n_stars > 0 && (!ids || !table))) throw std::runtime_error("b9h_write_pointwise: invalid argument");
        b9h::write_pointwise(path, strings(ids, n_stars), table);
    });
}

int b9h_write_model_score(const char *path, const double *totals)
{
    return guard([&] {
        if (!path || !totals) throw std::runtime_error("b9h_write_model_score: invalid argument");
        b9h::write_model_score(path, totals);
    });
}

int b9h_model_score_settings(int argc, char **argv, char *out, int cap)
{
    return settings_text("b9h_model_score_settings", argc, argv, b9h::kModelScoreFlags, out, cap, [&](const b9h::Settings &st) {
        const b9h::ModelScoreConfig c = b9h::model_score_config(st);
        return grid_text(b9h::chain_grid(st, "modelScore")) + "perRow = " + std::to_string((int)c.per_row) + "\ncompareTo = " + c.compare_to + "\n";
    });
}

int b9h_influence_table(const double *acc, const double *tail, int tail_len, long n_stars, int n_q, double *table)
{
    return guard([&] {
        if (n_stars < 0 || !table || tail_len < 0 || n_q < 1 || n_q > B9_INF_MAX_Q || (n_stars > 0 && !acc)) throw std::runtime_error("b9h_influence_table: invalid argument");
        b9h::influence_table(acc, tail_len > 0 ? tail : nullptr, tail_len, n_stars, n_q, table);
    });
}

int b9h_group_influence_table(const double *group_lpd, long n_rows, int n_groups, const double *q, int n_q, const int32_t *group, long n_stars, double *table)
{
    return guard([&] {
        if (n_rows < 0 || n_groups < 1 || n_groups > B9_INF_MAX_GROUPS || n_q < 1 || n_q > B9_INF_MAX_Q || n_stars < 0 || !table || (n_rows > 0 && (!group_lpd || !q)) ||
            (n_stars > 0 && !group))
            throw std::runtime_error("b9h_group_influence_table: invalid argument");
        b9h::group_influence_table(group_lpd, n_rows, n_groups, q, n_q, group, n_stars, table);
    });
}

int b9h_influence_quantities(int argc, char **argv, const double *rows, const double *log_post, long n_rows, char *names, int cap, double *q, double *mean, double *sd,
                             int *n_q)
{
    return guard([&] {
        if (!rows || !names || !q || !mean || !sd || !n_q) throw std::runtime_error("b9h_influence_quantities: invalid argument");
        b9h::Settings st;
        st.parse_args(argc, argv, b9h::kStarInfluenceFlags);
        const b9h::InfluenceQuantities iq = b9h::influence_quantities(b9h::star_influence_config(st), rows, log_post, n_rows);
        std::string joined;
        for (size_t j = 0; j < iq.names.size(); ++j) joined += (j ? " " : "") + iq.names[j];
        if ((int)joined.size() + 1 > cap) throw std::runtime_error("b9h_influence_quantities: the names do not fit");
        std::copy(joined.begin(), joined.end(), names); names[joined.size()] = 0;
        std::copy(iq.q.begin(), iq.q.end(), q); std::copy(iq.mean.begin(), iq.mean.end(), mean); std::copy(iq.sd.begin(), iq.sd.end(), sd);
        *n_q = (int)iq.names.size();
    });
}

int b9h_influence_groups(int argc, char **argv, const char *const *ids, const int32_t *stage, long n_stars, char *names, int cap, int32_t *group, int *n_groups)
{
    return guard([&] {
        if (n_stars < 0 || !names || !n_groups || (n_stars > 0 && (!ids || !stage || !group))) throw std::runtime_error("b9h_influence_groups: invalid argument");
        b9h::Settings st;
        st.parse_args(argc, argv, b9h::kStarInfluenceFlags);
        const b9h::InfluenceGroups g = b9h::influence_groups(b9h::star_influence_config(st), strings(ids, n_stars), std::vector<int32_t>(stage, stage + n_stars));
        std::string joined;
        for (size_t j = 0; j < g.names.size(); ++j) joined += (j ? " " : "") + g.names[j];
        if ((int)joined.size() + 1 > cap) throw std::runtime_error("b9h_influence_groups: the names do not fit");
        std::copy(joined.begin(), joined.end(), names); names[joined.size()] = 0;
        std::copy(g.id.begin(), g.id.end(), group);
        *n_groups = (int)g.names.size();
    });
}

int b9h_write_star_influence(const char *path, const char *const *ids, long n_stars, const char *const *quantities, int n_q, const double *table)
{
    return guard([&] {
        if (!path || n_stars < 0 || n_q < 1 || !quantities || (n_stars > 0 && (!ids || !table))) throw std::runtime_error("b9h_write_star_influence: invalid argument");
        b9h::write_star_influence(path, strings(ids, n_stars), strings(quantities, n_q), table);
    });
}

int b9h_write_group_influence(const char *path, const char *const *groups, int n_groups, const char *const *quantities, int n_q, const double *table)
{
    return guard([&] {
        if (!path || n_groups < 1 || n_q < 1 || !groups || !quantities || !table) throw std::runtime_error("b9h_write_group_influence: invalid argument");
        b9h::write_group_influence(path, strings(groups, n_groups), strings(quantities, n_q), table);
    });
}

int b9h_star_influence_settings(int argc, char **argv, char *out, int cap)
{
    return settings_text("b9h_star_influence_settings", argc, argv, b9h::kStarInfluenceFlags, out, cap, [&](const b9h::Settings &st) {
        const b9h::StarInfluenceConfig c = b9h::star_influence_config(st);
        std::string qs;
        for (size_t j = 0; j < c.quantities.size(); ++j) qs += (j ? " " : "") + c.quantities[j];
        return grid_text(b9h::chain_grid(st, "starInfluence")) + "quantity = " + qs + "\ngroupFile = " + c.group_file + "\nnoGroups = " + std::to_string((int)c.no_groups) + "\n";
    });
}

int b9h_merge_parts(const char *final_path, int world, int walkers_per_rank, long rows_per_part)
{
    return guard([&] { b9h::merge_result_parts(final_path, world, walkers_per_rank, rows_per_part); });
}

// ---- ranks, exchange ---------------------------------------------------------------------------------------------
void b9h_rank_from_env(int *rank, int *world, int *local_rank) { b9h::rank_from_env(*rank, *world, *local_rank); }

int b9h_device_synchronize(void)
{
    return guard([&] { if (hipDeviceSynchronize() != hipSuccess) throw std::runtime_error("hipDeviceSynchronize failed"); });
}

int b9h_exchange_local(void **out) { return guard([&] { *out = b9h::make_local_exchange().release(); }); }
int b9h_exchange_rccl(int rank, int world, const char *dir, int device, void **out)
{
    return guard([&] { *out = b9h::make_rccl_exchange(rank, world, dir && *dir ? std::string(dir) : b9h::default_bootstrap_dir(), device).release(); });
}
int b9h_exchange_callback(b9h_gather_fn gather, void *user, int rank, int world, void **out)
{
    return guard([&] { *out = b9h::make_callback_exchange(gather, user, rank, world).release(); });
}
void b9h_exchange_free(void *e) { delete static_cast<b9h::Exchange *>(e); }
int b9h_exchange_barrier(void *e) { return guard([&] { static_cast<b9h::Exchange *>(e)->barrier(); }); }
int b9h_exchange_max(void *e, double v, double *out) { return guard([&] { *out = static_cast<b9h::Exchange *>(e)->all_reduce_max(v); }); }
int b9h_exchange_world(void *e) { return static_cast<b9h::Exchange *>(e)->world(); }
const char *b9h_exchange_name(void *e) { return static_cast<b9h::Exchange *>(e)->name(); }
int b9h_exchange_comm_ranks(void *e) { return static_cast<b9h::Exchange *>(e)->comm_ranks(); }
int b9h_exchange_devices(void *e, char *out, int cap)
{
    const std::string d = static_cast<b9h::Exchange *>(e)->devices();
    if (!out || cap < 1 || (int)d.size() + 1 > cap) return -1;
    std::memcpy(out, d.c_str(), d.size() + 1);
    return 0;
}
int b9h_forced_ranks(void) { return b9h::forced_ranks() ? 1 : 0; }
int b9h_group_check(int world, int comm_ranks, const char *devices_csv, char *msg, int cap)
{
    const std::string bad = b9h::group_error(world, comm_ranks, devices_csv ? devices_csv : "");
    if (msg && cap > 0) { std::strncpy(msg, bad.c_str(), (size_t)cap - 1); msg[cap - 1] = '\0'; }
    return bad.empty() ? 0 : 1;
}
void b9h_test_stall(const char *where, int rank) { b9h::test_stall(where, rank); }

// ---- sampler --------------------------------------------------------------------------------------------------------
namespace {
struct SamplerBox {
    std::unique_ptr<b9h::BlockRunner> runner;
    std::unique_ptr<b9h::WalkerSampler> sampler;
};
b9h::SamplerConfig make_config(int n_walkers, const int32_t *free_idx, const double *step, int d, uint64_t seed, int block)
{
    b9h::SamplerConfig c;
    c.n_walkers = n_walkers; c.free_idx.assign(free_idx, free_idx + d); c.step.assign(step, step + d); c.seed = seed; c.block = block;
    return c;
}
std::vector<int32_t> local_ids(int n_walkers, b9h::Exchange *ex)
{
    if (n_walkers < 1 || n_walkers % ex->world()) throw std::runtime_error("the number of walkers must be a multiple of the number of ranks");
    const int per = n_walkers / ex->world();
    std::vector<int32_t> ids(per);
    for (int k = 0; k < per; ++k) ids[k] = ex->rank() * per + k;
    return ids;
}
}  // namespace

int b9h_sampler_create(b9_ctx *ctx, int mode, int n_walkers, const int32_t *free_idx, const double *step, int d, uint64_t seed,
                       int block, void *exchange, void **out)
{
    return guard([&] {
        auto *ex = static_cast<b9h::Exchange *>(exchange);
        const b9h::SamplerConfig cfg = make_config(n_walkers, free_idx, step, d, seed, block);
        const std::vector<int32_t> ids = local_ids(n_walkers, ex);
        auto box = std::make_unique<SamplerBox>();
        box->runner = b9h::make_device_runner(ctx, (int)ids.size(), ids, cfg.free_idx, seed, mode);
        box->sampler = std::make_unique<b9h::WalkerSampler>(cfg, box->runner.get(), ex);
        *out = box.release();
    });
}
int b9h_sampler_create_callback(b9h_block_fn run, b9h_logpost_fn eval, void *user, int n_walkers, const int32_t *free_idx,
                                const double *step, int d, uint64_t seed, int block, void *exchange, void **out)
{
    return guard([&] {
        auto *ex = static_cast<b9h::Exchange *>(exchange);
        const b9h::SamplerConfig cfg = make_config(n_walkers, free_idx, step, d, seed, block);
        const std::vector<int32_t> ids = local_ids(n_walkers, ex);
        auto box = std::make_unique<SamplerBox>();
        box->runner = b9h::make_callback_runner(run, eval, user, (int)ids.size(), ids, cfg.free_idx, seed);
        box->sampler = std::make_unique<b9h::WalkerSampler>(cfg, box->runner.get(), ex);
        *out = box.release();
    });
}
void b9h_sampler_free(void *s) { delete static_cast<SamplerBox *>(s); }
int b9h_sampler_initialise(void *s, const double *start) { return guard([&] { static_cast<SamplerBox *>(s)->sampler->initialise(start); }); }
int b9h_sampler_run(void *s, int64_t n_steps, int adapt, double *samples, double *lps)
{
    return guard([&] {
        b9h::WalkerSampler &sm = *static_cast<SamplerBox *>(s)->sampler;
        const long first = sm.steps();
        b9h::RecordFn rec;
        if (samples || lps)
            rec = [&](const b9h::BlockRecord &r) {
                const size_t row = (size_t)(r.step0 - first) * r.n_local;
                if (samples) std::memcpy(samples + row * r.d, r.samples, sizeof(double) * (size_t)r.n_steps * r.n_local * r.d);
                if (lps) std::memcpy(lps + row, r.lps, sizeof(double) * (size_t)r.n_steps * r.n_local);
            };
        sm.run((long)n_steps, adapt != 0, rec);
    });
}
int b9h_sampler_n_local(void *s) { return static_cast<SamplerBox *>(s)->sampler->n_local(); }
int b9h_sampler_state(void *s, int64_t *steps, int64_t *accepted_local, double *scale, double *chol, double *all_params, double *all_logpost)
{
    return guard([&] {
        const b9h::WalkerSampler &sm = *static_cast<SamplerBox *>(s)->sampler;
        if (steps) *steps = sm.steps();
        if (accepted_local) *accepted_local = sm.accepted_local();
        if (scale) *scale = sm.scale();
        if (chol) std::copy(sm.chol().begin(), sm.chol().end(), chol);
        if (all_params) std::copy(sm.all_params().begin(), sm.all_params().end(), all_params);
        if (all_logpost) std::copy(sm.all_logpost().begin(), sm.all_logpost().end(), all_logpost);
    });
}
int b9h_summary_rows(const double *samples, const double *params_end, const double *logpost_end, int n_steps, int n_local, int d,
                     const double *origin, double *rows)
{
    return guard([&] { b9h::summary_rows(samples, params_end, logpost_end, n_steps, n_local, d, origin, rows); });
}

}  // extern "C"
