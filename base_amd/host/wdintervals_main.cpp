// wdIntervals -- every WD-stage star's median and credible intervals of its ZAMS mass, WD mass, precursor log-age, log cooling
// age, log Teff and log g, from a saved chain.  Re-reads the cluster chain that singlePopMcmc wrote to <outputFileBase>.res, as
// wdSummary does; one b9_wd_moments pass over its main-run rows gives every line (star, quantity) its first range, then
// b9_wd_bins is looped over the rows: each pass bins the node weights of the nMassNodes grid exactly on the GPU on every line's
// OWN edges -- no draws --, and the host narrows each line's edges around its own quantile levels (b9h::refine_star_edges) until
// every level sits in a bracket that is final.  Writes
//   <outputFileBase>.wdIntervals   one header line, then one line per WD-stage star in .phot order:
//                                  id member {N_counted {N_q<level> N_q<level>_lo N_q<level>_hi} N_passes N_flags}
//                                  for N in the selected ones of zamsMass wdMass precLogAge logCoolAge logTeff logg
// Flags: [--quantities zamsMass,wdMass,..] [--levels a,b,..] [--tol t] [--maxPasses n] [--nMassNodes n] [--nPops n]
// Settings: wdIntervals.{quantities, levels, tol, maxPasses} (default: all six at 0.025, 0.16, 0.5, 0.84, 0.975, 1e-4 relative,
//           12 passes), wdIntervals.nMassNodes (default: wdSummary's, then sampleWDMass's, then 512), wdIntervals.nPops.
#include "cli_common.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        s.settings.parse_args(argc, argv, b9h::kWdIntervalsFlags);
        const int n_pops = b9h::chain_n_pops(s.settings, "wdIntervals");
        const b9h::WdIntervalsConfig c = b9h::wd_intervals_config(s.settings);
        const b9h::SavedChain chain = b9h::open_saved_chain(s, {n_pops, 0, 0});
        const long n_rows = chain.n_rows;
        std::vector<std::string> ids;
        for (int i : b9h::wd_stage_stars(s, "bin")) ids.push_back(s.phot.ids[i]);
        const int n_wd = (int)ids.size(), n_sel = c.n_sel();

        int passes = 0;
        const auto t0 = std::chrono::steady_clock::now();
        const b9h::WdIntervals r = b9h::wd_intervals([&](double *acc) {
            b9h::for_row_batches(n_rows, [&](long r0, long m) {
                if (b9_wd_moments(s.ctx, chain.row(r0), (int32_t)m, (int32_t)c.n_nodes, r0 ? B9_WDM_CONTINUE : 0, acc) != B9_OK)
                    throw std::runtime_error(b9_last_error(s.ctx));
            });
        }, [&](const double *edges, int n_bins, double *acc) {
            b9h::for_row_batches(n_rows, [&](long r0, long m) {
                if (b9_wd_bins(s.ctx, chain.row(r0), (int32_t)m, (int32_t)c.n_nodes, c.quantity_mask, edges, n_bins, r0 ? B9_WBIN_CONTINUE : 0, acc) != B9_OK)
                    throw std::runtime_error(b9_last_error(s.ctx));
            });
            ++passes;
        }, n_wd, n_rows, c.quantity_mask, c.levels, c.tol, c.max_passes);
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::vector<double> table((size_t)n_wd * (1 + (size_t)n_sel * (3 * c.levels.size() + 3)));
        b9h::wd_intervals_table(r, table.data());
        const std::string out = s.output_base + ".wdIntervals";
        b9h::write_wd_intervals(out, ids, c.quantity_mask, c.levels, table.data());
        long open = 0;
        for (long l = 0; l < (long)n_wd * n_sel; ++l) open += (r.lines.flags[l] & b9h::kSivOpen) != 0;
        std::fprintf(stderr, "wdIntervals: %ld chain rows x %d WD-stage stars x %d quantities x %zu levels in %d passes (%ld mass nodes), %ld lines unfinished, %.3f s -> %s\n",
                     n_rows, n_wd, n_sel, c.levels.size(), passes, c.n_nodes, open, sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("wdIntervals", e);
    }
}
