// starIntervals -- every star's median and credible intervals of its mass, from a saved chain.  Re-reads the cluster chain that
// singlePopMcmc wrote to <outputFileBase>.res, as massFunction does, and loops b9_star_bins over its main-run rows: each pass
// bins every star's node weights exactly on the GPU on that star's OWN edges -- no draws --, and the host narrows each star's
// edges around its own quantile levels (b9h::refine_star_edges) until every level sits in a bracket that is final.  Writes
//   <outputFileBase>.starIntervals   one header line, then one line per star in .phot order:
//                                    id member {q<level> q<level>_lo q<level>_hi} passes flags
// Flags: [--quantity primary|secondary|system] [--levels a,b,..] [--tol t] [--maxPasses n] [--nPops n]
// Settings: starIntervals.{quantity, levels, tol, maxPasses} (default: the primary mass at 0.025, 0.16, 0.5, 0.84, 0.975, 1e-4
//           relative, 12 passes), starIntervals.margIsoIncrem / nMassRatios (default: sampleMass's, 4 each), starIntervals.nPops.
#include "cli_common.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        s.settings.parse_args(argc, argv, b9h::kStarIntervalsFlags);
        const b9h::ChainGrid g = b9h::chain_grid(s.settings, "starIntervals");
        const b9h::SavedChain chain = b9h::open_saved_chain(s, g);
        const long n_rows = chain.n_rows;
        const b9h::StarIntervalsConfig c = b9h::star_intervals_config(s.settings);

        const int n = s.phot.n_stars();
        const double max_mass = std::max(*std::max_element(s.pack.mass.begin(), s.pack.mass.end()), s.pack.m_wd_up);
        int passes = 0;
        const auto t0 = std::chrono::steady_clock::now();
        const b9h::StarIntervals r = b9h::star_intervals([&](const double *edges, int n_bins, double *acc) {
            b9h::for_row_batches(n_rows, [&](long r0, long m) {
                if (b9_star_bins(s.ctx, chain.row(r0), (int32_t)m, c.quantity, edges, n_bins, r0 ? B9_SBIN_CONTINUE : 0, acc) != B9_OK)
                    throw std::runtime_error(b9_last_error(s.ctx));
            });
            ++passes;
        }, n, n_rows, B9_SBIN_MAX_BINS, max_mass, c.levels, c.tol, c.max_passes);
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::vector<double> table((size_t)n * (3 * c.levels.size() + 3));
        b9h::star_intervals_table(r, table.data());
        const std::string out = s.output_base + ".starIntervals";
        b9h::write_star_intervals(out, s.phot.ids, c.levels, table.data());
        long open = 0;
        for (int i = 0; i < n; ++i) open += (r.flags[i] & b9h::kSivOpen) != 0;
        std::fprintf(stderr, "starIntervals: %ld chain rows x %d stars x %zu levels in %d passes (%d x %d mass / mass-ratio nodes per EEP interval), %ld stars unfinished, %.3f s -> %s\n",
                     n_rows, n, c.levels.size(), passes, g.K, g.Q, open, sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("starIntervals", e);
    }
}
