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
        const std::vector<std::string> args = b9h::star_intervals_args(argc, argv);
        std::vector<char *> av;
        for (auto &a : args) av.push_back(const_cast<char *>(a.c_str()));
        b9h::Session s;
        {   // (the population count decides which starting values open_session reads: peek at the settings first)
            b9h::Settings peek;
            peek.parse_args((int)av.size(), av.data());
            const long n_pops = peek.integer("starIntervals.nPops", 1);
            if (n_pops != 1 && n_pops != 2) throw std::runtime_error("starIntervals.nPops must be 1 or 2");
            b9h::open_session(s, (int)av.size(), av.data(), (int)n_pops, true);
        }
        const b9h::StarIntervalsConfig c = b9h::star_intervals_config(s.settings);
        b9_options opt{B9_MODE_GIVEN_MASS, c.n_pops, c.K, c.Q};
        if (b9_set_options(s.ctx, &opt) != B9_OK) throw std::runtime_error(b9_last_error(s.ctx));

        const std::string res_path = s.output_base + ".res";
        const std::vector<double> rows = b9h::read_res_rows(res_path, s.start, 3);
        const long n_rows = (long)(rows.size() / B9_NPARAM);
        if (n_rows == 0) throw std::runtime_error(res_path + " holds no main-run (stage 3) rows");

        const int n = s.phot.n_stars();
        const double max_mass = std::max(*std::max_element(s.pack.mass.begin(), s.pack.mass.end()), s.pack.m_wd_up);
        const long batch = 256;
        int passes = 0;
        const auto t0 = std::chrono::steady_clock::now();
        const b9h::StarIntervals r = b9h::star_intervals([&](const double *edges, int n_bins, double *acc) {
            for (long r0 = 0; r0 < n_rows; r0 += batch) {
                const long m = std::min(batch, n_rows - r0);
                if (b9_star_bins(s.ctx, rows.data() + (size_t)r0 * B9_NPARAM, (int32_t)m, c.quantity, edges, n_bins, r0 ? B9_SBIN_CONTINUE : 0, acc) != B9_OK)
                    throw std::runtime_error(b9_last_error(s.ctx));
            }
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
                     n_rows, n, c.levels.size(), passes, c.K, c.Q, open, sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("starIntervals", e);
    }
}
