// massFunction -- the cluster's mass function with its credible band, and (--perStar) every star's mass posterior, from a saved
// chain.  Re-reads the cluster chain that singlePopMcmc wrote to <outputFileBase>.res, as starSummary does, and feeds its
// main-run rows in batches to b9_mass_hist: the node weights of the marginalisation grid are binned exactly on the GPU -- no
// draws -- and come back summed over the stars per row (the expected number of members per bin under that row) and summed over
// the rows per star.  Writes
//   <outputFileBase>.massFunction   one header line, then one line per bin:  lo hi mean sd p16 p50 p84 dNdlogM
//   <outputFileBase>.starMassHist   (--perStar) one header line, then one line per star in .phot order:
//                                   id rows member bin0 .. bin<n-1>   (the posterior probabilities of the bins)
// Flags: [--nBins n] [--minMass m] [--maxMass m] [--linearBins] [--quantity primary|secondary|system] [--perStar]
// Settings: massFunction.{nBins, minMass, maxMass, linearBins, quantity, perStar} (default: 24 log-spaced bins of the primary mass
//           over [0.1, M_wd_up]), massFunction.margIsoIncrem / nMassRatios (default: sampleMass's, 4 each), massFunction.nPops.
#include "cli_common.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        const std::vector<std::string> args = b9h::mass_function_args(argc, argv);
        std::vector<char *> av;
        for (auto &a : args) av.push_back(const_cast<char *>(a.c_str()));
        b9h::Session s;
        {   // (the population count decides which starting values open_session reads: peek at the settings first)
            b9h::Settings peek;
            peek.parse_args((int)av.size(), av.data());
            const long n_pops = peek.integer("massFunction.nPops", 1);
            if (n_pops != 1 && n_pops != 2) throw std::runtime_error("massFunction.nPops must be 1 or 2");
            b9h::open_session(s, (int)av.size(), av.data(), (int)n_pops, true);
        }
        const b9h::MassFunctionConfig c = b9h::mass_function_config(s.settings, s.pack.m_wd_up);
        const std::vector<double> edges = c.edges();
        b9_options opt{B9_MODE_GIVEN_MASS, c.n_pops, c.K, c.Q};
        if (b9_set_options(s.ctx, &opt) != B9_OK) throw std::runtime_error(b9_last_error(s.ctx));

        const std::string res_path = s.output_base + ".res";
        const std::vector<double> rows = b9h::read_res_rows(res_path, s.start, 3);
        const long n_rows = (long)(rows.size() / B9_NPARAM);
        if (n_rows == 0) throw std::runtime_error(res_path + " holds no main-run (stage 3) rows");

        const int n = s.phot.n_stars();
        const size_t ncol = (size_t)c.n_bins + 1;
        std::vector<double> star_hist(c.per_star ? (size_t)n * ncol : 0, 0.0), row_hist((size_t)n_rows * ncol, 0.0);
        const long batch = 256;
        const auto t0 = std::chrono::steady_clock::now();
        for (long r0 = 0; r0 < n_rows; r0 += batch) {
            const long m = std::min(batch, n_rows - r0);
            if (b9_mass_hist(s.ctx, rows.data() + (size_t)r0 * B9_NPARAM, (int32_t)m, c.quantity, edges.data(), c.n_bins, r0 ? B9_HIST_CONTINUE : 0,
                             c.per_star ? star_hist.data() : nullptr, row_hist.data() + (size_t)r0 * ncol) != B9_OK)
                throw std::runtime_error(b9_last_error(s.ctx));
        }
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::vector<double> table((size_t)c.n_bins * b9h::kMassFunctionCols);
        b9h::mass_function_table(row_hist.data(), n_rows, edges.data(), c.n_bins, table.data());
        const std::string out = s.output_base + ".massFunction";
        b9h::write_mass_function(out, table.data(), c.n_bins);
        if (c.per_star) b9h::write_star_mass_hist(s.output_base + ".starMassHist", s.phot.ids, star_hist.data(), c.n_bins, n_rows);
        std::fprintf(stderr, "massFunction: %ld chain rows x %d stars x %d bins (%d x %d mass / mass-ratio nodes per EEP interval) in %.3f s (%.3e star rows/s) -> %s\n",
                     n_rows, n, c.n_bins, c.K, c.Q, sec, (double)n_rows * n / sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("massFunction", e);
    }
}
