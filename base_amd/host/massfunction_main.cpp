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
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        s.settings.parse_args(argc, argv, b9h::kMassFunctionFlags);
        const b9h::ChainGrid g = b9h::chain_grid(s.settings, "massFunction");
        const b9h::SavedChain chain = b9h::open_saved_chain(s, g);
        const long n_rows = chain.n_rows;
        const b9h::MassFunctionConfig c = b9h::mass_function_config(s.settings, s.pack.m_wd_up);
        const std::vector<double> edges = c.edges();

        const int n = s.phot.n_stars();
        const size_t ncol = (size_t)c.n_bins + 1;
        std::vector<double> star_hist(c.per_star ? (size_t)n * ncol : 0, 0.0), row_hist((size_t)n_rows * ncol, 0.0);
        const double sec = b9h::for_row_batches(n_rows, [&](long r0, long m) {
            if (b9_mass_hist(s.ctx, chain.row(r0), (int32_t)m, c.quantity, edges.data(), c.n_bins, r0 ? B9_HIST_CONTINUE : 0,
                             c.per_star ? star_hist.data() : nullptr, row_hist.data() + (size_t)r0 * ncol) != B9_OK)
                throw std::runtime_error(b9_last_error(s.ctx));
        });
        std::vector<double> table((size_t)c.n_bins * b9h::kMassFunctionCols);
        b9h::mass_function_table(row_hist.data(), n_rows, edges.data(), c.n_bins, table.data());
        const std::string out = s.output_base + ".massFunction";
        b9h::write_mass_function(out, table.data(), c.n_bins);
        if (c.per_star) b9h::write_star_mass_hist(s.output_base + ".starMassHist", s.phot.ids, star_hist.data(), c.n_bins, n_rows);
        std::fprintf(stderr, "massFunction: %ld chain rows x %d stars x %d bins (%d x %d mass / mass-ratio nodes per EEP interval) in %.3f s (%.3e star rows/s) -> %s\n",
                     n_rows, n, c.n_bins, g.K, g.Q, sec, (double)n_rows * n / sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("massFunction", e);
    }
}
