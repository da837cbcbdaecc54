// starSummary -- the per-star answer of a saved chain: for every star its membership probability, posterior mean and
// standard deviation of the primary mass and the mass ratio, the probability of being a binary and (two populations) of
// belonging to the second population.  Re-reads the cluster chain that singlePopMcmc wrote to <outputFileBase>.res, as sampleMass
// does, and feeds its main-run rows in batches to b9_star_moments: the conditional expectations over the marginalisation grid
// are formed exactly on the GPU and only their sums over the rows come back -- no draws, no [rows][stars] file.  Writes
//   <outputFileBase>.starSummary   one header line, then one line per star in .phot order:
//                                  id rows member mass massSd massRatio massRatioSd pBinary [pPop2]
// Settings: starSummary.margIsoIncrem / starSummary.nMassRatios (default: sampleMass's, --margIsoIncrem / --nMassRatios, 4 each),
//           starSummary.nPops (1; 2 for a multiPopMcmc chain).
#include "cli_common.hpp"

#include <algorithm>
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        s.settings.parse_args(argc, argv);
        const b9h::ChainGrid g = b9h::chain_grid(s.settings, "starSummary");
        const b9h::SavedChain chain = b9h::open_saved_chain(s, g);
        const long n_rows = chain.n_rows;

        const int n = s.phot.n_stars();
        std::vector<double> acc((size_t)n * B9_MOM_N, 0.0);
        const double sec = b9h::for_row_batches(n_rows, [&](long r0, long m) {
            if (b9_star_moments(s.ctx, chain.row(r0), (int32_t)m, r0 ? B9_MOM_CONTINUE : 0, acc.data()) != B9_OK)
                throw std::runtime_error(b9_last_error(s.ctx));
        });
        const std::string out = s.output_base + ".starSummary";
        b9h::write_star_summary(out, s.phot.ids, acc.data(), g.n_pops);
        std::fprintf(stderr, "starSummary: %ld chain rows x %d stars (%d x %d mass / mass-ratio nodes per EEP interval) in %.3f s (%.3e star rows/s) -> %s\n",
                     n_rows, n, g.K, g.Q, sec, (double)n_rows * n / sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("starSummary", e);
    }
}
