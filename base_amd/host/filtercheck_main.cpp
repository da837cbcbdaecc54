// filterCheck -- which filter disagrees with the models, and which stars are bad in which band: per filter the members'
// leave-one-filter-out standardised residuals, reduced chi^2, zero-point offset and mean log predictive density over the chain,
// and (--perStar) per star and filter the magnitude the star's OTHER filters predict, the predictive z and the log predictive
// density of the observation.  Takes the settings of the fit that wrote <outputFileBase>.res, as photResiduals does, and feeds
// its main-run rows in batches to b9_filter_loo: every leave-out has its own weights over the marginalisation grid, from one walk
// of the node table; no draws, nothing left to Monte-Carlo error.  Writes
//   <outputFileBase>.filterCheck       one header line, then one line per filter:  filter nRows {meanZ chi2 offset lpd}_{mean sd p16 p50 p84}
//   <outputFileBase>.starFilterCheck   (--perStar) one header line, then one line per star in .phot order:
//                                      id rows member {looMag looSd resid z lpd per filter}
// (docs/FORMATS.md).
// Settings: filterCheck.{margIsoIncrem, nMassRatios} (default: sampleMass's, 4 each), filterCheck.nPops, filterCheck.perStar.
#include "cli_common.hpp"

#include <algorithm>
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        s.settings.parse_args(argc, argv, b9h::kFilterCheckFlags);
        const b9h::ChainGrid g = b9h::chain_grid(s.settings, "filterCheck");
        const b9h::FilterCheckConfig c = b9h::filter_check_config(s.settings);
        const b9h::SavedChain chain = b9h::open_saved_chain(s, g);
        const long n_rows = chain.n_rows;

        const int n = s.phot.n_stars(), nf = (int)s.phot.filters.size();
        const size_t ncol = 2 + 3 * (size_t)nf, nrow = 1 + 6 * (size_t)nf;
        std::vector<double> star_loo(c.per_star ? (size_t)n * ncol : 0, 0.0), row_loo((size_t)n_rows * nrow, 0.0);
        const double sec = b9h::for_row_batches(n_rows, [&](long r0, long m) {
            if (b9_filter_loo(s.ctx, chain.row(r0), (int32_t)m, r0 ? B9_LOO_CONTINUE : 0,
                              c.per_star ? star_loo.data() : nullptr, row_loo.data() + (size_t)r0 * nrow) != B9_OK)
                throw std::runtime_error(b9_last_error(s.ctx));
        });
        std::vector<double> ftab((size_t)nf * b9h::kFilterCheckCols);
        b9h::filter_loo_table(row_loo.data(), n_rows, nf, ftab.data());
        const std::string out = s.output_base + ".filterCheck";
        b9h::write_filter_check(out, s.phot.filters, ftab.data());
        if (c.per_star) {
            std::vector<double> stab((size_t)n * (2 + 5 * (size_t)nf));
            b9h::loo_table(star_loo.data(), s.phot.obs.data(), s.phot.sigma.data(), n, nf, stab.data());
            b9h::write_star_filter_check(s.output_base + ".starFilterCheck", s.phot.ids, s.phot.filters, stab.data());
        }
        std::fprintf(stderr, "filterCheck: %ld chain rows x %d stars x %d filters (%d x %d mass / mass-ratio nodes per EEP interval) in %.3f s (%.3e star rows/s) -> %s\n",
                     n_rows, n, nf, g.K, g.Q, sec, (double)n_rows * n / sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("filterCheck", e);
    }
}
