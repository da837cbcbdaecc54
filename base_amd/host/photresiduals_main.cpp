// photResiduals -- is the fit any good, and where does it fail: per filter the members' standardised residuals, reduced chi^2 and
// zero-point offset with their spread over the chain, and (--perStar) for every star the magnitudes the posterior predicts in
// every filter next to the observed ones.  Re-reads the cluster chain that singlePopMcmc wrote to <outputFileBase>.res, as
// massFunction does, and feeds its main-run rows in batches to b9_phot_resid: the node magnitudes of the marginalisation grid
// are averaged exactly on the GPU -- no draws -- and come back summed over the stars per row and summed over the rows per star.
// Writes
//   <outputFileBase>.filterResid   one header line, then one line per filter:  filter nRows {meanZ chi2 offset}_{mean sd p16 p50 p84}
//   <outputFileBase>.photResid     (--perStar) one header line, then one line per star in .phot order:
//                                  id rows member {predMag predSd resid rmsZ per filter}
// Flags: [--perStar] [--nPops n] [--margIsoIncrem k] [--nMassRatios q]
// Settings: photResiduals.{margIsoIncrem, nMassRatios} (default: sampleMass's, 4 each), photResiduals.nPops, photResiduals.perStar.
#include "cli_common.hpp"

#include <algorithm>
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        s.settings.parse_args(argc, argv, b9h::kPhotResidFlags);
        const b9h::ChainGrid g = b9h::chain_grid(s.settings, "photResiduals");
        const b9h::PhotResidConfig c = b9h::phot_resid_config(s.settings);
        const b9h::SavedChain chain = b9h::open_saved_chain(s, g);
        const long n_rows = chain.n_rows;

        const int n = s.phot.n_stars(), nf = (int)s.phot.filters.size();
        const size_t ncol = 2 + 2 * (size_t)nf, nrow = 1 + 5 * (size_t)nf;
        std::vector<double> star_resid(c.per_star ? (size_t)n * ncol : 0, 0.0), row_resid((size_t)n_rows * nrow, 0.0);
        const double sec = b9h::for_row_batches(n_rows, [&](long r0, long m) {
            if (b9_phot_resid(s.ctx, chain.row(r0), (int32_t)m, r0 ? B9_RESID_CONTINUE : 0,
                              c.per_star ? star_resid.data() : nullptr, row_resid.data() + (size_t)r0 * nrow) != B9_OK)
                throw std::runtime_error(b9_last_error(s.ctx));
        });
        std::vector<double> ftab((size_t)nf * b9h::kFilterResidCols);
        b9h::filter_resid_table(row_resid.data(), n_rows, nf, ftab.data());
        const std::string out = s.output_base + ".filterResid";
        b9h::write_filter_resid(out, s.phot.filters, ftab.data());
        if (c.per_star) {
            std::vector<double> stab((size_t)n * (2 + 4 * (size_t)nf));
            b9h::resid_table(star_resid.data(), s.phot.obs.data(), s.phot.sigma.data(), n, nf, stab.data());
            b9h::write_phot_resid(s.output_base + ".photResid", s.phot.ids, s.phot.filters, stab.data());
        }
        std::fprintf(stderr, "photResiduals: %ld chain rows x %d stars x %d filters (%d x %d mass / mass-ratio nodes per EEP interval) in %.3f s (%.3e star rows/s) -> %s\n",
                     n_rows, n, nf, g.K, g.Q, sec, (double)n_rows * n / sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("photResiduals", e);
    }
}
