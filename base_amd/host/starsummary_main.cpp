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
#include <chrono>
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        {   // (the population count decides which starting values open_session reads: peek at the settings first)
            b9h::Settings peek;
            peek.parse_args(argc, argv);
            const long n_pops = peek.integer("starSummary.nPops", 1);
            if (n_pops != 1 && n_pops != 2) throw std::runtime_error("starSummary.nPops must be 1 or 2");
            b9h::open_session(s, argc, argv, (int)n_pops, true);
        }
        const int n_pops = (int)s.settings.integer("starSummary.nPops", 1);
        const int K = (int)s.settings.integer("starSummary.margIsoIncrem", s.settings.integer("sampleMass.margIsoIncrem", 4));
        const int Q = (int)s.settings.integer("starSummary.nMassRatios", s.settings.integer("sampleMass.nMassRatios", 4));
        if (K < 1 || Q < 1) throw std::runtime_error("margIsoIncrem and nMassRatios must be positive");
        b9_options opt{B9_MODE_GIVEN_MASS, n_pops, K, Q};
        if (b9_set_options(s.ctx, &opt) != B9_OK) throw std::runtime_error(b9_last_error(s.ctx));

        const std::string res_path = s.output_base + ".res";
        const std::vector<double> rows = b9h::read_res_rows(res_path, s.start, 3);
        const long n_rows = (long)(rows.size() / B9_NPARAM);
        if (n_rows == 0) throw std::runtime_error(res_path + " holds no main-run (stage 3) rows");

        const int n = s.phot.n_stars();
        std::vector<double> acc((size_t)n * B9_MOM_N, 0.0);
        const long batch = 256;
        const auto t0 = std::chrono::steady_clock::now();
        for (long r0 = 0; r0 < n_rows; r0 += batch) {
            const long m = std::min(batch, n_rows - r0);
            if (b9_star_moments(s.ctx, rows.data() + (size_t)r0 * B9_NPARAM, (int32_t)m, r0 ? B9_MOM_CONTINUE : 0, acc.data()) != B9_OK)
                throw std::runtime_error(b9_last_error(s.ctx));
        }
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const std::string out = s.output_base + ".starSummary";
        b9h::write_star_summary(out, s.phot.ids, acc.data(), n_pops);
        std::fprintf(stderr, "starSummary: %ld chain rows x %d stars (%d x %d mass / mass-ratio nodes per EEP interval) in %.3f s (%.3e star rows/s) -> %s\n",
                     n_rows, n, K, Q, sec, (double)n_rows * n / sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("starSummary", e);
    }
}
