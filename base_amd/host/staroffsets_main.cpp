// starOffsets -- which stars sit behind more (or less) dust than the cluster, or in front of or behind it: per star and direction
// the posterior mean and spread of an offset of the star's own along a fixed direction in magnitude space, its significance and
// the log Bayes factor of "this star has an offset of its own" against "it has none"; per direction the distribution of those
// over the chain.  Takes the settings of the fit that wrote <outputFileBase>.res, as photResiduals does, and feeds its main-run
// rows in batches to b9_star_offset: predicted magnitudes are linear in the modulus and in A_V, so the offset integrates out of
// every node of the marginalisation grid analytically; no draws, nothing left to Monte-Carlo error.  Writes
//   <outputFileBase>.starOffsets   one header line, then one line per star in .phot order:
//                                  id rows member {mean sd z logBF per direction}
//   <outputFileBase>.offsetDist    one header line, then one line per direction:  direction nRows {mean rms logBF}_{mean sd p16 p50 p84}
// (docs/FORMATS.md).
// Settings: starOffsets.{margIsoIncrem, nMassRatios} (default: sampleMass's, 4 each), starOffsets.nPops, starOffsets.direction
// (--direction, repeatable: absorption | distance | filter:NAME | v0,v1,..; default absorption and distance), starOffsets.tau
// (--tau, one for all or one per direction, mag; default 0.1).
#include "cli_common.hpp"

#include <algorithm>
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        s.settings.parse_args(argc, argv, b9h::kStarOffsetsFlags);
        const b9h::ChainGrid g = b9h::chain_grid(s.settings, "starOffsets");
        const b9h::StarOffsetsConfig c = b9h::star_offsets_config(s.settings);
        const b9h::SavedChain chain = b9h::open_saved_chain(s, g);
        const long n_rows = chain.n_rows;

        const int n = s.phot.n_stars(), nf = (int)s.phot.filters.size(), nd = (int)c.directions.size();
        std::vector<double> k;
        for (const std::string &spec : c.directions) {
            const std::vector<double> kd = b9h::offset_direction(spec, s.phot.filters, s.pack.abs_coeff);
            k.insert(k.end(), kd.begin(), kd.end());
        }
        const size_t ncol = 2 + 3 * (size_t)nd, nrow = 1 + 4 * (size_t)nd;
        std::vector<double> star_off((size_t)n * ncol, 0.0), row_off((size_t)n_rows * nrow, 0.0);
        const double sec = b9h::for_row_batches(n_rows, [&](long r0, long m) {
            if (b9_star_offset(s.ctx, chain.row(r0), (int32_t)m, r0 ? B9_OFF_CONTINUE : 0, nd, k.data(), c.tau.data(), star_off.data(),
                               row_off.data() + (size_t)r0 * nrow) != B9_OK)
                throw std::runtime_error(b9_last_error(s.ctx));
        });
        std::vector<double> stab((size_t)n * (2 + 4 * (size_t)nd)), dtab((size_t)nd * b9h::kOffsetDistCols);
        b9h::offset_table(star_off.data(), s.phot.sigma.data(), k.data(), c.tau.data(), n, nf, nd, stab.data());
        b9h::offset_dist_table(row_off.data(), n_rows, nd, dtab.data());
        const std::string out = s.output_base + ".starOffsets";
        b9h::write_star_offsets(out, s.phot.ids, c.directions, stab.data());
        b9h::write_offset_dist(s.output_base + ".offsetDist", c.directions, dtab.data());
        std::fprintf(stderr, "starOffsets: %ld chain rows x %d stars x %d directions (%d x %d mass / mass-ratio nodes per EEP interval) in %.3f s (%.3e star rows/s) -> %s\n",
                     n_rows, n, nd, g.K, g.Q, sec, (double)n_rows * n / sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("starOffsets", e);
    }
}
