// binaryStats -- the cluster's binary fraction and mass-ratio distribution by primary mass, with their credible bands, and every
// star's posterior over the ratio nodes, from a saved chain.  Re-reads the cluster chain that singlePopMcmc wrote to
// <outputFileBase>.res, as massFunction does, and feeds its main-run rows in batches to b9_ratio_hist: the node weights of the
// marginalisation grid are summed exactly on the GPU per (primary-mass bin, mass-ratio node) -- no draws -- and come back summed
// over the stars per row and summed over the rows per star.  Writes
//   <outputFileBase>.binaryFraction  one header line, then one line per mass bin and one "all" line:
//                                    bin lo hi nRows N_{mean sd p16 p50 p84} f_{mean sd p16 p50 p84}
//   <outputFileBase>.ratioDist       one header line, then per line and ratio node: bin j q nRows mean sd p16 p50 p84
//   <outputFileBase>.starRatio       one header line, then one line per star in .phot order:
//                                    id rows member inRange pBinaryAbove q0 .. q<Q-1>
// Flags: [--massEdges e0,e1,..] | [--massBins n] [--qMin q] [--nPops n]
// Settings: binaryStats.{massEdges, massBins, qMin} (default: min(8, 128 / nMassRatios) log-spaced bins of the primary mass over
//           [0.1, M], M the larger of the models' largest mass and M_wd_up, as starIntervals takes it; qMin 0: every companion),
//           binaryStats.margIsoIncrem / nMassRatios (default: sampleMass's, 4 each), binaryStats.nPops.
#include "cli_common.hpp"

#include <algorithm>
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        s.settings.parse_args(argc, argv, b9h::kBinaryStatsFlags);
        const b9h::ChainGrid g = b9h::chain_grid(s.settings, "binaryStats");
        const b9h::SavedChain chain = b9h::open_saved_chain(s, g);
        const long n_rows = chain.n_rows;
        const double max_mass = std::max(*std::max_element(s.pack.mass.begin(), s.pack.mass.end()), s.pack.m_wd_up);
        const b9h::BinaryStatsConfig c = b9h::binary_stats_config(s.settings, max_mass, g.Q);
        const int n_mbins = c.n_mbins();

        const int n = s.phot.n_stars();
        const size_t ncol = (size_t)n_mbins * g.Q + 1;
        std::vector<double> star_cells((size_t)n * ncol, 0.0), row_cells((size_t)n_rows * ncol, 0.0);
        const double sec = b9h::for_row_batches(n_rows, [&](long r0, long m) {
            if (b9_ratio_hist(s.ctx, chain.row(r0), (int32_t)m, c.edges.data(), n_mbins, r0 ? B9_RH_CONTINUE : 0, star_cells.data(),
                              row_cells.data() + (size_t)r0 * ncol) != B9_OK)
                throw std::runtime_error(b9_last_error(s.ctx));
        });
        std::vector<double> frac((size_t)(n_mbins + 1) * b9h::kBinaryTableCols), dist((size_t)(n_mbins + 1) * g.Q * b9h::kRatioDistCols),
            per((size_t)n * (4 + (size_t)g.Q));
        b9h::binary_table(row_cells.data(), n_rows, c.edges.data(), n_mbins, g.Q, c.q_min, frac.data());
        b9h::ratio_dist_table(row_cells.data(), n_rows, n_mbins, g.Q, dist.data());
        b9h::star_ratio_table(star_cells.data(), n, n_mbins, g.Q, c.q_min, n_rows, per.data());
        const std::string out = s.output_base + ".binaryFraction";
        b9h::write_binary_fraction(out, frac.data(), n_mbins);
        b9h::write_ratio_dist(s.output_base + ".ratioDist", dist.data(), n_mbins, g.Q);
        b9h::write_star_ratio(s.output_base + ".starRatio", s.phot.ids, per.data(), g.Q);
        std::fprintf(stderr, "binaryStats: %ld chain rows x %d stars x %d mass bins x %d ratio nodes (%d x %d mass / mass-ratio nodes per EEP interval) in %.3f s (%.3e star rows/s) -> %s\n",
                     n_rows, n, n_mbins, g.Q, g.K, g.Q, sec, (double)n_rows * n / sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("binaryStats", e);
    }
}
