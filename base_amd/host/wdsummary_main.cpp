// wdSummary -- the per-WD answer of a saved chain: for every WD-stage star of the photometry its membership probability and the
// posterior mean and standard deviation of its ZAMS mass, WD mass, precursor log-age, log cooling age, log Teff and log g.
// Re-reads the cluster chain that singlePopMcmc wrote to <outputFileBase>.res, as sampleWDMass does, and feeds its main-run rows
// in batches to b9_wd_moments: the conditional expectations over the grid of nMassNodes equal steps between the row's AGB tip
// and M_wd_up are formed exactly on the GPU, weighted by membership, and only their sums over the rows come back -- no draws,
// no [rows][stars] files.  Writes
//   <outputFileBase>.wdSummary   one header line, then one line per WD-stage star in .phot order:
//                                id rows member pCooled zamsMass zamsMassSd wdMass wdMassSd precLogAge precLogAgeSd
//                                logCoolAge logCoolAgeSd logTeff logTeffSd logg loggSd [pPop2]
// Settings: wdSummary.nMassNodes (--nMassNodes; default: sampleWDMass.nMassNodes, else 512),
//           wdSummary.nPops (1, or 2 for a multiPopMcmc chain).
#include "cli_common.hpp"

#include <algorithm>
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        s.settings.parse_args(argc, argv);
        const int n_pops = b9h::chain_n_pops(s.settings, "wdSummary");
        const long nodes = b9h::wd_mass_nodes(s.settings, "wdSummary");
        const b9h::SavedChain chain = b9h::open_saved_chain(s, {n_pops, 0, 0});
        const long n_rows = chain.n_rows;
        std::vector<std::string> ids;
        for (int i : b9h::wd_stage_stars(s, "summarise")) ids.push_back(s.phot.ids[i]);
        const int n_wd = (int)ids.size();

        std::vector<double> acc((size_t)n_wd * B9_WDM_N, 0.0);
        const double sec = b9h::for_row_batches(n_rows, [&](long r0, long m) {
            if (b9_wd_moments(s.ctx, chain.row(r0), (int32_t)m, (int32_t)nodes, r0 ? B9_WDM_CONTINUE : 0, acc.data()) != B9_OK)
                throw std::runtime_error(b9_last_error(s.ctx));
        });
        const std::string out = s.output_base + ".wdSummary";
        b9h::write_wd_summary(out, ids, acc.data(), n_pops);
        std::fprintf(stderr, "wdSummary: %ld chain rows x %d WD-stage stars (%ld mass nodes) in %.3f s (%.3e node evaluations/s) -> %s\n",
                     n_rows, n_wd, nodes, sec, (double)n_rows * n_wd * (double)nodes * n_pops / sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("wdSummary", e);
    }
}
