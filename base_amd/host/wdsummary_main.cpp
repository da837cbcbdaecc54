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
            const long n_pops = peek.integer("wdSummary.nPops", 1);
            if (n_pops != 1 && n_pops != 2) throw std::runtime_error("wdSummary.nPops must be 1 or 2");
            b9h::open_session(s, argc, argv, (int)n_pops, true);
        }
        const int n_pops = (int)s.settings.integer("wdSummary.nPops", 1);
        const long nodes = s.settings.integer("wdSummary.nMassNodes", s.settings.integer("sampleWDMass.nMassNodes", 512));
        if (nodes < 1 || nodes > 2147483647l) throw std::runtime_error("nMassNodes must be a positive 32-bit number");
        const int n_wd = b9_n_wd_stars(s.ctx);
        if (n_wd < 0) throw std::runtime_error(b9_last_error(s.ctx));
        if (n_wd == 0) throw std::runtime_error("the photometry holds no WD-stage star (stage 3): nothing to summarise");
        std::vector<std::string> ids;
        for (int i = 0; i < s.phot.n_stars(); ++i) if (s.phot.stage[i] == B9_STAGE_WD) ids.push_back(s.phot.ids[i]);
        if ((int)ids.size() != n_wd) throw std::runtime_error("the staged catalogue and the photometry disagree on the WD-stage stars");

        const std::string res_path = s.output_base + ".res";
        const std::vector<double> rows = b9h::read_res_rows(res_path, s.start, 3);
        const long n_rows = (long)(rows.size() / B9_NPARAM);
        if (n_rows == 0) throw std::runtime_error(res_path + " holds no main-run (stage 3) rows");

        std::vector<double> acc((size_t)n_wd * B9_WDM_N, 0.0);
        const long batch = 256;
        const auto t0 = std::chrono::steady_clock::now();
        for (long r0 = 0; r0 < n_rows; r0 += batch) {
            const long m = std::min(batch, n_rows - r0);
            if (b9_wd_moments(s.ctx, rows.data() + (size_t)r0 * B9_NPARAM, (int32_t)m, (int32_t)nodes, r0 ? B9_WDM_CONTINUE : 0, acc.data()) != B9_OK)
                throw std::runtime_error(b9_last_error(s.ctx));
        }
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const std::string out = s.output_base + ".wdSummary";
        b9h::write_wd_summary(out, ids, acc.data(), n_pops);
        std::fprintf(stderr, "wdSummary: %ld chain rows x %d WD-stage stars (%ld mass nodes) in %.3f s (%.3e node evaluations/s) -> %s\n",
                     n_rows, n_wd, nodes, sec, (double)n_rows * n_wd * (double)nodes * n_pops / sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("wdSummary", e);
    }
}
