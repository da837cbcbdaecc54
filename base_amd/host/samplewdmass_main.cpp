// sampleWDMass -- per-WD posterior of the ZAMS mass and what follows from it ([RECALL] BASE-9 sampleWDMass): re-reads the
// cluster chain that singlePopMcmc wrote to <outputFileBase>.res and, for every main-run (stage 3) row and every WD-stage
// star of the photometry, draws the star's ZAMS mass from its conditional posterior on a grid of nMassNodes equal steps
// between the row's AGB tip and M_wd_up, and reports the WD mass, the precursor's log-age, the log cooling age, log Teff,
// log g and the membership probability at the drawn node.  All of it is one call per batch of rows to b9_sample_wd_mass
// (include/base9_hip.h states the definition).  Writes, one line per chain row, header = ids of the WD-stage stars in
// .phot order:
//   <outputFileBase>.wd.zamsMass  .wd.mass  .wd.precLogAge  .wd.coolingAge (log10 yr)  .wd.logTeff  .wd.logg  .wd.membership
// Settings: sampleWDMass.nMassNodes (--nMassNodes, default 512: about 0.012 Msun between nodes on a 1.5 - 8 Msun range),
//           general.seed.  Single population, like sampleMass.
#include "cli_common.hpp"

#include <algorithm>
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        s.settings.parse_args(argc, argv);
        const long nodes = b9h::wd_mass_nodes(s.settings, "sampleWDMass");
        const b9h::SavedChain chain = b9h::open_saved_chain(s, {1, 0, 0});
        const long n_rows = chain.n_rows;
        const std::vector<int> wd = b9h::wd_stage_stars(s, "sample");
        const int n_wd = (int)wd.size();

        // the seven files, in the order of b9_sample_wd_mass's outputs
        static const char *const kind[7] = {"zamsMass", "mass", "precLogAge", "coolingAge", "logTeff", "logg", "membership"};
        FILE *f[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        std::string names;
        for (int k = 0; k < 7; ++k) {
            const std::string p = s.output_base + ".wd." + kind[k];
            f[k] = std::fopen(p.c_str(), "w");
            if (!f[k]) { for (int j = 0; j < k; ++j) std::fclose(f[j]); throw std::runtime_error("cannot write " + p); }
            for (int c = 0; c < n_wd; ++c) std::fprintf(f[k], "%s%s", c ? " " : "", s.phot.ids[wd[c]].c_str());
            std::fprintf(f[k], "\n");
            names += (k ? ", " : "") + p;
        }
        std::vector<double> out[7];
        for (auto &v : out) v.resize((size_t)b9h::kChainBatch * n_wd);
        const double sec = b9h::for_row_batches(n_rows, [&](long r0, long m) {
            if (b9_sample_wd_mass(s.ctx, chain.row(r0), (int32_t)m, (int32_t)nodes, s.mcmc.seed, r0, out[0].data(),
                                  out[1].data(), out[2].data(), out[3].data(), out[4].data(), out[5].data(), out[6].data(), nullptr) != B9_OK) {
                for (FILE *p : f) std::fclose(p);
                throw std::runtime_error(b9_last_error(s.ctx));
            }
            for (int k = 0; k < 7; ++k)
                for (long r = 0; r < m; ++r) {
                    for (int c = 0; c < n_wd; ++c) std::fprintf(f[k], "%s%.6f", c ? " " : "", out[k][(size_t)r * n_wd + c]);
                    std::fprintf(f[k], "\n");
                }
        });
        for (FILE *p : f) std::fclose(p);
        std::fprintf(stderr, "sampleWDMass: %ld chain rows x %d WD-stage stars (%ld mass nodes) in %.3f s (%.3e star draws/s) -> %s\n",
                     n_rows, n_wd, nodes, sec, (double)n_rows * n_wd / sec, names.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("sampleWDMass", e);
    }
}
