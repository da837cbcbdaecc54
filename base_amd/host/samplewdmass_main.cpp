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
#include <chrono>
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        b9h::open_session(s, argc, argv, 1, true);
        const long nodes = s.settings.integer("sampleWDMass.nMassNodes", 512);
        if (nodes < 1 || nodes > 2147483647l) throw std::runtime_error("nMassNodes must be a positive 32-bit number");
        const int n_wd = b9_n_wd_stars(s.ctx);
        if (n_wd < 0) throw std::runtime_error(b9_last_error(s.ctx));
        if (n_wd == 0) throw std::runtime_error("the photometry holds no WD-stage star (stage 3): nothing to sample");
        std::vector<int> wd;
        for (int i = 0; i < s.phot.n_stars(); ++i) if (s.phot.stage[i] == B9_STAGE_WD) wd.push_back(i);
        if ((int)wd.size() != n_wd) throw std::runtime_error("the staged catalogue and the photometry disagree on the WD-stage stars");

        const std::string res_path = s.output_base + ".res";
        const std::vector<double> rows = b9h::read_res_rows(res_path, s.start, 3);
        const long n_rows = (long)(rows.size() / B9_NPARAM);
        if (n_rows == 0) throw std::runtime_error(res_path + " holds no main-run (stage 3) rows");

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
        const long batch = 256;
        std::vector<double> out[7];
        for (auto &v : out) v.resize((size_t)batch * n_wd);
        const auto t0 = std::chrono::steady_clock::now();
        for (long r0 = 0; r0 < n_rows; r0 += batch) {
            const long m = std::min(batch, n_rows - r0);
            if (b9_sample_wd_mass(s.ctx, rows.data() + (size_t)r0 * B9_NPARAM, (int32_t)m, (int32_t)nodes, s.mcmc.seed, r0, out[0].data(),
                                  out[1].data(), out[2].data(), out[3].data(), out[4].data(), out[5].data(), out[6].data(), nullptr) != B9_OK) {
                for (FILE *p : f) std::fclose(p);
                throw std::runtime_error(b9_last_error(s.ctx));
            }
            for (int k = 0; k < 7; ++k)
                for (long r = 0; r < m; ++r) {
                    for (int c = 0; c < n_wd; ++c) std::fprintf(f[k], "%s%.6f", c ? " " : "", out[k][(size_t)r * n_wd + c]);
                    std::fprintf(f[k], "\n");
                }
        }
        for (FILE *p : f) std::fclose(p);
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::fprintf(stderr, "sampleWDMass: %ld chain rows x %d WD-stage stars (%ld mass nodes) in %.3f s (%.3e star draws/s) -> %s\n",
                     n_rows, n_wd, nodes, sec, (double)n_rows * n_wd / sec, names.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("sampleWDMass", e);
    }
}
