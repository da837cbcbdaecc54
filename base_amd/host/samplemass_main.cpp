// sampleMass -- per-star mass posterior ([RECALL] BASE-9 sampleMass): re-reads the cluster chain that
// singlePopMcmc wrote to <outputFileBase>.res and, for every main-run row and every star, draws the
// primary mass and the mass ratio from the star's conditional posterior and reports the membership
// probability.  All of it is one call per batch of rows to b9_sample_mass (the marginalised-mode
// kernel in its sampling form).  Writes
//   <outputFileBase>.massSamples   one line per chain row:  mass ratio  mass ratio ...  (star order of the .phot)
//   <outputFileBase>.membership    one line per chain row:  membership probability of every star
// Settings: sampleMass.margIsoIncrem (--margIsoIncrem, default 4 sub-steps per EEP interval),
//           sampleMass.nMassRatios (--nMassRatios, default 4), general.seed.
#include "cli_common.hpp"

#include <algorithm>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        s.settings.parse_args(argc, argv);
        const b9h::ChainGrid g = b9h::sample_mass_grid(s.settings);
        const b9h::SavedChain chain = b9h::open_saved_chain(s, g);
        const long n_rows = chain.n_rows;

        const int n = s.phot.n_stars();
        const std::string mp = s.output_base + ".massSamples", bp = s.output_base + ".membership";
        FILE *fm = std::fopen(mp.c_str(), "w"), *fb = std::fopen(bp.c_str(), "w");
        if (!fm || !fb) throw std::runtime_error("cannot write " + mp + " / " + bp);
        for (int i = 0; i < n; ++i) std::fprintf(fm, "%s%s_mass %s_massRatio", i ? " " : "", s.phot.ids[i].c_str(), s.phot.ids[i].c_str());
        std::fprintf(fm, "\n");
        for (int i = 0; i < n; ++i) std::fprintf(fb, "%s%s", i ? " " : "", s.phot.ids[i].c_str());
        std::fprintf(fb, "\n");
        const size_t cap = (size_t)b9h::kChainBatch * n;
        std::vector<double> mass(cap), ratio(cap), member(cap);
        const double sec = b9h::for_row_batches(n_rows, [&](long r0, long m) {
            if (b9_sample_mass(s.ctx, chain.row(r0), (int32_t)m, s.mcmc.seed, r0, mass.data(), ratio.data(),
                               member.data(), nullptr) != B9_OK)
                throw std::runtime_error(b9_last_error(s.ctx));
            for (long r = 0; r < m; ++r) {
                for (int i = 0; i < n; ++i)
                    std::fprintf(fm, "%s%.6f %.4f", i ? " " : "", mass[(size_t)r * n + i], ratio[(size_t)r * n + i]);
                std::fprintf(fm, "\n");
                for (int i = 0; i < n; ++i) std::fprintf(fb, "%s%.6f", i ? " " : "", member[(size_t)r * n + i]);
                std::fprintf(fb, "\n");
            }
        });
        std::fclose(fm); std::fclose(fb);
        std::fprintf(stderr, "sampleMass: %ld chain rows x %d stars (%d x %d mass / mass-ratio nodes per EEP interval) in %.3f s (%.3e star draws/s) -> %s, %s\n",
                     n_rows, n, g.K, g.Q, sec, (double)n_rows * n / sec, mp.c_str(), bp.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("sampleMass", e);
    }
}
