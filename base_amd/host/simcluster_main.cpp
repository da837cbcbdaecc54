// simCluster -- simulates a cluster from a model directory ([RECALL] BASE-9 simCluster): the truth is the starting row
// (general.cluster.starting.*; with simCluster.nPops 2 also multiPopMcmc.{YA_start, YB_start, lambda_start}), the systems'
// masses, mass ratios, atmospheres and populations are drawn on the host (b9sim.hpp), their magnitudes come from
// b9_predict_mags on the GPU.  Writes <outputFileBase>.sim.out: the members, then the field stars (docs/FORMATS.md).
#include "b9sim.hpp"
#include "cli_common.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        s.settings.parse_args(argc, argv);
        const b9h::SimConfig cfg = b9h::sim_config(s.settings);       // (settings errors before anything touches a GPU)
        b9h::open_session(s, cfg.n_pops, false);
        auto check = [&](int rc) { if (rc != B9_OK) throw std::runtime_error(b9_last_error(s.ctx)); };
        const int nf = (int)s.pack.filters.size();
        int cap = 0;
        for (int n : s.pack.iso_n_eep) cap = std::max(cap, n);
        std::vector<double> mass(cap), mags((size_t)cap * nf);
        double tip[2] = {0.0, 0.0};
        for (int k = 0; k < cfg.n_pops; ++k) {
            int32_t first = 0, n = 0;
            check(b9_derive_isochrone(s.ctx, s.start.data(), k, cap, mass.data(), mags.data(), &first, &n, &tip[k]));
            if (n == 0) throw std::runtime_error("the cluster parameters lie outside the model grid");
        }
        if (cfg.n_pops == 1) tip[1] = tip[0];
        const int64_t n_all = cfg.n_stars + cfg.n_field;
        b9h::SimTable t;
        t.filters = s.pack.filters;
        t.id.resize(n_all); t.mags.resize((size_t)n_all * nf); t.mass1.resize(n_all); t.mass_ratio.resize(n_all);
        t.stage.resize(n_all); t.wd_type.resize(n_all); t.pop.resize(n_all); t.member.resize(n_all);
        b9h::sim_draw_systems(cfg, s.start[B9_P_LAMBDA], tip, 0, n_all, t.mass1.data(), t.mass_ratio.data(), t.wd_type.data(), t.pop.data());
        // every system through the forward model: the members' magnitudes, and every system's stage (a field star's
        // magnitudes are replaced below, its mass, mass ratio and stage are its own draws')
        check(b9_predict_mags(s.ctx, s.start.data(), n_all, t.mass1.data(), t.mass_ratio.data(), t.wd_type.data(), t.pop.data(),
                              t.mags.data(), t.stage.data()));
        for (int64_t i = 0; i < n_all; ++i) { t.id[i] = i; t.member[i] = i < cfg.n_stars ? 1 : 0; }
        if (cfg.n_field > 0) {
            // the members' noiseless-magnitude box (systems that give flux), +- 0.5
            std::vector<double> lo(nf, 1e300), hi(nf, -1e300);
            for (int64_t i = 0; i < cfg.n_stars; ++i)
                for (int f = 0; f < nf; ++f) {
                    const double m = t.mags[(size_t)i * nf + f];
                    if (m == B9_MAG_NOFLUX || !std::isfinite(m)) continue;
                    lo[f] = std::min(lo[f], m); hi[f] = std::max(hi[f], m);
                }
            for (int f = 0; f < nf; ++f) {
                if (!(hi[f] >= lo[f])) throw std::runtime_error("no member gives flux in filter " + t.filters[f] + ": no box for the field stars");
                lo[f] -= 0.5; hi[f] += 0.5;
            }
            b9h::sim_field_mags(cfg.seed, cfg.n_stars, cfg.n_field, nf, lo.data(), hi.data(), &t.mags[(size_t)cfg.n_stars * nf]);
        }
        const std::string path = s.output_base + ".sim.out";
        b9h::write_sim_table(path, t);
        std::fprintf(stderr, "simCluster: %ld members + %ld field stars (tip %.6f Msun) -> %s\n", cfg.n_stars, cfg.n_field, tip[0], path.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("simCluster", e);
    }
}
