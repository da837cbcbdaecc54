// b9sim.hpp -- the host-side draws of simCluster and scatterCluster ([RECALL] the upstream validation loop
// simCluster -> scatterCluster -> singlePopMcmc) and their settings.  docs/FORMATS.md states every
// draw; this file is their one definition (tests/test_sim_host.py restates them in numpy).
//
// Every number is counter-based Philox4x32-10 (as b9sampler / base_amd/mcmc.py): key = (seed lo, seed hi), counter =
// (i lo, i hi, purpose, j), so a system's values are a function of (seed, i, settings) alone.  Uniforms: u(a, b) =
// ((a >> 5) 2^26 + (b >> 6) + 0.5) / 2^53; normals: Box-Muller, z0 = sqrt(-2 log u(r0, r1)) cos(2 pi u(r2, r3)),
// z1 = ... sin(...).  No GPU work here: the magnitudes of the members come from b9_predict_mags.
#pragma once
#include "b9host.hpp"

#include <cstdint>
#include <string>
#include <vector>

namespace b9h {

enum SimPurpose { SIM_MASS = 0, SIM_BINARY = 1, SIM_DB = 2, SIM_POP = 3, SIM_FIELD = 4, SIM_NOISE = 5 };

// log-normal IMF in log10 m of the marginalised mode's mass prior (DESIGN.md "Math")
constexpr double kImfMu = -1.02, kImfSigma = 0.677;
constexpr int kMaxMassAttempts = 4096;
constexpr double kMinAcceptance = 1e-3;

struct SimConfig {                       // simCluster.*
    long n_stars = 100, n_field = 0;
    double percent_binary = 0.0, percent_db = 0.0;
    double min_mass = 0.1, max_mass = 8.0;          // max_mass default: general.white_dwarfs.M_wd_up
    double min_mass_ratio = 0.0, member_prior = 0.9;
    int n_pops = 1;
    uint64_t seed = 73;                  // general.seed
};
struct ScatterConfig {                   // scatterCluster.*
    double bright_limit = -100.0, faint_limit = 100.0, limit_s2n = 0.0;
    int relevant_filt = 0;
    double sigma_floor = 0.005, sigma_at_limit = 0.1;
    double member_prior = 0.9;           // simCluster.memberPrior: the CMprior column
    uint64_t seed = 74;                  // default general.seed + 1
};
// Resolve and validate (throws std::runtime_error naming the offending key)
SimConfig sim_config(const Settings &st);
ScatterConfig scatter_config(const Settings &st);

void philox4x32(const uint32_t ctr[4], uint32_t k0, uint32_t k1, uint32_t out[4]);
double u01(uint32_t hi, uint32_t lo);

// Systems i0 .. i0 + n - 1: primary mass (purpose 0), mass ratio (1), DB atmosphere (2), population (3).  tip[k]: the AGB-tip
// mass of population k's isochrone at the truth (q = 0 above it); lambda: fraction of population 0 (n_pops == 2).
void sim_draw_systems(const SimConfig &c, double lambda, const double tip[2], int64_t i0, int64_t n,
                      double *mass1, double *mass_ratio, int32_t *wd_type, int32_t *pop);
// Field-star magnitudes of systems i0 .. i0 + n - 1 (purpose 4): uniform in [lo[f], hi[f]] per filter; mags [n][nf]
void sim_field_mags(uint64_t seed, int64_t i0, int64_t n, int nf, const double *lo, const double *hi, double *mags);
// scatterCluster's noise of systems ids[0 .. n) (purpose 5): sigma[k][f] = sqrt(floor^2 + (at_limit 10^(0.2 (m - faint)))^2),
// obs = m + sigma z; mags / sigma / obs [n][nf]
void scatter_noise(const ScatterConfig &c, const int64_t *ids, int64_t n, int nf, const double *mags, double *sigma, double *obs);

// ---- .sim.out ([RECALL] name, [OWN] layout): "id <filters> mass1 massRatio stage wdType pop member" -------------------------
struct SimTable {
    std::vector<std::string> filters;
    std::vector<int64_t> id;
    std::vector<double> mags, mass1, mass_ratio;     // mags [n][nf]
    std::vector<int32_t> stage, wd_type, pop, member;
    size_t size() const { return id.size(); }
};
void write_sim_table(const std::string &path, const SimTable &t);
SimTable read_sim_table(const std::string &path);

// scatterCluster's whole transformation of a .sim.out (noise, then the cuts of docs/FORMATS.md) into .phot rows: returns the
// number of systems kept
long scatter_cluster(const ScatterConfig &c, const SimTable &in, const std::string &phot_path);

}  // namespace b9h
