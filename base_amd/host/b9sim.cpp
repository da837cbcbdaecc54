// b9sim.cpp -- simCluster / scatterCluster host side: settings, the counter-based draws, the .sim.out table and the
// scatter step (b9sim.hpp; docs/FORMATS.md is the statement of every draw and cut).
#include "b9sim.hpp"

#include <cmath>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <stdexcept>

namespace b9h {

namespace {

[[noreturn]] void fail(const std::string &msg) { throw std::runtime_error(msg); }

std::vector<std::string> split_ws(const std::string &line)
{
    std::istringstream is(line);
    std::vector<std::string> t;
    std::string w;
    while (is >> w) t.push_back(w);
    return t;
}

double num_at(const std::string &s, const std::string &path, int lineno)
{
    char *end = nullptr;
    const double v = std::strtod(s.c_str(), &end);
    if (end == s.c_str() || *end) fail(path + ":" + std::to_string(lineno) + ": not a number: '" + s + "'");
    return v;
}

// standard normal CDF
double Phi(double x) { return 0.5 * std::erfc(-x * M_SQRT1_2); }

void philox_at(uint64_t seed, int64_t i, uint32_t purpose, uint32_t j, uint32_t r[4])
{
    const uint32_t c[4] = {(uint32_t)(uint64_t)i, (uint32_t)((uint64_t)i >> 32), purpose, j};
    philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32), r);
}

}  // namespace

// ---- settings ---------------------------------------------------------------------------------------------------------
SimConfig sim_config(const Settings &st)
{
    SimConfig c;
    c.n_stars = st.integer("simCluster.nStars", c.n_stars);
    c.n_field = st.integer("simCluster.nFieldStars", c.n_field);
    c.percent_binary = st.num("simCluster.percentBinary", c.percent_binary);
    c.percent_db = st.num("simCluster.percentDB", c.percent_db);
    c.min_mass = st.num("simCluster.minMass", c.min_mass);
    c.max_mass = st.num("simCluster.maxMass", st.num("general.white_dwarfs.M_wd_up", 8.0));
    c.min_mass_ratio = st.num("simCluster.minMassRatio", c.min_mass_ratio);
    c.member_prior = st.num("simCluster.memberPrior", c.member_prior);
    c.n_pops = (int)st.integer("simCluster.nPops", c.n_pops);
    c.seed = (uint64_t)st.integer("general.seed", 73);
    if (c.n_stars < 1) fail("simCluster.nStars must be at least 1");
    if (c.n_field < 0) fail("simCluster.nFieldStars must not be negative");
    if (!(c.percent_binary >= 0.0 && c.percent_binary <= 100.0)) fail("simCluster.percentBinary must lie in [0, 100]");
    if (!(c.percent_db >= 0.0 && c.percent_db <= 100.0)) fail("simCluster.percentDB must lie in [0, 100]");
    if (!(c.min_mass > 0.0)) fail("simCluster.minMass must be positive");
    if (!(c.min_mass < c.max_mass) || !std::isfinite(c.max_mass)) fail("simCluster.minMass must be smaller than simCluster.maxMass");
    if (!(c.min_mass_ratio >= 0.0 && c.min_mass_ratio < 1.0)) fail("simCluster.minMassRatio must lie in [0, 1)");
    if (!(c.member_prior >= 0.0 && c.member_prior <= 1.0)) fail("simCluster.memberPrior must lie in [0, 1]");
    if (c.n_pops != 1 && c.n_pops != 2) fail("simCluster.nPops must be 1 or 2");
    return c;
}

ScatterConfig scatter_config(const Settings &st)
{
    ScatterConfig c;
    c.bright_limit = st.num("scatterCluster.brightLimit", c.bright_limit);
    c.faint_limit = st.num("scatterCluster.faintLimit", c.faint_limit);
    c.relevant_filt = (int)st.integer("scatterCluster.relevantFilt", c.relevant_filt);
    c.limit_s2n = st.num("scatterCluster.limitS2N", c.limit_s2n);
    c.sigma_floor = st.num("scatterCluster.sigmaFloor", c.sigma_floor);
    c.sigma_at_limit = st.num("scatterCluster.sigmaAtLimit", c.sigma_at_limit);
    c.member_prior = st.num("simCluster.memberPrior", c.member_prior);
    c.seed = (uint64_t)st.integer("scatterCluster.seed", st.integer("general.seed", 73) + 1);
    if (!(c.bright_limit < c.faint_limit)) fail("scatterCluster.brightLimit must be smaller than scatterCluster.faintLimit");
    if (c.relevant_filt < 0) fail("scatterCluster.relevantFilt must not be negative");
    if (!(c.limit_s2n >= 0.0)) fail("scatterCluster.limitS2N must not be negative");
    if (!(c.sigma_floor >= 0.0 && c.sigma_at_limit >= 0.0) || !(c.sigma_floor > 0.0 || c.sigma_at_limit > 0.0))
        fail("scatterCluster.sigmaFloor and scatterCluster.sigmaAtLimit must not be negative, and not both zero");
    if (!(c.member_prior >= 0.0 && c.member_prior <= 1.0)) fail("simCluster.memberPrior must lie in [0, 1]");
    return c;
}

// ---- draws ------------------------------------------------------------------------------------------------------------
void philox4x32(const uint32_t ctr[4], uint32_t k0, uint32_t k1, uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)c0 * 0xD2511F53u, p1 = (uint64_t)c2 * 0xCD9E8D57u;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

double u01(uint32_t hi, uint32_t lo)
{
    const uint64_t x = (uint64_t)(hi >> 5) * (uint64_t)(1u << 26) + (uint64_t)(lo >> 6);
    const double u = ((double)x + 0.5) * (1.0 / 9007199254740992.0);
    return u < 1.0 ? u : 0x1.fffffffffffffp-1;      // (x = 2^53 - 1 rounds to 1: held below 1, as the device's u01)
}

void sim_draw_systems(const SimConfig &c, double lambda, const double tip[2], int64_t i0, int64_t n,
                      double *mass1, double *mass_ratio, int32_t *wd_type, int32_t *pop)
{
    const double zlow = (std::log10(c.min_mass) - kImfMu) / kImfSigma, zup = (std::log10(c.max_mass) - kImfMu) / kImfSigma;
    if (!(Phi(zup) - Phi(zlow) >= kMinAcceptance))
        fail("simCluster: the mass range [minMass, maxMass] holds less than 1e-3 of the IMF");
    uint32_t r[4];
    for (int64_t k = 0; k < n; ++k) {
        const int64_t i = i0 + k;
        double m1 = 0.0;
        int j = 0;
        for (; j < kMaxMassAttempts; ++j) {
            philox_at(c.seed, i, SIM_MASS, (uint32_t)j, r);
            const double z = std::sqrt(-2.0 * std::log(u01(r[0], r[1]))) * std::cos(2.0 * M_PI * u01(r[2], r[3]));
            if (z >= zlow && z <= zup) { m1 = std::pow(10.0, kImfMu + kImfSigma * z); break; }
        }
        if (j == kMaxMassAttempts) fail("simCluster: no primary mass accepted in 4096 attempts for system " + std::to_string(i));
        int p = 0;
        if (c.n_pops == 2) { philox_at(c.seed, i, SIM_POP, 0, r); p = u01(r[0], r[1]) >= lambda ? 1 : 0; }
        philox_at(c.seed, i, SIM_BINARY, 0, r);
        double q = u01(r[0], r[1]) < c.percent_binary / 100.0 ? c.min_mass_ratio + (1.0 - c.min_mass_ratio) * u01(r[2], r[3]) : 0.0;
        if (m1 > tip[p]) q = 0.0;                      // WD-stage stars are single in the marginalised model
        philox_at(c.seed, i, SIM_DB, 0, r);
        mass1[k] = m1; mass_ratio[k] = q;
        wd_type[k] = u01(r[0], r[1]) < c.percent_db / 100.0 ? 1 : 0;
        pop[k] = p;
    }
}

void sim_field_mags(uint64_t seed, int64_t i0, int64_t n, int nf, const double *lo, const double *hi, double *mags)
{
    uint32_t r[4];
    for (int64_t k = 0; k < n; ++k)
        for (int f2 = 0; 2 * f2 < nf; ++f2) {
            philox_at(seed, i0 + k, SIM_FIELD, (uint32_t)f2, r);
            for (int h = 0; h < 2 && 2 * f2 + h < nf; ++h) {
                const int f = 2 * f2 + h;
                mags[(size_t)k * nf + f] = lo[f] + (hi[f] - lo[f]) * u01(r[2 * h], r[2 * h + 1]);
            }
        }
}

void scatter_noise(const ScatterConfig &c, const int64_t *ids, int64_t n, int nf, const double *mags, double *sigma, double *obs)
{
    uint32_t r[4];
    for (int64_t k = 0; k < n; ++k)
        for (int f2 = 0; 2 * f2 < nf; ++f2) {
            philox_at(c.seed, ids[k], SIM_NOISE, (uint32_t)f2, r);
            const double rad = std::sqrt(-2.0 * std::log(u01(r[0], r[1]))), ang = 2.0 * M_PI * u01(r[2], r[3]);
            for (int h = 0; h < 2 && 2 * f2 + h < nf; ++h) {
                const size_t e = (size_t)k * nf + 2 * f2 + h;
                const double t = c.sigma_at_limit * std::pow(10.0, 0.2 * (mags[e] - c.faint_limit));
                sigma[e] = std::sqrt(c.sigma_floor * c.sigma_floor + t * t);
                obs[e] = mags[e] + sigma[e] * (h ? rad * std::sin(ang) : rad * std::cos(ang));
            }
        }
}

// ---- files ------------------------------------------------------------------------------------------------------------
void write_sim_table(const std::string &path, const SimTable &t)
{
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) fail("cannot write " + path);
    const size_t nf = t.filters.size();
    std::fprintf(f, "id");
    for (auto &fl : t.filters) std::fprintf(f, " %s", fl.c_str());
    std::fprintf(f, " mass1 massRatio stage wdType pop member\n");
    for (size_t i = 0; i < t.size(); ++i) {
        std::fprintf(f, "%lld", (long long)t.id[i]);
        for (size_t k = 0; k < nf; ++k) std::fprintf(f, " %.10f", t.mags[i * nf + k]);
        std::fprintf(f, " %.12f %.12f %d %d %d %d\n", t.mass1[i], t.mass_ratio[i], t.stage[i], t.wd_type[i], t.pop[i], t.member[i]);
    }
    if (std::fclose(f) != 0) fail("cannot write " + path);
}

SimTable read_sim_table(const std::string &path)
{
    std::ifstream in(path);
    if (!in) fail("cannot open " + path);
    SimTable t;
    std::string line;
    if (!std::getline(in, line)) fail(path + ": empty file");
    const auto head = split_ws(line);
    if (head.empty() || head[0] != "id") fail(path + ": header must start with 'id'");
    size_t k = 1;
    while (k < head.size() && head[k] != "mass1") t.filters.push_back(head[k++]);
    const char *rest[] = {"mass1", "massRatio", "stage", "wdType", "pop", "member"};
    for (int r = 0; r < 6; ++r)
        if (k + r >= head.size() || head[k + r] != rest[r]) fail(path + std::string(": expected column ") + rest[r]);
    const size_t nf = t.filters.size(), ncol = 1 + nf + 6;
    if (nf == 0) fail(path + ": no filter columns");
    int lineno = 1;
    while (std::getline(in, line)) {
        ++lineno;
        const auto v = split_ws(line);
        if (v.empty() || v[0][0] == '#') continue;
        if (v.size() != ncol) fail(path + ":" + std::to_string(lineno) + ": expected " + std::to_string(ncol) + " columns");
        t.id.push_back((int64_t)num_at(v[0], path, lineno));
        for (size_t f = 0; f < nf; ++f) t.mags.push_back(num_at(v[1 + f], path, lineno));
        t.mass1.push_back(num_at(v[1 + nf], path, lineno));
        t.mass_ratio.push_back(num_at(v[2 + nf], path, lineno));
        t.stage.push_back((int32_t)num_at(v[3 + nf], path, lineno));
        t.wd_type.push_back((int32_t)num_at(v[4 + nf], path, lineno));
        t.pop.push_back((int32_t)num_at(v[5 + nf], path, lineno));
        t.member.push_back((int32_t)num_at(v[6 + nf], path, lineno));
    }
    return t;
}

long scatter_cluster(const ScatterConfig &c, const SimTable &in, const std::string &phot_path)
{
    const int nf = (int)in.filters.size();
    if (c.relevant_filt >= nf) fail("scatterCluster.relevantFilt is past the last filter column");
    const int64_t n = (int64_t)in.size();
    std::vector<double> sigma((size_t)n * nf), obs((size_t)n * nf);
    scatter_noise(c, in.id.data(), n, nf, in.mags.data(), sigma.data(), obs.data());
    FILE *f = std::fopen(phot_path.c_str(), "w");
    if (!f) fail("cannot write " + phot_path);
    std::fprintf(f, "id");
    for (auto &fl : in.filters) std::fprintf(f, " %s", fl.c_str());
    for (auto &fl : in.filters) std::fprintf(f, " sig%s", fl.c_str());
    std::fprintf(f, " mass1 massRatio stage CMprior useDBI wdType\n");
    long kept = 0;
    for (int64_t i = 0; i < n; ++i) {
        const double *m = &in.mags[(size_t)i * nf];
        bool dark = false;
        for (int k = 0; k < nf; ++k) dark = dark || m[k] == B9_MAG_NOFLUX;
        if (dark || in.stage[i] == B9_STAGE_NSBH || in.stage[i] == B9_STAGE_DNE) continue;
        const double mr = m[c.relevant_filt], sr = sigma[(size_t)i * nf + c.relevant_filt];
        if (mr < c.bright_limit || mr > c.faint_limit) continue;
        if (1.0857 / sr < c.limit_s2n) continue;
        std::fprintf(f, "%lld", (long long)in.id[i]);
        for (int k = 0; k < nf; ++k) std::fprintf(f, " %.10f", obs[(size_t)i * nf + k]);
        for (int k = 0; k < nf; ++k) std::fprintf(f, " %.10f", sigma[(size_t)i * nf + k]);
        std::fprintf(f, " %.12f %.12f %d %.10g 1 %d\n", in.mass1[i], in.mass_ratio[i], in.stage[i], c.member_prior, in.wd_type[i]);
        ++kept;
    }
    if (std::fclose(f) != 0) fail("cannot write " + phot_path);
    return kept;
}

}  // namespace b9h
