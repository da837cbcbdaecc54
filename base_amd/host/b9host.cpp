// b9host.cpp -- see b9host.hpp.  File formats: docs/FORMATS.md.
#include "b9host.hpp"

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <sstream>
#include <stdexcept>

namespace b9h {

namespace {

std::string trim(const std::string &s)
{
    size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n");
    return a == std::string::npos ? "" : s.substr(a, b - a + 1);
}

std::string unquote(std::string v)
{
    v = trim(v);
    if (v.size() >= 2 && ((v.front() == '"' && v.back() == '"') || (v.front() == '\'' && v.back() == '\'')))
        v = v.substr(1, v.size() - 2);
    return v;
}

[[noreturn]] void fail(const std::string &msg) { throw std::runtime_error(msg); }

std::vector<std::string> split_ws(const std::string &line)
{
    std::vector<std::string> out;
    std::istringstream is(line);
    std::string t;
    while (is >> t) out.push_back(t);
    return out;
}

double to_double(const std::string &s, const std::string &what)
{
    std::string v = s;
    std::transform(v.begin(), v.end(), v.begin(), ::tolower);
    if (v == ".inf" || v == "inf" || v == "+inf") return INFINITY;
    if (v == "-.inf" || v == "-inf") return -INFINITY;
    char *end = nullptr;
    double d = std::strtod(s.c_str(), &end);
    if (end == s.c_str() || *end != '\0') fail("not a number (" + what + "): '" + s + "'");
    return d;
}

// value after "key=" inside a %s / %a / %c / %m / %g header line
double header_value(const std::string &line, const std::string &key)
{
    size_t p = line.find(key);
    if (p == std::string::npos) fail("header line lacks '" + key + "': " + line);
    p += key.size();
    while (p < line.size() && (line[p] == '=' || line[p] == ' ')) ++p;
    size_t e = p;
    while (e < line.size() && !isspace((unsigned char)line[e])) ++e;
    return to_double(line.substr(p, e - p), key);
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// Settings
// ---------------------------------------------------------------------------------------------
void Settings::load_yaml(const std::string &path)
{
    std::ifstream in(path);
    if (!in) fail("cannot open settings file " + path);
    std::vector<std::pair<int, std::string>> stack;      // (indent, key)
    std::string line;
    int lineno = 0;
    while (std::getline(in, line)) {
        ++lineno;
        size_t hash = std::string::npos;
        bool in_q = false;
        for (size_t i = 0; i < line.size(); ++i) {
            if (line[i] == '"' || line[i] == '\'') in_q = !in_q;
            if (line[i] == '#' && !in_q) { hash = i; break; }
        }
        if (hash != std::string::npos) line = line.substr(0, hash);
        if (trim(line).empty() || trim(line) == "---") continue;
        int indent = 0;
        while (indent < (int)line.size() && line[indent] == ' ') ++indent;
        size_t colon = line.find(':');
        if (colon == std::string::npos) fail(path + ":" + std::to_string(lineno) + ": expected 'key: value'");
        std::string key = trim(line.substr(0, colon)), value = unquote(line.substr(colon + 1));
        while (!stack.empty() && stack.back().first >= indent) stack.pop_back();
        if (value.empty()) { stack.emplace_back(indent, key); continue; }
        std::string full;
        for (auto &s : stack) full += s.second + ".";
        kv[full + key] = value;
    }
}

const std::map<std::string, std::string> &Settings::flag_map()
{
    static const std::map<std::string, std::string> m = {
        {"photFile", "general.files.photFile"}, {"outputFileBase", "general.files.outputFileBase"},
        {"modelDirectory", "general.files.modelDirectory"},
        {"msRgbModel", "general.main_sequence.msRgbModel"}, {"filterSet", "general.main_sequence.filterSet"},
        {"wdModel", "general.white_dwarfs.wdModel"}, {"ifmr", "general.white_dwarfs.ifmr"},
        {"M_wd_up", "general.white_dwarfs.M_wd_up"},
        {"priorFe_H", "general.cluster.priors.means.Fe_H"}, {"sigmaFe_H", "general.cluster.priors.sigmas.Fe_H"},
        {"priorDistMod", "general.cluster.priors.means.distMod"}, {"sigmaDistMod", "general.cluster.priors.sigmas.distMod"},
        {"priorAv", "general.cluster.priors.means.Av"}, {"sigmaAv", "general.cluster.priors.sigmas.Av"},
        {"priorY", "general.cluster.priors.means.Y"}, {"sigmaY", "general.cluster.priors.sigmas.Y"},
        {"priorCarbonicity", "general.cluster.priors.means.carbonicity"},
        {"sigmaCarbonicity", "general.cluster.priors.sigmas.carbonicity"},
        {"startingFe_H", "general.cluster.starting.Fe_H"}, {"startingDistMod", "general.cluster.starting.distMod"},
        {"startingAv", "general.cluster.starting.Av"}, {"startingY", "general.cluster.starting.Y"},
        {"startingCarbonicity", "general.cluster.starting.carbonicity"}, {"logAge", "general.cluster.starting.logAge"},
        {"startingYA", "multiPopMcmc.YA_start"}, {"startingYB", "multiPopMcmc.YB_start"},
        {"startingLambda", "multiPopMcmc.lambda_start"},
        {"minMag", "general.cluster.minMag"}, {"maxMag", "general.cluster.maxMag"}, {"index", "general.cluster.index"},
        {"burnIter", "singlePopMcmc.stage2IterMax"}, {"stage3Iter", "singlePopMcmc.stage3Iter"},
        {"runIter", "singlePopMcmc.runIter"}, {"thin", "singlePopMcmc.thin"},
        {"seed", "general.seed"}, {"verbose", "general.verbose"},
        {"walkers", "gpu.walkers"}, {"device", "gpu.device"}, {"block", "gpu.block"}, {"gpus", "gpu.gpus"},
        {"mode", "gpu.mode"}, {"marginalise", "gpu.marginalise"}, {"forceRanks", "gpu.forceRanks"}, {"tilesPerBlock", "gpu.tilesPerBlock"},
        {"resComment", "gpu.resComment"},
        {"margIsoIncrem", "sampleMass.margIsoIncrem"}, {"nMassRatios", "sampleMass.nMassRatios"},
        {"nMassNodes", "sampleWDMass.nMassNodes"},
        {"nBins", "massFunction.nBins"}, {"massFunctionMinMass", "massFunction.minMass"}, {"massFunctionMaxMass", "massFunction.maxMass"},
        {"linearBins", "massFunction.linearBins"}, {"quantity", "massFunction.quantity"}, {"perStar", "massFunction.perStar"},
        {"starIntervalsQuantity", "starIntervals.quantity"}, {"starIntervalsNPops", "starIntervals.nPops"}, {"levels", "starIntervals.levels"},
        {"tol", "starIntervals.tol"}, {"maxPasses", "starIntervals.maxPasses"},
        {"photResidualsPerStar", "photResiduals.perStar"}, {"photResidualsNPops", "photResiduals.nPops"},
        {"modelScorePerRow", "modelScore.perRow"}, {"modelScoreNPops", "modelScore.nPops"}, {"compareTo", "modelScore.compareTo"},
        {"nStars", "simCluster.nStars"}, {"percentBinary", "simCluster.percentBinary"}, {"percentDB", "simCluster.percentDB"},
        {"nFieldStars", "simCluster.nFieldStars"}, {"minMass", "simCluster.minMass"}, {"maxMass", "simCluster.maxMass"},
        {"minMassRatio", "simCluster.minMassRatio"}, {"memberPrior", "simCluster.memberPrior"}, {"nPops", "simCluster.nPops"},
        {"brightLimit", "scatterCluster.brightLimit"}, {"faintLimit", "scatterCluster.faintLimit"},
        {"relevantFilt", "scatterCluster.relevantFilt"}, {"limitS2N", "scatterCluster.limitS2N"},
        {"sigmaFloor", "scatterCluster.sigmaFloor"}, {"sigmaAtLimit", "scatterCluster.sigmaAtLimit"},
        {"scatterSeed", "scatterCluster.seed"},
    };
    return m;
}

void Settings::parse_args(int argc, char **argv)
{
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (a.rfind("--", 0) != 0) fail("unexpected argument '" + a + "'");
        a = a.substr(2);
        std::string value;
        size_t eq = a.find('=');
        if (eq != std::string::npos) { value = a.substr(eq + 1); a = a.substr(0, eq); }
        else if (a == "verbose" || a == "marginalise" || a == "forceRanks" || a == "resComment" || a == "linearBins" || a == "perStar") value = "1";
        else { if (i + 1 >= argc) fail("flag --" + a + " needs a value"); value = argv[++i]; }
        if (a == "config") { load_yaml(value); continue; }
        auto it = flag_map().find(a);
        if (it == flag_map().end()) fail("unknown flag --" + a);
        kv[it->second] = value;
    }
}

std::string Settings::str(const std::string &key, const std::string &def) const
{
    auto it = kv.find(key);
    return it == kv.end() ? def : it->second;
}
double Settings::num(const std::string &key, double def) const
{
    auto it = kv.find(key);
    return it == kv.end() ? def : to_double(it->second, key);
}
long Settings::integer(const std::string &key, long def) const { return (long)std::llround(num(key, (double)def)); }
std::string Settings::dump() const
{
    std::string s;
    for (auto &p : kv) s += p.first + " = " + p.second + "\n";
    return s;
}

// ---------------------------------------------------------------------------------------------
// Model packs
// ---------------------------------------------------------------------------------------------
b9_pack ModelPack::view() const
{
    b9_pack p{};
    p.n_filt = (int32_t)filters.size();
    p.n_feh = (int32_t)feh.size(); p.n_y = (int32_t)y.size(); p.n_age = (int32_t)log_age.size();
    p.feh = feh.data(); p.y = y.data(); p.log_age = log_age.data();
    p.iso_first_eep = iso_first_eep.data(); p.iso_n_eep = iso_n_eep.data(); p.iso_offset = iso_offset.data();
    p.n_points = (int64_t)mass.size();
    p.mass = mass.data(); p.mags = mags.data(); p.abs_coeff = abs_coeff.data();
    p.n_wc_carb = (int32_t)wc_carb.size(); p.n_wc_mass = (int32_t)wc_mass.size(); p.n_wc_points = (int64_t)wc_log_age.size();
    p.wc_carb = wc_carb.data(); p.wc_mass = wc_mass.data(); p.wc_log_age = wc_log_age.data();
    p.wc_n_age = wc_n_age.data(); p.wc_offset = wc_offset.data();
    p.wc_log_teff = wc_log_teff.data(); p.wc_log_radius = wc_log_radius.data();
    p.n_at_type = n_at_type; p.n_at_logg = (int32_t)at_logg.size(); p.n_at_teff = (int32_t)at_log_teff.size();
    p.at_logg = at_logg.data(); p.at_log_teff = at_log_teff.data(); p.at_mags = at_mags.data();
    p.ifmr_id = ifmr_id; p.m_wd_up = m_wd_up;
    return p;
}

namespace {

std::vector<int> select_columns(const std::vector<std::string> &have, const std::vector<std::string> &want,
                                const std::string &where)
{
    std::vector<int> cols;
    for (auto &f : want) {
        auto it = std::find(have.begin(), have.end(), f);
        if (it == have.end()) fail("filter '" + f + "' is not provided by " + where);
        cols.push_back((int)(it - have.begin()));
    }
    return cols;
}

struct RawIso { double feh, y, log_age; int first_eep; std::vector<double> mass, mags; };

void insert_axis(std::vector<double> &ax, double v)
{
    for (double a : ax) if (std::fabs(a - v) < 1e-9) return;
    ax.push_back(v);
}
int axis_index(const std::vector<double> &ax, double v)
{
    for (size_t i = 0; i < ax.size(); ++i) if (std::fabs(ax[i] - v) < 1e-9) return (int)i;
    return -1;
}

}  // namespace

std::vector<std::string> model_filters(const std::string &dir, const std::string &ms_model)
{
    std::ifstream in(dir + "/msrgb/" + ms_model + ".model");
    if (!in) fail("cannot open " + dir + "/msrgb/" + ms_model + ".model");
    std::string line;
    while (std::getline(in, line))
        if (line.rfind("%f", 0) == 0) { auto t = split_ws(line.substr(2)); return t; }
    fail("no %f line in " + ms_model + ".model");
}

ModelPack load_model_pack(const std::string &dir, const std::string &ms_model, const std::string &wd_model,
                          const std::vector<std::string> &filters)
{
    ModelPack pk;
    pk.filters = filters;
    const int nf = (int)filters.size();
    // ---- MS/RGB grid -------------------------------------------------------------------------
    {
        const std::string path = dir + "/msrgb/" + ms_model + ".model";
        std::ifstream in(path);
        if (!in) fail("cannot open " + path);
        std::vector<std::string> have;
        std::vector<int> cols;
        std::vector<RawIso> isos;
        double feh = NAN, y = NAN;
        std::string line;
        int lineno = 0;
        while (std::getline(in, line)) {
            ++lineno;
            if (line.empty() || line[0] == '#') continue;
            if (line[0] == '%') {
                if (line.size() < 2) continue;
                if (line[1] == 'f') { have = split_ws(line.substr(2)); cols = select_columns(have, filters, path); }
                else if (line[1] == 's') { feh = header_value(line, "[Fe/H]"); y = header_value(line, "Y"); }
                else if (line[1] == 'a') {
                    if (std::isnan(feh)) fail(path + ": %a before %s");
                    isos.push_back(RawIso{feh, y, header_value(line, "logAge"), -1, {}, {}});
                }
                continue;
            }
            if (isos.empty() || cols.empty()) fail(path + ":" + std::to_string(lineno) + ": data before %f/%s/%a");
            auto t = split_ws(line);
            if ((int)t.size() != (int)have.size() + 2) fail(path + ":" + std::to_string(lineno) + ": expected EEP, mass and one magnitude per filter");
            RawIso &iso = isos.back();
            int eep = (int)std::lround(to_double(t[0], "EEP"));
            if (iso.first_eep < 0) iso.first_eep = eep;
            else if (eep != iso.first_eep + (int)iso.mass.size()) fail(path + ":" + std::to_string(lineno) + ": EEPs must be consecutive");
            iso.mass.push_back(to_double(t[1], "mass"));
            for (int c : cols) iso.mags.push_back(to_double(t[2 + c], "magnitude"));
        }
        if (isos.empty()) fail(path + ": no isochrones");
        for (auto &i : isos) { insert_axis(pk.feh, i.feh); insert_axis(pk.y, i.y); insert_axis(pk.log_age, i.log_age); }
        std::sort(pk.feh.begin(), pk.feh.end()); std::sort(pk.y.begin(), pk.y.end()); std::sort(pk.log_age.begin(), pk.log_age.end());
        const size_t n_iso = pk.feh.size() * pk.y.size() * pk.log_age.size();
        if (n_iso != isos.size()) fail(path + ": the (FeH, Y, logAge) grid is not rectangular (" + std::to_string(isos.size()) + " isochrones for " + std::to_string(n_iso) + " grid nodes)");
        std::vector<const RawIso *> at(n_iso, nullptr);
        for (auto &i : isos) {
            size_t k = ((size_t)axis_index(pk.feh, i.feh) * pk.y.size() + axis_index(pk.y, i.y)) * pk.log_age.size() + axis_index(pk.log_age, i.log_age);
            if (at[k]) fail(path + ": duplicate isochrone");
            at[k] = &i;
        }
        pk.iso_first_eep.resize(n_iso); pk.iso_n_eep.resize(n_iso); pk.iso_offset.resize(n_iso);
        for (size_t k = 0; k < n_iso; ++k) {
            pk.iso_first_eep[k] = at[k]->first_eep; pk.iso_n_eep[k] = (int32_t)at[k]->mass.size(); pk.iso_offset[k] = (int64_t)pk.mass.size();
            pk.mass.insert(pk.mass.end(), at[k]->mass.begin(), at[k]->mass.end());
            pk.mags.insert(pk.mags.end(), at[k]->mags.begin(), at[k]->mags.end());
        }
    }
    // ---- absorption coefficients ---------------------------------------------------------------
    {
        std::map<std::string, double> coeff;
        std::ifstream in(dir + "/absorption.dat");
        std::string line;
        while (in && std::getline(in, line)) {
            if (line.empty() || line[0] == '#') continue;
            auto t = split_ws(line);
            if (t.size() >= 2) coeff[t[0]] = to_double(t[1], "absorption coefficient");
        }
        for (auto &f : filters) {
            if (!coeff.count(f)) fail("no absorption coefficient for filter '" + f + "' in " + dir + "/absorption.dat");
            pk.abs_coeff.push_back(coeff[f]);
        }
    }
    // ---- WD cooling ------------------------------------------------------------------------------
    if (!wd_model.empty()) {
        const std::string path = dir + "/wd/cooling_" + wd_model + ".dat";
        std::ifstream in(path);
        if (in) {
            struct Track { double carb, mass; std::vector<double> age, teff, rad; };
            std::vector<Track> tracks;
            double carb = 0.38;
            std::string line;
            while (std::getline(in, line)) {
                if (line.empty() || line[0] == '#') continue;
                if (line[0] == '%') {
                    if (line[1] == 'c') carb = header_value(line, "carbonicity");
                    else if (line[1] == 'm') tracks.push_back(Track{carb, header_value(line, "mass"), {}, {}, {}});
                    continue;
                }
                auto t = split_ws(line);
                if (t.size() != 3 || tracks.empty()) fail(path + ": expected 'logCoolAge logTeff logRadius' rows after %m");
                tracks.back().age.push_back(to_double(t[0], "age")); tracks.back().teff.push_back(to_double(t[1], "teff")); tracks.back().rad.push_back(to_double(t[2], "radius"));
            }
            if (tracks.empty()) fail(path + ": no cooling tracks");
            for (auto &t : tracks) { insert_axis(pk.wc_carb, t.carb); insert_axis(pk.wc_mass, t.mass); }
            std::sort(pk.wc_carb.begin(), pk.wc_carb.end()); std::sort(pk.wc_mass.begin(), pk.wc_mass.end());
            // every (carbonicity, mass) node needs exactly one track; each keeps ITS OWN age axis (tracks are ragged)
            const size_t nC = pk.wc_carb.size(), nM = pk.wc_mass.size();
            std::vector<const Track *> at(nC * nM, nullptr);
            for (auto &t : tracks) {
                const size_t k = (size_t)axis_index(pk.wc_carb, t.carb) * nM + axis_index(pk.wc_mass, t.mass);
                if (at[k]) fail(path + ": duplicate cooling track");
                if (t.age.size() < 2) fail(path + ": a cooling track needs at least two points");
                for (size_t i = 1; i < t.age.size(); ++i)
                    if (!(t.age[i] > t.age[i - 1])) fail(path + ": the cooling ages of a track must ascend");
                at[k] = &t;
            }
            for (size_t k = 0; k < at.size(); ++k) {
                if (!at[k]) fail(path + ": the (carbonicity, mass) grid of cooling tracks has holes");
                pk.wc_n_age.push_back((int32_t)at[k]->age.size());
                pk.wc_offset.push_back((int64_t)pk.wc_log_age.size());
                pk.wc_log_age.insert(pk.wc_log_age.end(), at[k]->age.begin(), at[k]->age.end());
                pk.wc_log_teff.insert(pk.wc_log_teff.end(), at[k]->teff.begin(), at[k]->teff.end());
                pk.wc_log_radius.insert(pk.wc_log_radius.end(), at[k]->rad.begin(), at[k]->rad.end());
            }
        }
        // ---- WD atmospheres ------------------------------------------------------------------------
        for (int type = 0; type < 2; ++type) {
            const std::string apath = dir + "/wd/atmos_" + (type ? "DB" : "DA") + ".dat";
            std::ifstream ia(apath);
            if (!ia) break;
            std::vector<std::string> have;
            std::vector<int> cols;
            std::vector<double> loggs, teff_axis, cur_teff;
            std::vector<std::vector<double>> blocks;       // per logg: rows of nf mags
            std::string line;
            while (std::getline(ia, line)) {
                if (line.empty() || line[0] == '#') continue;
                if (line[0] == '%') {
                    if (line[1] == 'f') { have = split_ws(line.substr(2)); cols = select_columns(have, filters, apath); }
                    else if (line[1] == 'g') {
                        if (!blocks.empty()) { if (teff_axis.empty()) teff_axis = cur_teff; else if (teff_axis != cur_teff) fail(apath + ": Teff axes differ between log g blocks"); }
                        loggs.push_back(header_value(line, "logg")); blocks.emplace_back(); cur_teff.clear();
                    }
                    continue;
                }
                auto t = split_ws(line);
                if (blocks.empty() || t.size() != have.size() + 1) fail(apath + ": expected 'logTeff mags...' rows after %g");
                cur_teff.push_back(to_double(t[0], "logTeff"));
                for (int c : cols) blocks.back().push_back(to_double(t[1 + c], "magnitude"));
            }
            if (teff_axis.empty()) teff_axis = cur_teff; else if (teff_axis != cur_teff) fail(apath + ": Teff axes differ between log g blocks");
            if (type == 0) { pk.at_logg = loggs; pk.at_log_teff = teff_axis; }
            else if (loggs != pk.at_logg || teff_axis != pk.at_log_teff) fail(apath + ": DA and DB tables must share their axes");
            for (auto &b : blocks) {
                if (b.size() != teff_axis.size() * (size_t)nf) fail(apath + ": ragged atmosphere block");
                pk.at_mags.insert(pk.at_mags.end(), b.begin(), b.end());
            }
            pk.n_at_type = type + 1;
        }
    }
    return pk;
}

// ---------------------------------------------------------------------------------------------
// Photometry
// ---------------------------------------------------------------------------------------------
b9_stars Photometry::view() const
{
    b9_stars s{};
    s.n_stars = n_stars(); s.n_filt = (int32_t)filters.size();
    s.obs = obs.data(); s.sigma = sigma.data(); s.mass1 = mass1.data(); s.mass_ratio = mass_ratio.data();
    s.clust_prior = clust_prior.data(); s.stage = stage.data(); s.wd_type = wd_type.data();
    s.filter_prior_min = filter_prior_min.data(); s.filter_prior_max = filter_prior_max.data();
    return s;
}

Photometry read_photometry(const std::string &path, double min_mag, double max_mag, int index)
{
    std::ifstream in(path);
    if (!in) fail("cannot open photometry file " + path);
    Photometry ph;
    std::string line;
    if (!std::getline(in, line)) fail(path + ": empty file");
    auto head = split_ws(line);
    if (head.empty() || head[0] != "id") fail(path + ": header must start with 'id'");
    size_t k = 1;
    while (k < head.size() && head[k].rfind("sig", 0) != 0) ph.filters.push_back(head[k++]);
    const size_t nf = ph.filters.size();
    if (nf == 0) fail(path + ": no filter columns");
    for (size_t f = 0; f < nf; ++f)
        if (k + f >= head.size() || head[k + f] != "sig" + ph.filters[f]) fail(path + ": expected column sig" + ph.filters[f]);
    k += nf;
    const char *rest[] = {"mass1", "massRatio", "stage", "CMprior", "useDBI"};
    for (int r = 0; r < 5; ++r)
        if (k + r >= head.size() || head[k + r] != rest[r]) fail(path + std::string(": expected column ") + rest[r]);
    const size_t ncol = 1 + 2 * nf + 5;
    if (index < 0 || index >= (int)nf) fail("magnitude-cut filter index out of range");
    int lineno = 1;
    while (std::getline(in, line)) {
        ++lineno;
        if (trim(line).empty() || line[0] == '#') continue;
        auto t = split_ws(line);
        if (t.size() < ncol) fail(path + ":" + std::to_string(lineno) + ": too few columns");
        std::vector<double> o(nf), s(nf);
        for (size_t f = 0; f < nf; ++f) { o[f] = to_double(t[1 + f], "magnitude"); s[f] = to_double(t[1 + nf + f], "sigma"); }
        int stage = (int)std::lround(to_double(t[1 + 2 * nf + 2], "stage"));
        // [RECALL] the magnitude window applies to MS/RGB stars in filter `index`; WDs are always kept
        if (stage != B9_STAGE_WD && (o[index] < min_mag || o[index] > max_mag)) continue;
        ph.ids.push_back(t[0]);
        ph.obs.insert(ph.obs.end(), o.begin(), o.end());
        ph.sigma.insert(ph.sigma.end(), s.begin(), s.end());
        ph.mass1.push_back(to_double(t[1 + 2 * nf], "mass1"));
        ph.mass_ratio.push_back(to_double(t[1 + 2 * nf + 1], "massRatio"));
        ph.stage.push_back(stage);
        ph.clust_prior.push_back(to_double(t[1 + 2 * nf + 3], "CMprior"));
        ph.use_dbi.push_back((int)std::lround(to_double(t[1 + 2 * nf + 4], "useDBI")));
        ph.wd_type.push_back(t.size() > ncol ? (int)std::lround(to_double(t[ncol], "wdType")) : 0);
    }
    if (ph.n_stars() == 0) fail(path + ": no stars inside the magnitude window");
    // field-star magnitude box = observed range per filter (over the stars in use) [RECALL filterPriorMin/Max]
    ph.filter_prior_min.assign(nf, 1e300); ph.filter_prior_max.assign(nf, -1e300);
    for (int i = 0; i < ph.n_stars(); ++i)
        for (size_t f = 0; f < nf; ++f) {
            if (ph.sigma[i * nf + f] <= 0) continue;
            ph.filter_prior_min[f] = std::min(ph.filter_prior_min[f], ph.obs[i * nf + f]);
            ph.filter_prior_max[f] = std::max(ph.filter_prior_max[f], ph.obs[i * nf + f]);
        }
    for (size_t f = 0; f < nf; ++f)
        if (!(ph.filter_prior_max[f] > ph.filter_prior_min[f])) { ph.filter_prior_min[f] = 0.0; ph.filter_prior_max[f] = 1.0; }
    return ph;
}

// ---------------------------------------------------------------------------------------------
// Results
// ---------------------------------------------------------------------------------------------
ResultWriter::ResultWriter(const std::string &path, const std::vector<std::string> &columns, const std::string &comment)
{
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) fail("cannot write " + path);
    if (!comment.empty()) std::fprintf(f, "# %s\n", comment.c_str());
    for (auto &c : columns) std::fprintf(f, "%12s ", c.c_str());
    std::fprintf(f, "%14s %5s\n", "logPost", "stage");
    fp = f;
}
ResultWriter::~ResultWriter() { if (fp) std::fclose((FILE *)fp); }
void ResultWriter::row(const std::vector<double> &values, double logpost, int stage)
{
    FILE *f = (FILE *)fp;
    for (double v : values) std::fprintf(f, "%12.6f ", v);
    std::fprintf(f, "%14.6f %5d\n", logpost, stage);
}

// ---------------------------------------------------------------------------------------------
// starSummary
// ---------------------------------------------------------------------------------------------
void star_table(const double *acc, long n_stars, double *table)
{
    for (long i = 0; i < n_stars; ++i) {
        const double *a = acc + (size_t)i * B9_MOM_N;
        double *t = table + (size_t)i * kStarTableCols;
        for (int c = 0; c < kStarTableCols; ++c) t[c] = 0.0;
        t[0] = a[B9_MOM_ROWS];
        if (a[B9_MOM_ROWS] > 0.0) t[1] = a[B9_MOM_MEMBER] / a[B9_MOM_ROWS];
        if (!(a[B9_MOM_MEMBER] > 0.0)) continue;             // no membership weight: every derived value is 0
        const double w = a[B9_MOM_MEMBER];
        t[2] = a[B9_MOM_M1] / w;
        t[3] = std::sqrt(std::max(0.0, a[B9_MOM_M1SQ] / w - t[2] * t[2]));
        t[4] = a[B9_MOM_Q] / w;
        t[5] = std::sqrt(std::max(0.0, a[B9_MOM_QSQ] / w - t[4] * t[4]));
        t[6] = a[B9_MOM_BINARY] / w;
        t[7] = a[B9_MOM_POP1] / w;
    }
}

void write_star_summary(const std::string &path, const std::vector<std::string> &ids, const double *acc, int n_pops)
{
    const long n = (long)ids.size();
    std::vector<double> table((size_t)n * kStarTableCols);
    star_table(acc, n, table.data());
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) fail("cannot write " + path);
    std::fprintf(f, "id rows member mass massSd massRatio massRatioSd pBinary%s\n", n_pops == 2 ? " pPop2" : "");
    for (long i = 0; i < n; ++i) {
        const double *t = table.data() + (size_t)i * kStarTableCols;
        std::fprintf(f, "%s %.0f %.6f %.6f %.6f %.6f %.6f %.6f", ids[i].c_str(), t[0], t[1], t[2], t[3], t[4], t[5], t[6]);
        if (n_pops == 2) std::fprintf(f, " %.6f", t[7]);
        std::fprintf(f, "\n");
    }
    if (std::fclose(f) != 0) fail("cannot write " + path);
}

// ---------------------------------------------------------------------------------------------
// wdSummary
// ---------------------------------------------------------------------------------------------
void wd_table(const double *acc, long n_wd, double *table)
{
    for (long i = 0; i < n_wd; ++i) {
        const double *a = acc + (size_t)i * B9_WDM_N;
        double *t = table + (size_t)i * kWdTableCols;
        for (int c = 0; c < kWdTableCols; ++c) t[c] = 0.0;
        t[0] = a[B9_WDM_ROWS];
        if (a[B9_WDM_ROWS] > 0.0) t[1] = a[B9_WDM_MEMBER] / a[B9_WDM_ROWS];
        if (!(a[B9_WDM_MEMBER] > 0.0)) continue;             // no membership weight: every further value is 0
        const double w = a[B9_WDM_MEMBER], wc = a[B9_WDM_COOLED];
        t[2] = wc / w;
        t[3] = a[B9_WDM_M1] / w;
        t[4] = std::sqrt(std::max(0.0, a[B9_WDM_M1SQ] / w - t[3] * t[3]));
        t[15] = a[B9_WDM_POP1] / w;
        if (!(wc > 0.0)) continue;                           // no cooled weight: the derived values' columns are 0
        for (int q = 0; q < 5; ++q) {
            const double mean = a[B9_WDM_WDMASS + 2 * q] / wc;
            t[5 + 2 * q] = mean;
            t[6 + 2 * q] = std::sqrt(std::max(0.0, a[B9_WDM_WDMASS_SQ + 2 * q] / wc - mean * mean));
        }
    }
}

void write_wd_summary(const std::string &path, const std::vector<std::string> &ids, const double *acc, int n_pops)
{
    const long n = (long)ids.size();
    std::vector<double> table((size_t)n * kWdTableCols);
    wd_table(acc, n, table.data());
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) fail("cannot write " + path);
    std::fprintf(f, "id rows member pCooled zamsMass zamsMassSd wdMass wdMassSd precLogAge precLogAgeSd logCoolAge logCoolAgeSd logTeff logTeffSd "
                    "logg loggSd%s\n", n_pops == 2 ? " pPop2" : "");
    for (long i = 0; i < n; ++i) {
        const double *t = table.data() + (size_t)i * kWdTableCols;
        std::fprintf(f, "%s %.0f", ids[i].c_str(), t[0]);
        for (int c = 1; c < (n_pops == 2 ? kWdTableCols : kWdTableCols - 1); ++c) std::fprintf(f, " %.6f", t[c]);
        std::fprintf(f, "\n");
    }
    if (std::fclose(f) != 0) fail("cannot write " + path);
}

// ---------------------------------------------------------------------------------------------
// massFunction
// ---------------------------------------------------------------------------------------------
namespace {
// numpy's default percentile of an ascending sample: linear interpolation between the order statistics around (n - 1) q
double percentile_sorted(const std::vector<double> &v, double q)
{
    const double pos = (double)(v.size() - 1) * q;
    const size_t lo = (size_t)std::floor(pos), hi = std::min(lo + 1, v.size() - 1);
    const double t = pos - (double)lo;
    return v[lo] + (v[hi] - v[lo]) * t;
}
}  // namespace

void mass_function_table(const double *row_hist, long n_rows, const double *edges, int n_bins, double *table)
{
    const size_t ncol = (size_t)n_bins + 1;
    std::vector<long> use;
    for (long r = 0; r < n_rows; ++r)
        if (row_hist[(size_t)r * ncol + n_bins] > 0.0) use.push_back(r);
    std::vector<double> v(use.size());
    for (int b = 0; b < n_bins; ++b) {
        double *t = table + (size_t)b * kMassFunctionCols;
        for (int c = 0; c < kMassFunctionCols; ++c) t[c] = 0.0;
        t[0] = edges[b]; t[1] = edges[b + 1];
        if (use.empty()) continue;
        double sum = 0.0;
        for (size_t k = 0; k < use.size(); ++k) { v[k] = row_hist[(size_t)use[k] * ncol + b]; sum += v[k]; }
        const double mean = sum / (double)use.size();
        double ss = 0.0;
        for (double x : v) ss += (x - mean) * (x - mean);
        std::sort(v.begin(), v.end());
        t[2] = mean;
        t[3] = std::sqrt(ss / (double)use.size());
        t[4] = percentile_sorted(v, 0.16); t[5] = percentile_sorted(v, 0.50); t[6] = percentile_sorted(v, 0.84);
        if (edges[b] > 0.0) t[7] = mean / std::log10(edges[b + 1] / edges[b]);
    }
}

void write_mass_function(const std::string &path, const double *table, int n_bins)
{
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) fail("cannot write " + path);
    std::fprintf(f, "lo hi mean sd p16 p50 p84 dNdlogM\n");
    for (int b = 0; b < n_bins; ++b) {
        const double *t = table + (size_t)b * kMassFunctionCols;
        std::fprintf(f, "%.6f %.6f %.6f %.6f %.6f %.6f %.6f %.6f\n", t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
    }
    if (std::fclose(f) != 0) fail("cannot write " + path);
}

void write_star_mass_hist(const std::string &path, const std::vector<std::string> &ids, const double *star_hist, int n_bins, long n_rows)
{
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) fail("cannot write " + path);
    std::fprintf(f, "id rows member");
    for (int b = 0; b < n_bins; ++b) std::fprintf(f, " bin%d", b);
    std::fprintf(f, "\n");
    const size_t ncol = (size_t)n_bins + 1;
    for (size_t i = 0; i < ids.size(); ++i) {
        const double *a = star_hist + i * ncol, tot = a[n_bins];
        std::fprintf(f, "%s %ld %.6f", ids[i].c_str(), n_rows, n_rows > 0 ? tot / (double)n_rows : 0.0);
        for (int b = 0; b < n_bins; ++b) std::fprintf(f, " %.6f", tot > 0.0 ? a[b] / tot : 0.0);
        std::fprintf(f, "\n");
    }
    if (std::fclose(f) != 0) fail("cannot write " + path);
}

std::vector<double> MassFunctionConfig::edges() const
{
    std::vector<double> e((size_t)n_bins + 1);
    for (int b = 0; b <= n_bins; ++b) {
        const double t = (double)b / (double)n_bins;
        e[b] = linear ? min_mass + (max_mass - min_mass) * t : min_mass * std::pow(max_mass / min_mass, t);
    }
    e[0] = min_mass; e[n_bins] = max_mass;
    for (int b = 0; b < n_bins; ++b)
        if (!(e[b + 1] > e[b])) fail("massFunction: the bins are too narrow to tell their edges apart");
    return e;
}

MassFunctionConfig mass_function_config(const Settings &st, double m_wd_up)
{
    MassFunctionConfig c;
    c.n_bins = (int)st.integer("massFunction.nBins", 24);
    c.min_mass = st.num("massFunction.minMass", 0.1);
    c.max_mass = st.num("massFunction.maxMass", m_wd_up);
    c.linear = st.integer("massFunction.linearBins", 0) != 0;
    c.per_star = st.integer("massFunction.perStar", 0) != 0;
    const std::string q = st.str("massFunction.quantity", "primary");
    if (q == "primary") c.quantity = B9_HQ_PRIMARY;
    else if (q == "secondary") c.quantity = B9_HQ_SECONDARY;
    else if (q == "system") c.quantity = B9_HQ_SYSTEM;
    else fail("massFunction.quantity must be primary, secondary or system, not '" + q + "'");
    c.K = (int)st.integer("massFunction.margIsoIncrem", st.integer("sampleMass.margIsoIncrem", 4));
    c.Q = (int)st.integer("massFunction.nMassRatios", st.integer("sampleMass.nMassRatios", 4));
    c.n_pops = (int)st.integer("massFunction.nPops", 1);
    if (c.n_bins < 1 || c.n_bins > B9_HIST_MAX_BINS) fail("massFunction.nBins must lie in 1 .. " + std::to_string(B9_HIST_MAX_BINS));
    if (!std::isfinite(c.min_mass) || !std::isfinite(c.max_mass) || !(c.max_mass > c.min_mass)) fail("massFunction: maxMass must exceed minMass");
    if (!c.linear && !(c.min_mass > 0.0)) fail("massFunction: log-spaced bins need minMass > 0 (or --linearBins)");
    if (c.K < 1 || c.Q < 1) fail("margIsoIncrem and nMassRatios must be positive");
    if (c.n_pops != 1 && c.n_pops != 2) fail("massFunction.nPops must be 1 or 2");
    return c;
}

std::vector<std::string> mass_function_args(int argc, char **argv)
{
    std::vector<std::string> out;
    for (int i = 0; i < argc; ++i) {
        std::string a = argv[i];
        for (const char *name : {"minMass", "maxMass"}) {
            const std::string flag = std::string("--") + name;
            if (a == flag || a.rfind(flag + "=", 0) == 0)
                a = std::string("--massFunction") + (char)std::toupper(name[0]) + (name + 1) + a.substr(flag.size());
        }
        out.push_back(a);
    }
    return out;
}

// ---------------------------------------------------------------------------------------------
// starIntervals
// ---------------------------------------------------------------------------------------------
namespace {
void check_levels(const double *levels, int m, int n_bins, const char *who)
{
    if (m < 1 || 3 * m > n_bins + 1) fail(std::string(who) + ": the levels need 3 edges each: at most (n_bins + 1) / 3 of them, at least one");
    for (int l = 0; l < m; ++l)
        if (!(levels[l] > 0.0 && levels[l] < 1.0) || (l > 0 && !(levels[l] > levels[l - 1])))
            fail(std::string(who) + ": the levels must lie strictly inside (0, 1) and ascend strictly");
}
}  // namespace

void refine_star_edges(const double *edges, const double *acc, long n_stars, int n_bins, const double *levels, int n_levels, double tol,
                       double *lo, double *hi, double *below, double *inside, double *value, int32_t *is_final, int32_t *flags, double *next_edges)
{
    const int B = n_bins, m = n_levels;
    if (B < 1) fail("refine_star_edges: n_bins must be positive");
    check_levels(levels, m, B, "refine_star_edges");
    if (!(tol >= 0.0)) fail("refine_star_edges: tol must not be negative");
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> cum((size_t)B + 2), pts, out;
    std::vector<int> col(m);
    for (long i = 0; i < n_stars; ++i) {
        const double *e = edges + (size_t)i * (B + 1), *a = acc + (size_t)i * (B + 3);
        double *ne = next_edges + (size_t)i * (B + 1);
        std::copy(e, e + B + 1, ne);                         // a finished star keeps its edges
        // the counted mass: below, the bins, at or above, summed in that order (the total column may hold more: B9_HQ_SECONDARY)
        double c = 0.0;
        for (int k = 0; k < B + 2; ++k) { c = c + a[k]; cum[k] = c; }
        const double C = cum[B + 1];
        flags[i] = 0;
        if (!(C > 0.0)) {
            flags[i] = kSivNoMass;
            for (int l = 0; l < m; ++l) {
                const size_t o = (size_t)i * m + l;
                lo[o] = hi[o] = value[o] = nan; below[o] = inside[o] = 0.0; is_final[o] = 1;
            }
            continue;
        }
        auto col_final = [&](int k) {
            if (k < 1 || k > B) return false;
            const double L = e[k - 1], H = e[k];
            return H - L <= tol * std::max(std::fabs(L), std::fabs(H)) || H == std::nextafter(L, inf);
        };
        bool open = false;
        for (int l = 0; l < m; ++l) {
            const size_t o = (size_t)i * m + l;
            const double target = levels[l] * C;
            // the column in which the cumulative sum first reaches the level -- within kSivSlack C, the rounding of the sums: a
            // level that falls exactly between two nodes (whole rows on either side: 17 of 34 at the median) is a tie that rounding
            // would decide one way in one pass and the other way in the next; with the slack every pass takes the lower node
            int k = 0;
            while (k < B + 1 && !(cum[k] >= target - kSivSlack * C)) ++k;
            col[l] = k;
            lo[o] = k == 0 ? -inf : e[k - 1];
            hi[o] = k == B + 1 ? inf : e[k];
            below[o] = k == 0 ? 0.0 : cum[k - 1];
            inside[o] = a[k];
            is_final[o] = col_final(k);
            open = open || !is_final[o];
            if (k == 0) value[o] = e[0];
            else if (k == B + 1) value[o] = e[B];
            else {
                const double t = a[k] > 0.0 ? std::min(1.0, std::max(0.0, (target - below[o]) / a[k])) : 0.0;
                value[o] = std::min(hi[o], std::max(lo[o], lo[o] + (hi[o] - lo[o]) * t));
            }
        }
        if (!open) continue;
        flags[i] = kSivOpen;
        // the next pass's edges: every distinct bracket keeps its two ends (an open one is widened to twice the range), the
        // unfinished ones share the remaining edges evenly as interior points
        const double range = e[B] - e[0];
        struct Iv { double L, H; bool todo; int extra; };
        std::vector<Iv> iv;
        for (int l = 0; l < m; ++l) {
            if (l > 0 && col[l] == col[l - 1]) continue;    // coinciding brackets share their sub-bins
            const int k = col[l];
            if (k == 0) iv.push_back({e[0] - 2.0 * range, e[0], true, 0});
            else if (k == B + 1) iv.push_back({e[B], e[B] + 2.0 * range, true, 0});
            else iv.push_back({e[k - 1], e[k], !col_final(k), 0});
        }
        int mandatory = 0, todo = 0;
        for (size_t j = 0; j < iv.size(); ++j) {
            mandatory += (j > 0 && iv[j].L == iv[j - 1].H) ? 1 : 2;
            todo += iv[j].todo;
        }
        int spare = B + 1 - mandatory;
        if (spare < todo) fail("refine_star_edges: too few bins for the levels");
        for (int j = 0, t = 0; j < (int)iv.size(); ++j)
            if (iv[j].todo) { iv[j].extra = spare / todo + (t < spare % todo); ++t; }
        out.clear();
        int left_over = 0;
        for (size_t j = 0; j < iv.size(); ++j) {
            if (out.empty() || out.back() != iv[j].L) out.push_back(iv[j].L);
            const int q = iv[j].extra;
            for (int s = 1; s <= q; ++s) {
                double x = iv[j].L + (iv[j].H - iv[j].L) * ((double)s / (double)(q + 1));
                if (!(x > out.back())) x = std::nextafter(out.back(), inf);
                if (!(x < iv[j].H)) { left_over += q - s + 1; break; }      // no double left inside the bracket
                out.push_back(x);
            }
            out.push_back(iv[j].H);
        }
        // (edges a bracket could not take go above the top one, a range apart: they cut nothing that matters)
        for (int s = 0; s < left_over; ++s) out.push_back(out.back() + std::max(range, std::fabs(out.back())));
        if ((int)out.size() != B + 1) fail("refine_star_edges: internal error: edge count");
        for (int b = 0; b <= B; ++b) {
            if (!std::isfinite(out[b]) || (b > 0 && !(out[b] > out[b - 1]))) fail("refine_star_edges: the next edges of star " + std::to_string(i) + " do not ascend");
            ne[b] = out[b];
        }
    }
}

StarIntervals star_intervals(const StarBinsFn &bins, long n_stars, long n_rows, int n_bins, double max_mass, const std::vector<double> &levels, double tol,
                             int max_passes)
{
    const int B = n_bins, m = (int)levels.size();
    check_levels(levels.data(), m, B, "star_intervals");
    if (max_passes < 1) fail("star_intervals: maxPasses must be positive");
    if (!(max_mass > 0.0) || !std::isfinite(max_mass)) fail("star_intervals: the largest mass must be positive");
    StarIntervals r;
    r.n_levels = m; r.n_stars = n_stars;
    const size_t nm = (size_t)n_stars * m;
    r.member.assign(n_stars, 0.0); r.value.assign(nm, 0.0); r.lo.assign(nm, 0.0); r.hi.assign(nm, 0.0);
    r.is_final.assign(nm, 0); r.passes.assign(n_stars, 0); r.flags.assign(n_stars, 0);
    std::vector<double> edges((size_t)n_stars * (B + 1)), next(edges.size()), acc((size_t)n_stars * (B + 3)), below(nm), inside(nm);
    for (long i = 0; i < n_stars; ++i)
        for (int b = 0; b <= B; ++b) edges[(size_t)i * (B + 1) + b] = (2.0 * max_mass) * ((double)b / (double)B);
    for (int pass = 1; pass <= max_passes; ++pass) {
        bins(edges.data(), B, acc.data());
        refine_star_edges(edges.data(), acc.data(), n_stars, B, levels.data(), m, tol, r.lo.data(), r.hi.data(), below.data(), inside.data(), r.value.data(),
                          r.is_final.data(), r.flags.data(), next.data());
        bool all = true;
        for (long i = 0; i < n_stars; ++i) {
            const bool done = !(r.flags[i] & kSivOpen);
            if (r.passes[i] == 0 && (done || pass == max_passes)) r.passes[i] = pass;
            all = all && done;
            r.member[i] = n_rows > 0 ? acc[(size_t)i * (B + 3) + B + 2] / (double)n_rows : 0.0;
        }
        if (all) break;
        edges.swap(next);
    }
    return r;
}

void star_intervals_table(const StarIntervals &r, double *table)
{
    const int m = r.n_levels;
    const size_t tcol = 3 * (size_t)m + 3;
    for (long i = 0; i < r.n_stars; ++i) {
        double *t = table + (size_t)i * tcol;
        t[0] = r.member[i];
        for (int l = 0; l < m; ++l) {
            const size_t o = (size_t)i * m + l;
            t[1 + 3 * l] = r.value[o]; t[2 + 3 * l] = r.lo[o]; t[3 + 3 * l] = r.hi[o];
        }
        t[tcol - 2] = (double)r.passes[i]; t[tcol - 1] = (double)r.flags[i];
    }
}

void write_star_intervals(const std::string &path, const std::vector<std::string> &ids, const std::vector<double> &levels, const double *table)
{
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) fail("cannot write " + path);
    std::fprintf(f, "id member");
    for (double a : levels) std::fprintf(f, " q%.12g q%.12g_lo q%.12g_hi", a, a, a);
    std::fprintf(f, " passes flags\n");
    const size_t tcol = 3 * levels.size() + 3;
    for (size_t i = 0; i < ids.size(); ++i) {
        const double *t = table + i * tcol;
        std::fprintf(f, "%s", ids[i].c_str());
        for (size_t c = 0; c + 2 < tcol; ++c) std::fprintf(f, " %.17g", t[c]);
        std::fprintf(f, " %.0f %.0f\n", t[tcol - 2], t[tcol - 1]);
    }
    if (std::fclose(f) != 0) fail("cannot write " + path);
}

StarIntervalsConfig star_intervals_config(const Settings &st)
{
    StarIntervalsConfig c;
    const std::string q = st.str("starIntervals.quantity", "primary");
    if (q == "primary") c.quantity = B9_HQ_PRIMARY;
    else if (q == "secondary") c.quantity = B9_HQ_SECONDARY;
    else if (q == "system") c.quantity = B9_HQ_SYSTEM;
    else fail("starIntervals.quantity must be primary, secondary or system, not '" + q + "'");
    std::string lv = st.str("starIntervals.levels", "0.025,0.16,0.5,0.84,0.975");
    for (char &ch : lv) if (ch == ',' || ch == '[' || ch == ']') ch = ' ';
    std::istringstream ls(lv);
    std::string tok;
    while (ls >> tok) {
        char *end = nullptr;
        const double v = std::strtod(tok.c_str(), &end);
        if (end == tok.c_str() || *end) fail("starIntervals.levels: '" + tok + "' is not a number");
        c.levels.push_back(v);
    }
    c.tol = st.num("starIntervals.tol", 1e-4);
    c.max_passes = (int)st.integer("starIntervals.maxPasses", 12);
    c.K = (int)st.integer("starIntervals.margIsoIncrem", st.integer("sampleMass.margIsoIncrem", 4));
    c.Q = (int)st.integer("starIntervals.nMassRatios", st.integer("sampleMass.nMassRatios", 4));
    c.n_pops = (int)st.integer("starIntervals.nPops", 1);
    check_levels(c.levels.data(), (int)c.levels.size(), B9_SBIN_MAX_BINS, "starIntervals.levels");
    if (!(c.tol >= 0.0)) fail("starIntervals.tol must not be negative");
    if (c.max_passes < 1) fail("starIntervals.maxPasses must be positive");
    if (c.K < 1 || c.Q < 1) fail("margIsoIncrem and nMassRatios must be positive");
    if (c.n_pops != 1 && c.n_pops != 2) fail("starIntervals.nPops must be 1 or 2");
    return c;
}

std::vector<std::string> star_intervals_args(int argc, char **argv)
{
    std::vector<std::string> out;
    for (int i = 0; i < argc; ++i) {
        std::string a = argv[i];
        for (const char *name : {"quantity", "nPops"}) {
            const std::string flag = std::string("--") + name;
            if (a == flag || a.rfind(flag + "=", 0) == 0)
                a = std::string("--starIntervals") + (char)std::toupper(name[0]) + (name + 1) + a.substr(flag.size());
        }
        out.push_back(a);
    }
    return out;
}

// ---------------------------------------------------------------------------------------------
// photResiduals
// ---------------------------------------------------------------------------------------------
void resid_table(const double *star_resid, const double *obs, const double *sigma, long n_stars, int nf, double *table)
{
    const size_t ncol = 2 + 2 * (size_t)nf, tcol = 2 + 4 * (size_t)nf;
    for (long i = 0; i < n_stars; ++i) {
        const double *a = star_resid + (size_t)i * ncol;
        double *t = table + (size_t)i * tcol;
        for (size_t c = 0; c < tcol; ++c) t[c] = 0.0;
        t[0] = a[0];
        if (a[0] > 0.0) t[1] = a[1] / a[0];
        if (!(a[1] > 0.0)) continue;                         // no membership weight: every derived value is 0
        for (int f = 0; f < nf; ++f) {
            const double sg = sigma[(size_t)i * nf + f], o = obs[(size_t)i * nf + f];
            const bool used = sg > 0.0;
            const double m1 = a[2 + 2 * f] / a[1], m2 = a[3 + 2 * f] / a[1];
            double *tf = t + 2 + 4 * (size_t)f;
            tf[0] = (used ? o : 0.0) + m1;
            tf[1] = std::sqrt(std::max(0.0, m2 - m1 * m1));
            if (used) { tf[2] = o - tf[0]; tf[3] = std::sqrt(m2) / sg; }
        }
    }
}

void filter_resid_table(const double *row_resid, long n_rows, int nf, double *table)
{
    const size_t ncol = 1 + 5 * (size_t)nf;
    std::vector<double> v;
    for (int f = 0; f < nf; ++f) {
        double *t = table + (size_t)f * kFilterResidCols;
        for (int c = 0; c < kFilterResidCols; ++c) t[c] = 0.0;
        std::vector<long> use;
        for (long r = 0; r < n_rows; ++r)
            if (row_resid[(size_t)r * ncol + 1 + 5 * f] > 0.0) use.push_back(r);
        t[0] = (double)use.size();
        if (use.empty()) continue;
        for (int q = 0; q < 3; ++q) {
            v.resize(use.size());
            double sum = 0.0;
            for (size_t k = 0; k < use.size(); ++k) {
                const double *x = row_resid + (size_t)use[k] * ncol + 1 + 5 * f;          // N, R, C, W, D
                v[k] = q == 0 ? x[1] / x[0] : q == 1 ? x[2] / x[0] : (x[3] > 0.0 ? x[4] / x[3] : 0.0);
                sum += v[k];
            }
            const double mean = sum / (double)use.size();
            double ss = 0.0;
            for (double x : v) ss += (x - mean) * (x - mean);
            std::sort(v.begin(), v.end());
            double *tq = t + 1 + 5 * q;
            tq[0] = mean;
            tq[1] = std::sqrt(ss / (double)use.size());
            tq[2] = percentile_sorted(v, 0.16); tq[3] = percentile_sorted(v, 0.50); tq[4] = percentile_sorted(v, 0.84);
        }
    }
}

void write_phot_resid(const std::string &path, const std::vector<std::string> &ids, const std::vector<std::string> &filters, const double *table)
{
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) fail("cannot write " + path);
    std::fprintf(f, "id rows member");
    for (const std::string &n : filters) std::fprintf(f, " %s_predMag %s_predSd %s_resid %s_rmsZ", n.c_str(), n.c_str(), n.c_str(), n.c_str());
    std::fprintf(f, "\n");
    const size_t tcol = 2 + 4 * filters.size();
    for (size_t i = 0; i < ids.size(); ++i) {
        std::fprintf(f, "%s", ids[i].c_str());
        for (size_t c = 0; c < tcol; ++c) std::fprintf(f, " %.17g", table[i * tcol + c]);
        std::fprintf(f, "\n");
    }
    if (std::fclose(f) != 0) fail("cannot write " + path);
}

void write_filter_resid(const std::string &path, const std::vector<std::string> &filters, const double *table)
{
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) fail("cannot write " + path);
    std::fprintf(f, "filter nRows");
    for (const char *q : {"meanZ", "chi2", "offset"})
        for (const char *s : {"mean", "sd", "p16", "p50", "p84"}) std::fprintf(f, " %s_%s", q, s);
    std::fprintf(f, "\n");
    for (size_t k = 0; k < filters.size(); ++k) {
        std::fprintf(f, "%s", filters[k].c_str());
        for (int c = 0; c < kFilterResidCols; ++c) std::fprintf(f, " %.17g", table[k * kFilterResidCols + c]);
        std::fprintf(f, "\n");
    }
    if (std::fclose(f) != 0) fail("cannot write " + path);
}

// ---------------------------------------------------------------------------------------------
// modelScore
// ---------------------------------------------------------------------------------------------
namespace {
const double kInf = std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();

// PSIS of one star: r[0 .. n_t) the finite tail values, descending (r[0] = RMAX); -> paretoK, elpdLoo (elpd_is where no fit is made)
void psis_star(const double *r, long n_t, double n_f, double rmax, double sneg, double elpd_is, double &pareto_k, double &elpd_loo)
{
    pareto_k = kNaN;
    elpd_loo = elpd_is;
    const long M = std::min({(long)std::floor(n_f / 5.0), (long)std::ceil(3.0 * std::sqrt(n_f)), n_t - 1});
    if (M < 5) return;
    const long N = M;
    std::vector<double> rho((size_t)M + 1), x((size_t)M);
    for (long j = 0; j <= M; ++j) rho[(size_t)j] = r[j] - r[0];
    const double ec = std::exp(rho[(size_t)M]);
    for (long j = 0; j < M; ++j) x[(size_t)(M - 1 - j)] = std::exp(rho[(size_t)j]) - ec;          // ascending: rho descends
    const double x_n = x[(size_t)N - 1], x_star = x[(size_t)std::floor((double)N / 4.0 + 0.5) - 1];
    if (x_n == 0.0 || !(x_star > 0.0)) return;
    // Zhang & Stephens' profile fit of the generalised Pareto distribution, with the weakly informative prior on k
    const long m = 30 + (long)std::floor(std::sqrt((double)N));
    std::vector<double> theta((size_t)m), ell((size_t)m);
    auto mean_log1p = [&](double th) { double sum = 0.0; for (long i = 0; i < N; ++i) sum += std::log1p(-th * x[(size_t)i]); return sum / (double)N; };
    for (long j = 1; j <= m; ++j) {
        const double th = 1.0 / x_n + (1.0 - std::sqrt((double)m / ((double)j - 0.5))) / (3.0 * x_star);
        const double k = mean_log1p(th);
        theta[(size_t)j - 1] = th;
        ell[(size_t)j - 1] = (double)N * (std::log(-th / k) - k - 1.0);
    }
    double theta_hat = 0.0;
    for (long j = 0; j < m; ++j) {
        double den = 0.0;
        for (long l = 0; l < m; ++l) den += std::exp(ell[(size_t)l] - ell[(size_t)j]);
        theta_hat += theta[(size_t)j] * (1.0 / den);
    }
    double k_hat = mean_log1p(theta_hat);
    const double sigma = -k_hat / theta_hat;
    k_hat = ((double)N * k_hat + 5.0) / ((double)N + 10.0);
    // the smoothed weights, paired by rank: the j-th smallest tail value takes the quantile at p_j = (j - 1/2) / M
    double num = n_f - (double)M, tail_raw = 0.0, tail_smooth = 0.0;
    for (long j = 1; j <= M; ++j) {
        const double p = ((double)j - 0.5) / (double)M, lp = std::log1p(-p);
        const double q = k_hat == 0.0 ? -sigma * lp : sigma * std::expm1(-k_hat * lp) / k_hat;
        const double w = std::min(1.0, ec + q), rh = rho[(size_t)(M - j)];
        num += std::exp(std::log(w) - rh);
        tail_smooth += w;
        tail_raw += std::exp(rh);
    }
    const double den = std::max(0.0, sneg - tail_raw) + tail_smooth;
    pareto_k = k_hat;
    elpd_loo = std::log(num) - std::log(den) - rmax;
}

// sum and sqrt(N var_ddof1) of v
void sum_se(const std::vector<double> &v, double &sum, double &se)
{
    sum = 0.0; se = 0.0;
    for (double x : v) sum += x;
    const size_t n = v.size();
    if (n < 2) return;
    const double mean = sum / (double)n;
    double ss = 0.0;
    for (double x : v) ss += (x - mean) * (x - mean);
    se = std::sqrt((double)n * (ss / (double)(n - 1)));
}
}  // namespace

void pointwise_table(const double *acc, const double *tail, int tail_len, long n_stars, double *table)
{
    for (long i = 0; i < n_stars; ++i) {
        const double *a = acc + (size_t)i * 8;
        double *t = table + (size_t)i * kPointwiseCols;
        for (int c = 0; c < kPointwiseCols; ++c) t[c] = 0.0;
        const double rows = a[0], n_inf = a[1], n_f = rows - n_inf;
        t[0] = rows; t[1] = n_inf;
        if (n_inf > 0.0) {                               // a row gives the star no likelihood at all: no finite score
            t[2] = n_f > 0.0 ? a[2] + std::log(a[3]) - std::log(rows) : -kInf;
            t[3] = n_f >= 2.0 ? a[7] / (n_f - 1.0) : 0.0;
            t[4] = t[5] = t[7] = -kInf; t[6] = kInf; t[8] = kInf;
            continue;
        }
        if (!(n_f > 0.0)) continue;
        const double lppd = a[2] + std::log(a[3]) - std::log(rows);
        const double p_waic = n_f >= 2.0 ? a[7] / (n_f - 1.0) : 0.0;
        const double elpd_is = std::log(n_f) - (a[4] + std::log(a[5]));
        long n_t = 0;
        const double *r = tail ? tail + (size_t)i * (size_t)tail_len : nullptr;
        while (r && n_t < tail_len && std::isfinite(r[n_t])) ++n_t;
        double k, loo;
        psis_star(r, n_t, n_f, a[4], a[5], elpd_is, k, loo);
        t[2] = lppd; t[3] = p_waic; t[4] = lppd - p_waic; t[5] = elpd_is; t[6] = k; t[7] = loo; t[8] = lppd - loo;
    }
}

void score_totals(const double *table, long n_stars, double *totals)
{
    std::vector<double> lppd, waic, loo;
    double p_waic = 0.0, p_loo = 0.0, n_infs = 0.0, n_high = 0.0, k_max = kNaN;
    for (long i = 0; i < n_stars; ++i) {
        const double *t = table + (size_t)i * kPointwiseCols;
        if (!(t[0] > 0.0)) continue;
        lppd.push_back(t[2]); waic.push_back(t[4]); loo.push_back(t[7]);
        p_waic += t[3]; p_loo += t[8];
        if (t[1] > 0.0) n_infs += 1.0;
        if (t[6] > 0.7) n_high += 1.0;
        if (std::isfinite(t[6]) && !(k_max >= t[6])) k_max = t[6];
    }
    totals[0] = (double)lppd.size();
    sum_se(lppd, totals[1], totals[2]);
    sum_se(waic, totals[3], totals[4]);
    sum_se(loo, totals[5], totals[6]);
    totals[7] = p_waic; totals[8] = p_loo; totals[9] = n_infs; totals[10] = n_high; totals[11] = k_max;
}

void score_compare(const double *table_a, const std::vector<std::string> &ids_a, const double *table_b, const std::vector<std::string> &ids_b,
                   double *out)
{
    if (ids_a.size() != ids_b.size()) fail("modelScore: the two catalogues differ in their number of stars");
    for (size_t i = 0; i < ids_a.size(); ++i)
        if (ids_a[i] != ids_b[i]) fail("modelScore: the two catalogues differ at star " + std::to_string(i) + " ('" + ids_a[i] + "' against '" + ids_b[i] + "')");
    std::vector<double> d_loo, d_waic;
    double dropped = 0.0;
    for (size_t i = 0; i < ids_a.size(); ++i) {
        const double *a = table_a + i * kPointwiseCols, *b = table_b + i * kPointwiseCols;
        if ((a[0] > 0.0) != (b[0] > 0.0)) dropped += 1.0;                  // scored by one fit only
        if (!(a[0] > 0.0) || !(b[0] > 0.0)) continue;
        d_loo.push_back(a[7] - b[7]);
        d_waic.push_back(a[4] - b[4]);
    }
    out[0] = (double)d_loo.size();
    sum_se(d_loo, out[1], out[2]);
    sum_se(d_waic, out[3], out[4]);
    out[5] = dropped;
}

static const char *const kPointwiseNames[kPointwiseCols] = {"rows", "nInf", "lppd", "pWaic", "elpdWaic", "elpdIs", "paretoK", "elpdLoo", "pLoo"};
static const char *const kScoreNames[kScoreTotals] = {"nStars", "lppd", "lppdSe", "elpdWaic", "elpdWaicSe", "elpdLoo", "elpdLooSe", "pWaic", "pLoo",
                                                      "nInfStars", "nHighK", "maxK"};
static const char *const kCompareNames[kScoreCompare] = {"nStars", "dElpdLoo", "dElpdLooSe", "dElpdWaic", "dElpdWaicSe", "nDropped"};

void write_pointwise(const std::string &path, const std::vector<std::string> &ids, const double *table)
{
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) fail("cannot write " + path);
    std::fprintf(f, "id");
    for (const char *n : kPointwiseNames) std::fprintf(f, " %s", n);
    std::fprintf(f, "\n");
    for (size_t i = 0; i < ids.size(); ++i) {
        std::fprintf(f, "%s", ids[i].c_str());
        for (int c = 0; c < kPointwiseCols; ++c) std::fprintf(f, " %.17g", table[i * kPointwiseCols + c]);
        std::fprintf(f, "\n");
    }
    if (std::fclose(f) != 0) fail("cannot write " + path);
}

static void write_named(const std::string &path, const char *const *names, int n, const double *v)
{
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) fail("cannot write " + path);
    for (int c = 0; c < n; ++c) std::fprintf(f, "%s%s", c ? " " : "", names[c]);
    std::fprintf(f, "\n");
    for (int c = 0; c < n; ++c) std::fprintf(f, "%s%.17g", c ? " " : "", v[c]);
    std::fprintf(f, "\n");
    if (std::fclose(f) != 0) fail("cannot write " + path);
}
void write_model_score(const std::string &path, const double *totals) { write_named(path, kScoreNames, kScoreTotals, totals); }
void write_model_compare(const std::string &path, const double *cmp) { write_named(path, kCompareNames, kScoreCompare, cmp); }

void write_row_lpd(const std::string &path, const double *row_lpd, long n_rows)
{
    FILE *f = std::fopen(path.c_str(), "w");
    if (!f) fail("cannot write " + path);
    std::fprintf(f, "row lpd\n");
    for (long r = 0; r < n_rows; ++r) std::fprintf(f, "%ld %.17g\n", r, row_lpd[r]);
    if (std::fclose(f) != 0) fail("cannot write " + path);
}

void read_pointwise(const std::string &path, std::vector<std::string> &ids, std::vector<double> &table)
{
    std::ifstream in(path);
    if (!in) fail("cannot read " + path);
    std::string line, word;
    if (!std::getline(in, line)) fail(path + ": empty file");
    {
        std::istringstream hs(line);
        hs >> word;
        if (word != "id") fail(path + ": not a .pointwise file (the header starts with '" + word + "')");
        for (const char *n : kPointwiseNames)
            if (!(hs >> word) || word != n) fail(path + ": column '" + std::string(n) + "' missing from the header");
    }
    ids.clear(); table.clear();
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        if (!(ls >> word)) continue;
        ids.push_back(word);
        for (int c = 0; c < kPointwiseCols; ++c) {
            if (!(ls >> word)) fail(path + ": short line for star '" + ids.back() + "'");
            table.push_back(std::strtod(word.c_str(), nullptr));         // (strtod reads inf / -inf / nan as printf wrote them)
        }
    }
}

const char *param_name(int idx)
{
    static const char *n[B9_NPARAM] = {"logAge", "Y", "FeH", "modulus", "absorption", "carbonicity",
                                       "IFMRconst", "IFMRlin", "IFMRquad", "YB", "lambda", "reserved"};
    return (idx >= 0 && idx < B9_NPARAM) ? n[idx] : "?";
}

}  // namespace b9h
