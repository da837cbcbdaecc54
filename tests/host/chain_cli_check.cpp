// chain_cli_check.cpp -- what the eight programs over a saved chain share below their mains (base_amd/host/b9chain.hpp), checked
// on the CPU by a stand-alone program: the loop over the chain's rows, the grid / population / node-count settings of every
// section, the programs' own flag tables, and the table writer with every format family.  Built with b9host.cpp and b9chain.cpp
// alone (nothing here needs a context), under AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_chain_cli_host.py.
// Exits non-zero at the first violated line.
#include "../../base_amd/host/b9host.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <sstream>
#include <stdexcept>
#include <utility>

namespace {

int g_checks = 0;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        ++g_checks;                                                                          \
        if (!(cond)) { std::fprintf(stderr, "chain_cli_check: line %d: %s\n", __LINE__, #cond); std::exit(1); } \
    } while (0)

// what f() throws ("" when it does not)
template <class F> std::string thrown(F f)
{
    try { f(); } catch (const std::exception &e) { return e.what(); }
    return "";
}

b9h::Settings with(std::initializer_list<std::pair<const char *, const char *>> kv)
{
    b9h::Settings st;
    for (auto &p : kv) st.set(p.first, p.second);
    return st;
}

b9h::Settings parsed(std::vector<const char *> args, const b9h::ProgramFlags &own = {})
{
    std::vector<char *> argv = {const_cast<char *>("prog")};
    for (const char *a : args) argv.push_back(const_cast<char *>(a));
    b9h::Settings st;
    st.parse_args((int)argv.size(), argv.data(), own);
    return st;
}

std::string slurp(const std::string &path)
{
    std::ifstream in(path, std::ios::binary);
    std::ostringstream s;
    s << in.rdbuf();
    return s.str();
}

void row_loop()
{
    for (long n_rows : {1l, 255l, 256l, 257l, 513l}) {
        std::vector<std::pair<long, long>> seen;
        const double sec = b9h::for_row_batches(n_rows, [&](long r0, long m) { seen.emplace_back(r0, m); });
        CHECK(sec >= 0.0 && std::isfinite(sec));
        CHECK((long)seen.size() == (n_rows + 255) / 256);
        long next = 0;
        for (size_t k = 0; k < seen.size(); ++k) {
            CHECK(seen[k].first == next);                    // in order, no gap, no overlap
            CHECK((seen[k].first == 0) == (k == 0));         // only the first batch starts the sums anew
            CHECK(seen[k].second >= 1 && seen[k].second <= 256);
            CHECK(seen[k].second == 256 || k + 1 == seen.size());
            next += seen[k].second;
        }
        CHECK(next == n_rows);
    }
    int calls = 0;
    b9h::for_row_batches(0, [&](long, long) { ++calls; });
    CHECK(calls == 0);
    std::vector<long> sizes;
    b9h::for_row_batches(7, [&](long, long m) { sizes.push_back(m); }, 3);
    CHECK((sizes == std::vector<long>{3, 3, 1}));
}

void grid_settings()
{
    for (const std::string sec : {"starSummary", "massFunction", "starIntervals", "photResiduals", "modelScore"}) {
        const std::string k = sec + ".margIsoIncrem", q = sec + ".nMassRatios", p = sec + ".nPops";
        b9h::ChainGrid g = b9h::chain_grid(b9h::Settings(), sec);
        CHECK(g.n_pops == 1 && g.K == 4 && g.Q == 4);
        g = b9h::chain_grid(with({{"sampleMass.margIsoIncrem", "6"}, {"sampleMass.nMassRatios", "5"}}), sec);        // sampleMass's beat 4
        CHECK(g.n_pops == 1 && g.K == 6 && g.Q == 5);
        g = b9h::chain_grid(with({{"sampleMass.margIsoIncrem", "6"}, {"sampleMass.nMassRatios", "5"}, {k.c_str(), "2"}, {p.c_str(), "2"}}), sec);
        CHECK(g.n_pops == 2 && g.K == 2 && g.Q == 5);                                                               // the own key beats sampleMass's
        g = b9h::chain_grid(with({{"sampleMass.nMassRatios", "5"}, {q.c_str(), "7"}}), sec);
        CHECK(g.K == 4 && g.Q == 7);
        for (const std::string other : {"starSummary", "massFunction", "starIntervals", "photResiduals", "modelScore", "wdSummary", "simCluster"})
            if (other != sec) {                                                                                     // no other section is read
                g = b9h::chain_grid(with({{(other + ".nPops").c_str(), "2"}, {(other + ".margIsoIncrem").c_str(), "9"}, {(other + ".nMassRatios").c_str(), "9"}}), sec);
                CHECK(g.n_pops == 1 && g.K == 4 && g.Q == 4);
            }
        for (const char *bad : {"0", "3", "-1"})
            CHECK(thrown([&] { b9h::chain_grid(with({{p.c_str(), bad}}), sec); }) == sec + ".nPops must be 1 or 2");
        const std::string positive = "margIsoIncrem and nMassRatios must be positive";
        CHECK(thrown([&] { b9h::chain_grid(with({{k.c_str(), "0"}}), sec); }) == positive);
        CHECK(thrown([&] { b9h::chain_grid(with({{q.c_str(), "-2"}}), sec); }) == positive);
        CHECK(thrown([&] { b9h::chain_grid(with({{"sampleMass.margIsoIncrem", "0"}}), sec); }) == positive);
        CHECK(b9h::chain_grid(with({{"sampleMass.margIsoIncrem", "0"}, {k.c_str(), "1"}}), sec).K == 1);
    }
    CHECK(b9h::chain_n_pops(b9h::Settings(), "wdSummary") == 1 && b9h::chain_n_pops(with({{"wdSummary.nPops", "2"}}), "wdSummary") == 2);
    CHECK(thrown([&] { b9h::chain_n_pops(with({{"wdSummary.nPops", "3"}}), "wdSummary"); }) == "wdSummary.nPops must be 1 or 2");
    // sampleMass: one population, its own two keys and nothing else
    b9h::ChainGrid g = b9h::sample_mass_grid(with({{"sampleMass.nPops", "2"}, {"starSummary.margIsoIncrem", "9"}}));
    CHECK(g.n_pops == 1 && g.K == 4 && g.Q == 4);
    g = b9h::sample_mass_grid(with({{"sampleMass.margIsoIncrem", "3"}, {"sampleMass.nMassRatios", "2"}}));
    CHECK(g.n_pops == 1 && g.K == 3 && g.Q == 2);
    CHECK(thrown([&] { b9h::sample_mass_grid(with({{"sampleMass.nMassRatios", "0"}})); }) == "margIsoIncrem and nMassRatios must be positive");
}

void mass_nodes()
{
    const std::string range = "nMassNodes must be a positive 32-bit number";
    for (const std::string sec : {"sampleWDMass", "wdSummary"}) {
        CHECK(b9h::wd_mass_nodes(b9h::Settings(), sec) == 512);
        CHECK(b9h::wd_mass_nodes(with({{"sampleWDMass.nMassNodes", "100"}}), sec) == 100);
        CHECK(b9h::wd_mass_nodes(with({{(sec + ".nMassNodes").c_str(), "2147483647"}}), sec) == 2147483647l);
        CHECK(b9h::wd_mass_nodes(with({{(sec + ".nMassNodes").c_str(), "1"}}), sec) == 1);
        for (const char *bad : {"0", "-5", "2147483648"})
            CHECK(thrown([&] { b9h::wd_mass_nodes(with({{(sec + ".nMassNodes").c_str(), bad}}), sec); }) == range);
    }
    CHECK(b9h::wd_mass_nodes(with({{"sampleWDMass.nMassNodes", "100"}, {"wdSummary.nMassNodes", "64"}}), "wdSummary") == 64);      // own, then sampleWDMass's, then 512
    CHECK(b9h::wd_mass_nodes(with({{"sampleWDMass.nMassNodes", "100"}, {"wdSummary.nMassNodes", "64"}}), "sampleWDMass") == 100);
    CHECK(thrown([&] { b9h::wd_mass_nodes(with({{"sampleWDMass.nMassNodes", "0"}}), "wdSummary"); }) == range);
    CHECK(b9h::wd_mass_nodes(parsed({"--nMassNodes", "300"}), "wdSummary") == 300);                                                // the flag is sampleWDMass's key
}

void program_flags()
{
    // a program's own spelling wins on its command line only, and sets what the long spelling sets
    b9h::Settings st = parsed({"--perStar", "--nPops", "2"}, b9h::kPhotResidFlags);
    CHECK(st.dump() == "photResiduals.nPops = 2\nphotResiduals.perStar = 1\n");
    CHECK(!st.has("massFunction.perStar") && !st.has("simCluster.nPops"));
    CHECK(st.dump() == parsed({"--photResidualsPerStar=1", "--photResidualsNPops=2"}).dump());
    CHECK(parsed({"--perStar", "--nPops", "2"}).dump() == "massFunction.perStar = 1\nsimCluster.nPops = 2\n");
    CHECK(parsed({"--perStar=0", "--nPops=2"}, b9h::kPhotResidFlags).dump() == "photResiduals.nPops = 2\nphotResiduals.perStar = 0\n");
    CHECK(parsed({"--perRow", "--nPops", "2"}, b9h::kModelScoreFlags).dump() == "modelScore.nPops = 2\nmodelScore.perRow = 1\n");
    CHECK(parsed({"--perStar"}, b9h::kModelScoreFlags).dump() == "massFunction.perStar = 1\n");           // not modelScore's: the shared table's
    CHECK(parsed({"--minMass", "0.5", "--maxMass=5"}, b9h::kMassFunctionFlags).dump() == "massFunction.maxMass = 5\nmassFunction.minMass = 0.5\n");
    CHECK(parsed({"--nPops", "2", "--quantity", "system"}, b9h::kMassFunctionFlags).dump() == "massFunction.quantity = system\nsimCluster.nPops = 2\n");
    CHECK(parsed({"--quantity", "system", "--nPops", "2"}, b9h::kStarIntervalsFlags).dump() == "starIntervals.nPops = 2\nstarIntervals.quantity = system\n");
    CHECK(parsed({"--minMass", "0.5"}, b9h::kStarIntervalsFlags).dump() == "simCluster.minMass = 0.5\n");
    // the long spellings stay flags of every program
    for (const b9h::ProgramFlags *own : {&b9h::kMassFunctionFlags, &b9h::kStarIntervalsFlags, &b9h::kPhotResidFlags, &b9h::kModelScoreFlags})
        CHECK(parsed({"--massFunctionMinMass", "1", "--massFunctionMaxMass", "2", "--starIntervalsQuantity", "system", "--starIntervalsNPops", "2",
                      "--photResidualsPerStar", "1", "--photResidualsNPops", "2", "--modelScorePerRow", "1", "--modelScoreNPops", "2"}, *own).dump() ==
              "massFunction.maxMass = 2\nmassFunction.minMass = 1\nmodelScore.nPops = 2\nmodelScore.perRow = 1\nphotResiduals.nPops = 2\n"
              "photResiduals.perStar = 1\nstarIntervals.nPops = 2\nstarIntervals.quantity = system\n");
    // messages
    CHECK(thrown([&] { parsed({"--perRow", "0"}, b9h::kModelScoreFlags); }) == "unexpected argument '0'");
    CHECK(thrown([&] { parsed({"--perStar", "0"}, b9h::kPhotResidFlags); }) == "unexpected argument '0'");
    CHECK(thrown([&] { parsed({"--perRow"}, b9h::kPhotResidFlags); }) == "flag --perRow needs a value");
    CHECK(thrown([&] { parsed({"--perRow=1"}, b9h::kPhotResidFlags); }) == "unknown flag --perRow");
    CHECK(thrown([&] { parsed({"--nPops"}, b9h::kModelScoreFlags); }) == "flag --modelScoreNPops needs a value");
    // what is the programs' own in the configs
    CHECK(b9h::phot_resid_config(parsed({"--perStar"}, b9h::kPhotResidFlags)).per_star && !b9h::phot_resid_config(parsed({"--perStar"})).per_star);
    const b9h::ModelScoreConfig ms = b9h::model_score_config(parsed({"--perRow", "--compareTo", "other/run"}, b9h::kModelScoreFlags));
    CHECK(ms.per_row && ms.compare_to == "other/run");
    const b9h::MassFunctionConfig mf = b9h::mass_function_config(parsed({"--minMass", "0.5", "--nBins", "3", "--linearBins"}, b9h::kMassFunctionFlags), 8.0);
    CHECK(mf.n_bins == 3 && mf.min_mass == 0.5 && mf.max_mass == 8.0 && mf.linear && !mf.per_star && mf.quantity == B9_HQ_PRIMARY);
    CHECK((mf.edges() == std::vector<double>{0.5, 3.0, 5.5, 8.0}));
    CHECK(thrown([&] { b9h::star_intervals_config(with({{"starIntervals.quantity", "total"}})); }) ==
          "starIntervals.quantity must be primary, secondary or system, not 'total'");
}

void table_writer(const std::string &dir)
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const std::string path = dir + "/table.txt";
    const std::vector<std::string> labels = {"s1", "a/b#c"};
    // every format family, a stride wider than the columns, a label column
    const std::vector<b9h::TableColumn> cols = {{"rows", "%.0f"}, {"n", "%ld"}, {"six", "%.6f"}, {"g", "%.17g"}};
    const double v[2][5] = {{400.0, 400.0, -0.0, 0.1 + 0.2, 99.0}, {1e15, 2147483648.0, 0.30000049, -inf, 99.0}};
    b9h::write_table(path, "id", &labels, cols, 2, &v[0][0], 5);
    CHECK(slurp(path) == "id rows n six g\ns1 400 400 -0.000000 0.30000000000000004\na/b#c 1000000000000000 2147483648 0.300000 -inf\n");
    // no label column: the header and every line start with their first column; no line at all
    const double w[3] = {nan, inf, -0.0};
    b9h::write_table(path, nullptr, nullptr, {{"a", "%.17g"}, {"b", "%.17g"}, {"c", "%.17g"}}, 1, w, 3);
    const std::string got = slurp(path);
    CHECK(got == "a b c\nnan inf -0\n" || got == "a b c\n-nan inf -0\n");
    b9h::write_table(path, "id", &labels, cols, 0, nullptr, 5);
    CHECK(slurp(path) == "id rows n six g\n");
    CHECK(thrown([&] { b9h::write_table(dir + "/no_such_directory/t", nullptr, nullptr, cols, 0, nullptr, 4); }) == "cannot write " + dir + "/no_such_directory/t");
    // the writers over it, and the reader that checks the same column names
    const double pw[2 * b9h::kPointwiseCols] = {400, 0, -3.25, 0.5, -3.75, -3.5, 0.125, -3.625, 0.375, 400, 2, -inf, 0.1 + 0.2, -inf, -inf, inf, -inf, inf};
    b9h::write_pointwise(path, labels, pw);
    CHECK(slurp(path) == "id rows nInf lppd pWaic elpdWaic elpdIs paretoK elpdLoo pLoo\ns1 400 0 -3.25 0.5 -3.75 -3.5 0.125 -3.625 0.375\n"
                         "a/b#c 400 2 -inf 0.30000000000000004 -inf -inf inf -inf inf\n");
    std::vector<std::string> ids;
    std::vector<double> tab;
    b9h::read_pointwise(path, ids, tab);
    CHECK(ids == labels && tab == std::vector<double>(pw, pw + 2 * b9h::kPointwiseCols));
    const double lpd[3] = {-1.5, -inf, 0.1 + 0.2};
    b9h::write_row_lpd(path, lpd, 3);
    CHECK(slurp(path) == "row lpd\n0 -1.5\n1 -inf\n2 0.30000000000000004\n");
    const double acc[2 * B9_MOM_N] = {400, 200, 300, 500, 100, 60, 50, 20, 0, 0, 0, 0, 0, 0, 0, 0};
    b9h::write_star_summary(path, labels, acc, 1);
    CHECK(slurp(path) == "id rows member mass massSd massRatio massRatioSd pBinary\ns1 400 0.500000 1.500000 0.500000 0.500000 0.223607 0.250000\n"
                         "a/b#c 0 0.000000 0.000000 0.000000 0.000000 0.000000 0.000000\n");
    b9h::write_star_summary(path, labels, acc, 2);
    CHECK(slurp(path) == "id rows member mass massSd massRatio massRatioSd pBinary pPop2\ns1 400 0.500000 1.500000 0.500000 0.500000 0.223607 0.250000 0.100000\n"
                         "a/b#c 0 0.000000 0.000000 0.000000 0.000000 0.000000 0.000000 0.000000\n");
    std::remove(path.c_str());
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: chain_cli_check <scratch directory>\n"); return 2; }
    try {
        row_loop();
        grid_settings();
        mass_nodes();
        program_flags();
        table_writer(argv[1]);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "chain_cli_check: unexpected exception: %s\n", e.what());
        return 1;
    }
    std::printf("chain_cli_check: ok (%d checks)\n", g_checks);
    return 0;
}
