// modelScore -- which of two fits predicts the data better: the pointwise predictive density of every star over the saved
// chain, reduced to WAIC and to leave-one-star-out cross-validation by Pareto-smoothed importance sampling (PSIS-LOO), and the
// paired difference of two fits with its standard error.  Re-reads the cluster chain that singlePopMcmc / multiPopMcmc wrote
// to <outputFileBase>.res, as photResiduals does, and feeds its main-run rows in batches to b9_pointwise: every star's
// marginal log-likelihood over the marginalisation grid is formed exactly on the GPU -- no draws -- and reduced there over the
// rows (per star) and over the stars (per row).
// Writes
//   <outputFileBase>.pointwise     one header line, then one line per star in .phot order:
//                                  id rows nInf lppd pWaic elpdWaic elpdIs paretoK elpdLoo pLoo
//   <outputFileBase>.modelScore    the totals: one header line, one line of values
//   <outputFileBase>.rowLpd        (--perRow) "row lpd", one line per chain row: the row's summed log predictive density
// modelScore --compareTo <otherBase> needs no GPU: it reads <outputFileBase>.pointwise and <otherBase>.pointwise, prints
// delta elpd +- se for LOO and WAIC (this base minus the other) and writes <outputFileBase>.modelCompare.
// Flags: [--nPops n] [--margIsoIncrem k] [--nMassRatios q] [--perRow] [--compareTo otherBase]
// Settings: modelScore.{margIsoIncrem, nMassRatios} (default: sampleMass's, 4 each), modelScore.nPops, modelScore.perRow.
#include "cli_common.hpp"

#include <algorithm>
#include <cstdio>
#include <stdexcept>

static int compare(const std::string &base, const std::string &other)
{
    std::vector<std::string> ids_a, ids_b;
    std::vector<double> tab_a, tab_b;
    b9h::read_pointwise(base + ".pointwise", ids_a, tab_a);
    b9h::read_pointwise(other + ".pointwise", ids_b, tab_b);
    double cmp[b9h::kScoreCompare];
    b9h::score_compare(tab_a.data(), ids_a, tab_b.data(), ids_b, cmp);
    const std::string out = base + ".modelCompare";
    b9h::write_model_compare(out, cmp);
    std::printf("%s - %s over %ld stars\n  delta elpd (PSIS-LOO) = %.6f +- %.6f\n  delta elpd (WAIC)     = %.6f +- %.6f\n", base.c_str(), other.c_str(),
                (long)cmp[0], cmp[1], cmp[2], cmp[3], cmp[4]);
    if (cmp[5] > 0.0) std::printf("  %ld star(s) scored by one of the two fits only: left out\n", (long)cmp[5]);
    std::fprintf(stderr, "modelScore: -> %s\n", out.c_str());
    return 0;
}

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        s.settings.parse_args(argc, argv, b9h::kModelScoreFlags);
        const b9h::ChainGrid g = b9h::chain_grid(s.settings, "modelScore");
        const b9h::ModelScoreConfig c = b9h::model_score_config(s.settings);
        if (!c.compare_to.empty()) return compare(s.settings.str("general.files.outputFileBase", "base9"), c.compare_to);     // (no GPU context yet)
        const b9h::SavedChain chain = b9h::open_saved_chain(s, g);
        const long n_rows = chain.n_rows;

        const int n = s.phot.n_stars(), tail_len = b9h::model_score_tail_len(n_rows);
        std::vector<double> acc((size_t)n * B9_PW_N, 0.0), tail((size_t)n * (size_t)tail_len, 0.0), row_lpd(c.per_row ? (size_t)n_rows : 0, 0.0);
        const double sec = b9h::for_row_batches(n_rows, [&](long r0, long m) {
            if (b9_pointwise(s.ctx, chain.row(r0), (int32_t)m, r0 ? B9_PW_CONTINUE : 0, tail_len, acc.data(),
                             tail_len > 0 ? tail.data() : nullptr, c.per_row ? row_lpd.data() + r0 : nullptr) != B9_OK)
                throw std::runtime_error(b9_last_error(s.ctx));
        });
        std::vector<double> table((size_t)n * b9h::kPointwiseCols);
        b9h::pointwise_table(acc.data(), tail_len > 0 ? tail.data() : nullptr, tail_len, n, table.data());
        double totals[b9h::kScoreTotals];
        b9h::score_totals(table.data(), n, totals);
        b9h::write_pointwise(s.output_base + ".pointwise", s.phot.ids, table.data());
        const std::string out = s.output_base + ".modelScore";
        b9h::write_model_score(out, totals);
        if (c.per_row) b9h::write_row_lpd(s.output_base + ".rowLpd", row_lpd.data(), n_rows);
        std::printf("elpd (PSIS-LOO) = %.6f +- %.6f   p_loo = %.3f   stars with pareto k > 0.7: %ld\nelpd (WAIC)     = %.6f +- %.6f   p_waic = %.3f\n",
                    totals[5], totals[6], totals[8], (long)totals[10], totals[3], totals[4], totals[7]);
        std::fprintf(stderr, "modelScore: %ld chain rows x %d stars (%d x %d mass / mass-ratio nodes per EEP interval, tail of %d) in %.3f s (%.3e star rows/s) -> %s\n",
                     n_rows, n, g.K, g.Q, tail_len, sec, (double)n_rows * n / sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("modelScore", e);
    }
}
