// starInfluence -- which stars and which groups of stars drive the cluster parameters: stars are independent given the cluster
// parameters, so the posterior without star i is the saved chain reweighted by exp(-v_ri), v_ri the star's marginal
// log-likelihood under row r, and the posterior without a group of stars the chain reweighted by exp(-sum of their v_ri).
// Re-reads the cluster chain that singlePopMcmc / multiPopMcmc wrote to <outputFileBase>.res, as modelScore does, and feeds its
// main-run rows in batches to b9_star_influence: every star's v is formed exactly on the GPU -- no draws -- and reduced there to
// the leave-one-star-out moments of the quantities (per star) and to the groups' sums (per row).  A quantity is a cluster
// parameter (or logPost), passed as its z-score over the main-run rows: shifts are in units of the posterior sd.
// Writes
//   <outputFileBase>.starInfluence    one header line, then one line per star in .phot order:
//                                     id rows nInf ess paretoK {shift_<q> lin_<q> looSd_<q>}
//   <outputFileBase>.groupInfluence   (unless --noGroups) one line per group: group nStars rows nInf ess paretoK {shiftRaw_<q> shift_<q> looSd_<q>}
//   <outputFileBase>.influenceScale   "name mean sd", one line per quantity: what turns sd units back into dex or magnitudes
// Flags: [--nPops n] [--margIsoIncrem k] [--nMassRatios q] [--quantity NAME, repeatable] [--groupFile FILE | --noGroups]
// Settings: starInfluence.{margIsoIncrem, nMassRatios} (default: sampleMass's, 4 each), starInfluence.nPops,
// starInfluence.quantity (default: every cluster parameter that varies over the main-run rows), starInfluence.groupFile (lines
// "id name", at most 8 names; default: the groups ms and wd from the catalogue's stage), starInfluence.noGroups.
#include "cli_common.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        s.settings.parse_args(argc, argv, b9h::kStarInfluenceFlags);
        const b9h::ChainGrid g = b9h::chain_grid(s.settings, "starInfluence");
        const b9h::StarInfluenceConfig c = b9h::star_influence_config(s.settings);
        const b9h::SavedChain chain = b9h::open_saved_chain(s, g);
        const long n_rows = chain.n_rows;
        const b9h::InfluenceQuantities iq = b9h::influence_quantities(c, chain.rows.data(), chain.log_post.empty() ? nullptr : chain.log_post.data(), n_rows);
        const b9h::InfluenceGroups grp = b9h::influence_groups(c, s.phot.ids, s.phot.stage);

        const int n = s.phot.n_stars(), tail_len = b9h::model_score_tail_len(n_rows), Q = (int)iq.names.size(), G = (int)grp.names.size();
        std::vector<double> acc((size_t)n * B9_INF_N(Q), 0.0), tail((size_t)n * (size_t)tail_len, 0.0), group_lpd((size_t)n_rows * (size_t)G, 0.0);
        const double sec = b9h::for_row_batches(n_rows, [&](long r0, long m) {
            if (b9_star_influence(s.ctx, chain.row(r0), (int32_t)m, r0 ? B9_INF_CONTINUE : 0, Q, iq.q.data() + (size_t)r0 * Q, acc.data(), tail_len,
                                  tail_len > 0 ? tail.data() : nullptr, G, G ? grp.id.data() : nullptr, G ? group_lpd.data() + (size_t)r0 * G : nullptr) != B9_OK)
                throw std::runtime_error(b9_last_error(s.ctx));
        });
        const size_t n_col = (size_t)b9h::kInfluenceHead + 3 * (size_t)Q, g_col = (size_t)b9h::kGroupInfluenceHead + 3 * (size_t)Q;
        std::vector<double> table((size_t)n * n_col), gtable((size_t)G * g_col);
        b9h::influence_table(acc.data(), tail_len > 0 ? tail.data() : nullptr, tail_len, n, Q, table.data());
        const std::string out = s.output_base + ".starInfluence";
        b9h::write_star_influence(out, s.phot.ids, iq.names, table.data());
        b9h::write_influence_scale(s.output_base + ".influenceScale", iq.names, iq.mean.data(), iq.sd.data());
        if (G) {
            b9h::group_influence_table(group_lpd.data(), n_rows, G, iq.q.data(), Q, grp.id.data(), n, gtable.data());
            b9h::write_group_influence(s.output_base + ".groupInfluence", grp.names, iq.names, gtable.data());
        }
        // per quantity the five stars of largest |shift| among those whose weights are trustworthy (paretoK <= 0.7), then the groups
        for (int j = 0; j < Q; ++j) {
            std::vector<int> order;
            for (int i = 0; i < n; ++i)
                if (table[(size_t)i * n_col + 3] <= 0.7 && std::isfinite(table[(size_t)i * n_col + b9h::kInfluenceHead + 3 * (size_t)j])) order.push_back(i);
            auto mag = [&](int i) { return std::fabs(table[(size_t)i * n_col + b9h::kInfluenceHead + 3 * (size_t)j]); };
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return mag(a) > mag(b); });
            std::printf("%s (mean %.6g, sd %.6g): shift without the star, in sd\n", iq.names[(size_t)j].c_str(), iq.mean[(size_t)j], iq.sd[(size_t)j]);
            for (size_t k = 0; k < std::min<size_t>(5, order.size()); ++k) {
                const double *t = table.data() + (size_t)order[k] * n_col;
                std::printf("  %-16s shift %+.4f  lin %+.4f  ess %.1f  pareto k %.2f\n", s.phot.ids[(size_t)order[k]].c_str(), t[b9h::kInfluenceHead + 3 * j],
                            t[b9h::kInfluenceHead + 3 * j + 1], t[2], t[3]);
            }
            for (int k = 0; k < G; ++k) {
                const double *t = gtable.data() + (size_t)k * g_col;
                std::printf("  without group %-8s (%ld stars): shift %+.4f  (raw %+.4f)  ess %.1f  pareto k %.2f\n", grp.names[(size_t)k].c_str(), (long)t[0],
                            t[b9h::kGroupInfluenceHead + 3 * j + 1], t[b9h::kGroupInfluenceHead + 3 * j], t[3], t[4]);
            }
        }
        std::fprintf(stderr, "starInfluence: %ld chain rows x %d stars, %d quantities, %d groups (%d x %d mass / mass-ratio nodes per EEP interval, tail of %d) in %.3f s (%.3e star rows/s) -> %s\n",
                     n_rows, n, Q, G, g.K, g.Q, tail_len, sec, (double)n_rows * n / sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("starInfluence", e);
    }
}
