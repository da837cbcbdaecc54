// cmdBand -- the model locus a saved chain implies in the colour-magnitude diagram, with its credible band: every EEP of the
// MS/RGB isochrone at the chosen mass ratios (0: single stars, 1: the equal-mass binary sequence), the WD cooling sequence, every
// population -- per point the ZAMS mass, every filter's apparent magnitude and the chosen colours.  Takes makeCMD's settings (no
// photometry), re-reads the cluster chain that singlePopMcmc wrote to <outputFileBase>.res and uses its main-run rows:
//   1. b9_cmd_band on the first row alone gives every line its pivot (that row's value; 0 where the line is absent there);
//   2. one call over all the rows gives the moments about the pivots, hence every line's first range;
//   3. passes of b9_cmd_band's bins on every line's OWN edges, narrowed around the line's quantile levels by the host
//      (b9h::refine_star_edges), until every level sits in a bracket that is final or --maxPasses is reached.
// Every pass is an exact reduction on the GPU: no draws.  Writes
//   <outputFileBase>.cmdBand   one header line, then one line per band line:
//                              line N mean sd min max {q<level> q<level>_lo q<level>_hi} passes flags
// Flags: [--ratios a,b,..] [--wdNodes n] [--wdTypes da|db|both] [--colours f1-f2,..] [--levels a,b,..] [--tol t] [--maxPasses n] [--nPops n]
// Settings: cmdBand.{ratios, wdNodes, wdTypes, colours, levels, tol, maxPasses, nPops} (default: 0,1; 256; da; none; 0.025, 0.16,
//           0.5, 0.84, 0.975; 1e-4 relative; 12 passes; 1).  The EEP window is the pack's whole range.
#include "cli_common.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <stdexcept>

int main(int argc, char **argv)
{
    try {
        b9h::Session s;
        s.settings.parse_args(argc, argv, b9h::kCmdBandFlags);
        const int n_pops = b9h::chain_n_pops(s.settings, "cmdBand");
        const b9h::CmdBandConfig c = b9h::cmd_band_config(s.settings);
        b9h::open_session(s, n_pops, false);
        const std::string res_path = s.output_base + ".res";
        const std::vector<double> rows = b9h::read_res_rows(res_path, s.start, 3);
        const long n_rows = (long)(rows.size() / B9_NPARAM);
        if (n_rows == 0) throw std::runtime_error(res_path + " holds no main-run (stage 3) rows");

        int eep_lo = 0, eep_hi = 0;              // the pack's whole EEP range [eep_lo, eep_hi)
        for (size_t i = 0; i < s.pack.iso_n_eep.size(); ++i) {
            if (s.pack.iso_n_eep[i] < 1) continue;
            const int a = s.pack.iso_first_eep[i], b = a + s.pack.iso_n_eep[i];
            if (eep_hi == eep_lo) { eep_lo = a; eep_hi = b; }
            eep_lo = std::min(eep_lo, a); eep_hi = std::max(eep_hi, b);
        }
        const std::vector<int32_t> colours = b9h::band_colour_ids(c, s.pack.filters);
        b9_band_spec spec{};
        spec.eep0 = eep_lo; spec.n_eep = c.ratios.empty() ? 0 : eep_hi - eep_lo;
        spec.n_ratio = (int32_t)c.ratios.size(); spec.ratio = c.ratios.data();
        spec.n_wd_nodes = (int32_t)c.wd_nodes; spec.wd_types = c.wd_types;
        spec.n_colour = (int32_t)(colours.size() / 2); spec.colour = colours.data();
        const std::vector<std::string> names = b9h::band_line_names(n_pops, spec.eep0, spec.n_eep, spec.n_ratio, c.wd_nodes, c.wd_types, s.pack.filters, colours);
        const long n_lines = (long)names.size();
        if (n_lines == 0) throw std::runtime_error("the spec has no lines: nothing to do");
        const auto check = [&](int rc) { if (rc != B9_OK) throw std::runtime_error(b9_last_error(s.ctx)); };

        const auto t0 = std::chrono::steady_clock::now();
        std::vector<double> pivot((size_t)n_lines), first((size_t)n_lines * B9_BAND_NMOM);
        check(b9_cmd_band(s.ctx, rows.data(), 1, &spec, 0, nullptr, first.data(), nullptr, 0, nullptr));
        for (long l = 0; l < n_lines; ++l) pivot[l] = first[(size_t)l * B9_BAND_NMOM + B9_BAND_N] > 0.0 ? first[(size_t)l * B9_BAND_NMOM + B9_BAND_MIN] : 0.0;
        int passes = 0;
        // (one call per pass: b9_cmd_band chunks the rows itself, and a continued call would carry every line's state both ways)
        if (n_rows > 2147483647l) throw std::runtime_error(res_path + " holds more rows than one call takes");
        const b9h::CmdBand r = b9h::cmd_band([&](double *mom) {
            check(b9_cmd_band(s.ctx, rows.data(), (int32_t)n_rows, &spec, 0, pivot.data(), mom, nullptr, 0, nullptr));
        }, [&](const double *edges, int n_bins, double *acc) {
            check(b9_cmd_band(s.ctx, rows.data(), (int32_t)n_rows, &spec, 0, nullptr, nullptr, edges, n_bins, acc));
            ++passes;
        }, n_lines, n_rows, c.levels, c.tol, c.max_passes);
        const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const int m = (int)c.levels.size();
        std::vector<double> table((size_t)n_lines * (5 + 3 * (size_t)m + 2));
        b9h::band_table(r.mom.data(), pivot.data(), n_lines, m, r.lines.value.data(), r.lines.lo.data(), r.lines.hi.data(), r.lines.passes.data(),
                        r.lines.flags.data(), table.data());
        const std::string out = s.output_base + ".cmdBand";
        b9h::write_cmd_band(out, names, c.levels, table.data());
        long open = 0;
        for (long l = 0; l < n_lines; ++l) open += (r.lines.flags[l] & b9h::kSivOpen) != 0;
        std::fprintf(stderr, "cmdBand: %ld chain rows x %ld lines (%d population(s), EEPs %d .. %d at %d ratio(s), %ld WD nodes) x %d levels in %d passes, %ld lines unfinished, %.3f s -> %s\n",
                     n_rows, n_lines, n_pops, eep_lo, eep_hi - 1, spec.n_ratio, c.wd_nodes, m, passes, open, sec, out.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("cmdBand", e);
    }
}
