// scatterCluster -- adds photometric noise to a simCluster table and applies the survey's cuts ([RECALL] BASE-9
// scatterCluster): reads <outputFileBase>.sim.out, writes <outputFileBase>.sim.scatter in the .phot layout that
// singlePopMcmc / multiPopMcmc read (docs/FORMATS.md).  No model work, so no GPU: it never creates a context.
#include "b9sim.hpp"
#include "cli_common.hpp"

#include <cstdio>

int main(int argc, char **argv)
{
    try {
        b9h::Settings st;
        st.parse_args(argc, argv);
        const b9h::ScatterConfig cfg = b9h::scatter_config(st);
        const std::string base = st.str("general.files.outputFileBase", "base9");
        const b9h::SimTable t = b9h::read_sim_table(base + ".sim.out");
        const std::string path = base + ".sim.scatter";
        const long kept = b9h::scatter_cluster(cfg, t, path);
        std::fprintf(stderr, "scatterCluster: %ld of %zu systems kept -> %s\n", kept, t.size(), path.c_str());
        return 0;
    } catch (const std::exception &e) {
        return b9h::report_and_exit_code("scatterCluster", e);
    }
}
