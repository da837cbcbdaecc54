// cli_common.hpp -- what the command-line programs share where a GPU context is involved: settings -> context, the sampling run
// (walker-parallel over the GPUs of one node when launched with --gpus N), and what every program over a saved chain does before
// its own work.  (Their settings, tables and files need no context: b9chain.hpp.)
#pragma once
#include "b9host.hpp"
#include "b9sampler.hpp"

namespace b9h {

struct McmcConfig {
    std::vector<int32_t> free_idx;        // sampled parameters (B9_P_*)
    std::vector<double> step;             // initial step size per sampled parameter
    int n_walkers = 1;                    // all ranks together
    long burn_iter = 2000, run_iter = 10000, thin = 1, block = 50;
    uint64_t seed = 73;
    bool verbose = false;
};

struct McmcResult {
    long accepted = 0, steps = 0;         // accepted: this rank's walkers
    double seconds = 0.0, star_evals_per_s = 0.0;   // whole job (all ranks), max-over-ranks time
};

struct Session {
    Settings settings;
    ModelPack pack;
    Photometry phot;
    b9_ctx *ctx = nullptr;
    std::vector<double> start;        // B9_NPARAM starting row
    b9_priors priors{};
    b9_options options{B9_MODE_GIVEN_MASS, 1, 8, 8};
    McmcConfig mcmc;
    std::string output_base;
    int rank = 0, world = 1, local_rank = 0;      // this process within a --gpus N launch
    ~Session() { if (ctx) b9_ctx_destroy(ctx); }
};

// From s.settings (the caller has parsed its flags / YAML into them): loads the photometry (unless `need_phot` is false) and
// the model pack with the photometry's filters, creates the GPU context and stages everything.  Throws on error.
void open_session(Session &s, int n_pops, bool need_phot);

// --gpus N (or gpu.gpus): when this process is not yet a rank of a launch, starts N copies of itself -- one per GPU, with
// B9_RANK / B9_WORLD_SIZE / B9_LOCAL_RANK / B9_DIST_DIR set -- BEFORE anything touches a GPU, waits for them and
// returns their worst exit code through *exit_code (true = the caller is the launcher and must exit with that code).
bool launch_ranks_if_requested(int argc, char **argv, int *exit_code);

// Adaptive Metropolis ([RECALL] the staged burn-in of MpiMcmcApplication): burn-in with the proposal adapted after
// every block from the pooled rows of all walkers (all GPUs), then the main run with the proposal frozen.  Burn-in rows
// are written with stage 1..2, the main run with stage 3, walkers in id order within a step; with several ranks every
// rank writes a part file and rank 0 merges them into <output_base>.res.
McmcResult run_mcmc(Session &s, Exchange &exchange, const std::vector<std::string> &columns);

// Rank 0's merge of <final_path>.part<r>, r < world (each `rows_per_part` data rows, `per` walkers per step and rank), into
// <final_path>: comment + header of part 0, then the steps' rows in walker order.  Throws -- keeping every part file and
// leaving no merged file -- when a part is short, long or unreadable, or the output cannot be written; removes the parts
// only after the merged file is complete.
void merge_result_parts(const std::string &final_path, int world, int per, long rows_per_part);

// The rows of a chain file (.res) whose stage column equals `stage` (3 = main run), as full parameter rows: B9_NPARAM doubles
// each, `start` with the file's sampled columns written over it.  Leading lines starting with '#' are skipped; the header
// names the sampled parameters, then "logPost stage"; a column that is no parameter name is an error; data lines that do
// not hold one number per column are skipped.  Throws when the file cannot be read, is empty or has a malformed header.
// What sampleMass and sampleWDMass read (libbase9host exports it as b9h_read_res_rows).
// log_post (may be null): the rows' logPost column, empty when the file has none.
std::vector<double> read_res_rows(const std::string &res_path, const std::vector<double> &start, int stage, std::vector<double> *log_post = nullptr);

// What every program over a saved chain does before its own work, from s.settings: opens the session with the grid's
// population count, sets the options {given-mass mode, n_pops, K, Q} -- K = 0 (sampleWDMass, wdSummary: their calls read the
// population count alone) leaves open_session's -- and reads the main-run (stage 3) rows of <output_base>.res.  Throws
// "<path> holds no main-run (stage 3) rows" when there are none.
struct SavedChain {
    std::vector<double> rows;             // [n_rows][B9_NPARAM]
    std::vector<double> log_post;         // [n_rows] (empty: the file has no logPost column)
    long n_rows = 0;
    const double *row(long r) const { return rows.data() + (size_t)r * B9_NPARAM; }
};
SavedChain open_saved_chain(Session &s, const ChainGrid &g);
// The catalogue indices of the WD-stage stars in .phot order, checked against the staged catalogue's b9_n_wd_stars.  Throws
// "... no WD-stage star (stage 3): nothing to <nothing_to>" when there is none.
std::vector<int> wd_stage_stars(const Session &s, const char *nothing_to);

int report_and_exit_code(const char *prog, const std::exception &e);

}  // namespace b9h
