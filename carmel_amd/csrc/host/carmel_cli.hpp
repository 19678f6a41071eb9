// carmel_cli.hpp — the `carmel` front end's shared state and its stages.  run() (carmel_main.cpp) is the list of stages; a
// Job carries what they share: carmel_options.cpp parses, carmel_ranks.cpp forks the --gpus ranks and makes the communicator,
// carmel_load.cpp reads, composes and creates the trainer, carmel_decode.cpp / carmel_em.cpp / carmel_gibbs.cpp do the work,
// carmel_output.cpp writes the files.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <limits>
#include <memory>
#include <sstream>
#include "cli_util.hpp"
#include "compose.hpp"
#include "wfst.hpp"

inline std::string base2(double ln_value) {  // weight.h:529-532,603 as_base(2) at the stream's default precision
  char buf[64];
  std::snprintf(buf, sizeof buf, "2^%.6g", ln_value / std::log(2.0));
  return buf;
}
// Weight::ppxper (weight.h:311, 435-440): the n-th root of 1/p -- except that the root of a ZERO weight is ZERO
// (WEIGHT_CORRECT_ZERO), so a corpus of probability 0 reports perplexity 2^-inf and counts as "best"; kept, because
// the reference's iteration control then behaves the same way
inline double ppxper(double ln_p, double n) {
  return ln_p == -std::numeric_limits<double>::infinity() ? ln_p : -ln_p / n;
}
inline bool timing_on() { return std::getenv("CARMEL_TIMING") != nullptr; }  // per-stage wall clock on stderr

struct UsageError : std::runtime_error {
  explicit UsageError(const std::string& m) : std::runtime_error(m) {}
};

struct Options {
  bool flags[256] = {false};
  bool train_cascade = false;
  long restarts = 0;         // -! (train_opts::ran_restarts)
  // random_restart_acceptor (fst.h:999-1044; carmel.cc:1426-1430, 1741-1749); 0 = unset
  double restart_tolerance = 0, final_restart_tolerance = 0;
  long final_restart = 0;
  double rate_growth = 1.0;  // -o (train_opts::learning_rate_growth_factor, fst.h:1083)
  long max_iter = 500;  // train_opts default (fst.h:1080-1095); -1 == "-M" without a number
  double converge = 1e-4, converge_ppx_ratio = .999, smooth_floor = 0;
  int norm = CARMEL_HIP_NORM_CONDITIONAL;
  std::string normby, priors, out_file, digamma;
  bool have_digamma = false;       // --digamma=... (carmel.cc:495)
  bool plus_alpha_set = false;     // -+ a (carmel.cc:1009-1013): mean-field scale of the single transducer's method
  double plus_alpha = 0;
  int index_threshold = 32, gpu = 0;
  int gpus = 1;  // --gpus=N: corpus-sharded EM, one process per GPU (not a carmel option: carmel is single-process)
  std::string comm_plugin;  // --comm-plugin=LIB.so: a transport of the caller's own instead of RCCL (carmel_hip_comm_create_custom);
                            // every rank then runs on the device --gpu names (the transport decides where the data travels)
  bool random_set = false;  // --random-set (carmel.cc:609-612, 786-789): a new weight on (0..1] for every unlocked arc before training
  int exchange_form = 0;    // --exchange=auto|allreduce|collectives|direct (carmel_hip_exchange_plan's form)
  int exchange_chunks = 0;  // --exchange-chunks=K: arc-range chunks of the sharded count exchange (0: the library's default)
  // --crp (carmel.cc:255-304)
  bool expectation = false;  // --expectation (gibbs_opts.hpp:125)
  long crp_restarts = 0;     // --crp-restarts (carmel.cc:271-273)
  long init_em = 0;          // --init-em=N, --em-p0 (carmel.cc:276-277; gibbs.cc:400-423)
  bool em_p0 = false;
  bool init_from_p0 = false;   // --init-from-p0 (carmel.cc:298; gibbs.cc:405-421)
  bool cache_no_prune = false;     // --cache-no-prune
  bool stream_lattices = false;    // --disk-cache-derivations (carmel.cc:243-246): do not keep every pair's lattice resident
  uint64_t resident_bytes = 0;     // --disk-cache-bufsize=SIZE[K|M|G]: how much lattice memory may be resident at a time (0: 64 GB)
  bool matrix_fb = false;          // --matrix-fb (carmel.cc:238)
  bool gpu_compose = false;        // --gpu-compose: the product construction of the composition on the GPU (compose.hip)
  // prior-scale inference (carmel.cc:291-294, 497; gibbs.hpp:525-563)
  double pi_stddev = 0;
  bool pi_global = false, pi_restart_fresh = false, pi_show = false;
  std::string prior_groupby;
  long number_from = 0;            // --number-from=N (carmel.cc:768, 802-806)
  std::string write_loaded;        // --write-loaded=suffix (carmel.cc:758, 807)
  bool have_write_loaded = false;
  bool sample_prob_after = false;  // --sample-prob-after: log the add-back proposal probability (carmel_hip_gibbs_run_ex)
  bool crp_argmax_final = false, crp_argmax_sum = false;
  bool include_self = false, random_start = false;  // gibbs_opts.hpp:40-41, 127-128
  long print_every = 0;                              // gibbs_opts.hpp:78-79
  // the sampler's tables (gibbs_opts.hpp:64-77, 142-146, 197-203; gibbs.hpp:970-1078): parameter ids [from, to) of the count
  // table, norm-group ids [from, to) of the norm sums; 4294967295 = to the end
  unsigned long print_counts_from = 0, print_counts_to = 0, print_norms_from = 0, print_norms_to = 0;
  double print_counts_sparse = 0;
  bool rich_counts = false, norm_order = false;
  long width = 7;
  std::string fem_forest, fem_norm, fem_param, fem_alpha;  // forest-em export (carmel.cc:756-769, 818-831)
  long print_from = 0, print_to = 0;  // --print-from=m --print-to=n (gibbs_opts.hpp; gibbs.cc:258-296): the final sample's
                                      // path through input transducers m .. n-1, one line each, on stdout
  std::string fem_early_param;                             // --fem-early-param: the weights as loaded / normalised (carmel.cc:801)
  std::string load_fem_param;                              // --load-fem-param (carmel.cc:790-799; cascade.h:180-202)
  bool crp = false, crp_parallel = false, uniform_p0 = false, dirichlet_p0 = false, final_counts = false,
       exclude_prior = false;
  long crp_iters = -1, burnin = 0;
  double high_temp = 1, low_temp = 1;  // --high-temp / --low-temp (carmel.cc:289-290)
  unsigned long long seed = 1;
  long kpaths = 0;  // -k n (carmel.cc:1021): best paths per line; only n = 1 with -b / -i (batch decoding, decode_batch)
  long kbest = 0;   // --kbest=N: N best paths per line (print_kbest(N, ...), carmel.cc:379-397), where -k 1 is accepted
  bool have_kbest = false;
  long sample_paths = 0;  // --sample-paths=N: N derivations per line drawn from the posterior over the line's derivations
  bool have_sample = false;  // (carmel_hip_decode_sample, seeded by -R); not carmel's -G, which generates from the whole machine
  std::string posterior_counts;  // --posterior-counts=FILE: the composed machine with every arc's expected count over all derivations
  bool have_posterior = false;   // of the lines as its weight (carmel_hip_decode_posterior), written to FILE
  std::string pair_lines;  // --pair-lines=FILE (carmel's --post-b=FILE): line k of FILE is the other side's line of line k; every pair's
  bool have_pair_lines = false;  // best derivation is printed in place of the line's (carmel_hip_decode_pairs)
  std::string pair_alignments;   // --pair-alignments=OUT: every pair's best path as in:out symbol pairs, one line a pair
  bool have_pair_alignments = false;
  std::string pair_counts;       // --pair-counts=FILE: the composed machine with every arc's expected count over all derivations
  bool have_pair_counts = false;  // of the pairs as its weight (carmel_hip_decode_pairs_posterior), written to FILE
  long pair_samples = 0;          // --pair-samples=N: N alignments per pair drawn from the posterior over the pair's derivations
  bool have_pair_samples = false;  // (carmel_hip_decode_pairs_sample, seeded by -R), printed in place of the pair's best derivation
  long pair_kbest = 0;            // --pair-kbest=N: the N best alignments of every pair (carmel_hip_decode_pairs_kbest), printed best
  bool have_pair_kbest = false;   // first in place of the pair's best derivation; --kbest=N for the pairs of --pair-lines
  // --generate-paths=N (carmel's -G N) / --generate-pairs=N (carmel's -g N): N random paths / (input, output) pairs drawn from the
  // composed machine itself (carmel_hip_decoder_generate, seeded by -R); --generate-max-arcs=L is carmel's -L, --generate-tries=T
  // bounds the attempts a path may take
  long generate_paths = 0, generate_pairs = 0, generate_max_arcs = 1000, generate_tries = 256;
  bool have_generate_paths = false, have_generate_pairs = false, have_generate_max_arcs = false, have_generate_tries = false;
  long best_paths = 0;  // --best-paths=N (carmel's -k N without -b / -i): the N best paths of the composed machine itself
  bool have_best_paths = false;  // (carmel_hip_decoder_best_paths)
  // --prune-paths=W (carmel's -w w), --prune-states=N (-z n), --prune-arcs=W (-p w): the composed machine is pruned by best-path
  // weight before it is printed (carmel_hip_decoder_prune): ln of the ratio (below 1: 1), the state cap, ln of the arc threshold
  double prune_log_ratio = std::numeric_limits<double>::infinity(), prune_min_arc_logw = -std::numeric_limits<double>::infinity();
  long prune_states = 0;
  bool have_prune_paths = false, have_prune_states = false, have_prune_arcs = false;
  // -C (carmel's own switch: WFST::consolidateArcs): arcs of the composed machine with the same source, destination, input and
  // output become one arc of their summed weight (carmel_hip_consolidate); --consolidate-max keeps the largest weight instead,
  // --consolidate-unclamped lets a sum exceed 1
  bool consolidate_max = false, consolidate_unclamped = false;
  // --machine-sums: in place of the composed machine, the number of its paths and the sum of their weights
  // (carmel_hip_decoder_machine_sums); --machine-counts=FILE implies it and writes the machine with every arc's expected count
  // under the machine's own path distribution as its weight
  bool machine_sums = false, have_machine_counts = false;
  std::string machine_counts;
  bool sum = false;  // --sum-paths with -b / -i (carmel's --sum): the report also multiplies the lines' sums of all paths (report_batch, carmel.cc:354-377)
  std::vector<const char*> files;
};

struct CorpusStats {  // training_corpus counters over the pairs that have a derivation (train.h:151-168)
  double n_pairs = 0, total_weight = 0, n_input = 0, n_output = 0;
};

// One invocation: the options, this process's place among the --gpus ranks, the transducers and their composition, the
// corpus (this rank's shard of it), and the trainer with its communicator.
struct Job {
  Options o;
  int rank = 0, world = 1;
  bool quiet = false;
  int wstyle = 0;  // weight output (format_weight's style)
  size_t nw = 0;   // input transducers
  std::vector<carmel_host::Transducer> member;
  // normalisation methods per member (carmel.cc:488-499)
  std::vector<int> norms, priorgroup;
  std::vector<double> addc, dig_alpha;
  std::vector<uint8_t> dig_on;
  bool any_digamma = false;
  carmel_host::ParamTable params;
  carmel_host::ChainTable chains;
  std::unique_ptr<carmel_host::Transducer> composed;
  carmel_host::Transducer* result = nullptr;  // the composition (the only member when there is one)
  bool cascade = false;
  carmel_host::HostPairs pairs;
  std::vector<uint32_t> src, dst, in, out, group;  // result, flattened
  std::vector<double> logw;
  std::vector<uint64_t> coff, cpar;  // the chains of the cascade, flattened
  carmel_hip_trainer* t = nullptr;
  carmel_hip_comm* comm = nullptr;
  // --disk-cache-derivations with lattices beyond --disk-cache-bufsize: the corpus in shards of pairs [stream_cut[k], stream_cut[k+1]),
  // never more than one shard's lattices resident (set by train_em; empty: everything is resident)
  std::vector<size_t> stream_cut;
  bool streaming = false, stream_prune = true;

  Job() = default;
  Job(const Job&) = delete;
  bool comm_made = false;  // create_communicator returned (comm stays null when world == 1)
  ~Job() {  // the communicator goes first (a null one too, once made), then the trainer it summed the counts of
    if (comm_made) carmel_hip_comm_destroy(comm);
    if (t) carmel_hip_destroy(t);
  }
  size_t n_params() const { return cascade ? params.logw.size() : logw.size(); }
  std::vector<const carmel_host::Transducer*> members() const;  // the cascade's members, or the single result
  void set_methods(const std::vector<double>& add);  // the members' normalisation methods with these --priors
  void set_corpus_range(size_t lo, size_t hi);
  void set_whole_corpus();
};

// ---- the stages, in the order run() goes through them ----
Options parse_args(int argc, char** argv);                                 // carmel_options.cpp
bool fork_ranks(Job& j);                                                   // carmel_ranks.cpp
void create_communicator(Job& j, int my_device);
void shard_pairs(Job& j);
void report_error(const char* what);
int wait_for_ranks(int rc);
std::string slurp(const char* fn);                                         // carmel_load.cpp
int load_members(Job& j);
int compose_members(Job& j);
void read_corpus(Job& j, const std::string& corpus_text, bool weight_lines);
void create_trainer(Job& j);
int score_pairs(Job& j);
void begin_training(Job& j);
int decode_batch(const Options& o, carmel_host::Transducer& M, const std::string& text, int ws, bool quiet, int device);  // carmel_decode.cpp
int generate_batch(const Options& o, carmel_host::Transducer& M, int ws, int device);
int best_paths_batch(const Options& o, carmel_host::Transducer& M, int ws, int device);
int prune_composition(const Options& o, carmel_host::Transducer& M, bool quiet, int device);
int consolidate_composition(const Options& o, carmel_host::Transducer& M, bool quiet, int device);
int machine_sums_composition(const Options& o, carmel_host::Transducer& M, int ws, int device);
void log_lattice_stats(const carmel_hip_lattice_stats& ls, size_t n);      // carmel_em.cpp
void train_em(Job& j, const Options& iteration_controls);
int train_gibbs(Job& j);                                                   // carmel_gibbs.cpp
void write_loaded(const Job& j);                                           // carmel_output.cpp
void write_fem_forest(Job& j);
void write_fem_side_files(Job& j);
void write_trained_members(Job& j, const double* pw);
int write_single(Job& j);
// the norm groups of a member in NormGroupIter's order: f(index of the state's first arc within the member, the group's arcs
// as indices within the state)
void for_each_norm_group(const carmel_host::Transducer& m, int norm, const std::function<void(size_t, const std::vector<size_t>&)>& f);
