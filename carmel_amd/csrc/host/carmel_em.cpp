// carmel_em.cpp — EM training: WFST::train (train.cc:503-678) restated over the trainer of a Job; every E-step and M-step runs
// on the GPU.  EM log lines on stderr have the reference's wording (train.cc:587-613, 639-657, 669-671).
#include "carmel_cli.hpp"
using namespace carmel_host;

// A corpus every pair of which has probability 1: the reference's log-domain arithmetic lands on ln P = 0 exactly (a count
// divided by itself, weight.h:737-830) and its convergence test becomes the quotient of two zeros (weight.h:247-249,
// train.cc:611,630: the run goes on to -M); sums of exponentials land within an ulp or two of it, on either side, and the
// same test then sees a ratio of -1e16 or 1.  A corpus probability within two ulps per pair of 1 therefore counts as 1.
static void snap_certain(carmel_hip_estimate_result* er) {
  const double tol = 4.45e-16 * (double)std::max<uint64_t>(er->n_pairs, 1);
  if (std::fabs(er->sum_logprob) <= tol) er->sum_logprob = 0.0;
  if (std::fabs(er->sum_weighted_logprob) <= tol) er->sum_weighted_logprob = 0.0;
}
// shard by shard: lattices rebuilt, swept, dropped; the count buffers (counts + corpus scalars) added up on the device.
// A shard none of whose pairs has a derivation adds zeros: the reference gives up only when NO pair of the corpus has one
// (train.cc:241-252; train_em checks the summed count of kept pairs)
static void estimate_streamed(Job& j, carmel_hip_estimate_result* er) {
  carmel_hip_trainer* t = j.t;
  hip_check(carmel_hip_accumulate_counts(t, 0), "carmel_hip_accumulate_counts");
  for (size_t k = 0; k + 1 < j.stream_cut.size(); ++k) {
    j.set_corpus_range(j.stream_cut[k], j.stream_cut[k + 1]);
    hip_check(carmel_hip_build_lattices(t, j.stream_prune ? 1 : 0, 0, nullptr, nullptr), "carmel_hip_build_lattices");
    hip_check(carmel_hip_estimate_async(t), "carmel_hip_estimate_async");
    hip_check(carmel_hip_accumulate_counts(t, 1), "carmel_hip_accumulate_counts");
  }
  hip_check(carmel_hip_accumulate_counts(t, 2), "carmel_hip_accumulate_counts");
  if (j.comm) hip_check(carmel_hip_allreduce_counts(t, j.comm), "carmel_hip_allreduce_counts");
  hip_check(carmel_hip_read_scalars(t, er), "carmel_hip_read_scalars");
}
// one E-step over the whole corpus: the count pass on this rank's shard, then (N > 1) the sum over the ranks
static void estimate_all(Job& j, carmel_hip_estimate_result* er) {
  carmel_hip_trainer* t = j.t;
  if (j.streaming)
    estimate_streamed(j, er);
  else if (!j.comm)
    hip_check(carmel_hip_estimate(t, er, 0), "carmel_hip_estimate");
  else {
    hip_check(carmel_hip_estimate_async(t), "carmel_hip_estimate_async");
    hip_check(carmel_hip_allreduce_counts(t, j.comm), "carmel_hip_allreduce_counts");
    hip_check(carmel_hip_read_scalars(t, er), "carmel_hip_read_scalars");
  }
  snap_certain(er);
}

// `log << derivations::global_stats` of cache_derivations (cached_derivs.h:137; derivations.h:197-247), printed whenever
// the derivations are cached (-? -: --crp).  What the reference prints as "Pre pruning: (S states, A arcs)" is A summed
// over all pairs but S of the LAST pair, and "Post pruning" is the last pair that has a derivation (see
// carmel_hip_lattice_stats).  Its two "Avg # of paths" lines are not produced.
void log_lattice_stats(const carmel_hip_lattice_stats& ls, size_t n) {
  const double s0 = (double)ls.last_pair_explored_states, a0 = (double)ls.explored_arcs, s1 = (double)ls.last_pair_kept_states,
               a1 = (double)ls.last_pair_kept_arcs;
  std::cerr << "\nTotal for " << n << " cached derivations:\nPre pruning: (" << s0 << " states, " << a0
            << " arcs)\nPost pruning: (" << s1 << " states, " << a1 << " arcs)\nPortion kept: (" << (s0 ? s1 / s0 : 0.0)
            << " states, " << (a0 ? a1 / a0 : 1.0) << " arcs)\n";
}

// rank-local -- pairs.size() is this rank's shard, yet decide_streaming's all-reduce of any_over sits under it
static bool may_stream(const Job& j, const Options& o) {
  return o.stream_lattices && !o.crp && !o.matrix_fb && j.pairs.size() > 1;  // (--matrix-fb keeps no lattices)
}
// how much GPU memory do this corpus' lattices take?  A probe of its first pairs says (explicit lattices: the shards' count
// buffers must mean the same thing, carmel_hip_accumulate_counts); sets j.streaming and j.stream_cut
static void decide_streaming(Job& j, const Options& o) {
  carmel_hip_trainer* t = j.t;
  hip_check(carmel_hip_set_layout_policy(t, 0), "carmel_hip_set_layout_policy");
  const size_t n = j.pairs.size(), probe = std::min<size_t>(n, 16384);
  j.set_corpus_range(0, probe);
  carmel_hip_lattice_stats ps;
  hip_check(carmel_hip_build_lattices(t, j.stream_prune ? 1 : 0, 0, nullptr, &ps), "carmel_hip_build_lattices");
  const double per_pair = (double)ps.device_bytes / (double)probe;
  const double cap = o.resident_bytes ? (double)o.resident_bytes : 64.0 * 1024 * 1024 * 1024;
  // the ranks decide TOGETHER: a rank that streams keeps explicit lattices, plans no exchange and issues the plain all-reduce
  // once per iteration, so if one shard of the corpus is over its budget every rank streams (its own lattices in as many
  // shards as its own probe says, one if they fit) -- ranks on either side of the threshold would otherwise wait in
  // different collectives, or add up count buffers that mean different things
  double any_over[1] = {per_pair * (double)n > cap ? 1.0 : 0.0};
  if (j.comm) hip_check(carmel_hip_comm_allreduce_host(j.comm, any_over, 1, 1), "carmel_hip_comm_allreduce_host");
  j.streaming = any_over[0] != 0.0;
  if (j.streaming) {
    const size_t per_shard = std::max<size_t>(64, (size_t)std::min<double>(cap / std::max(per_pair, 1.0), 1e18));
    for (size_t lo = 0; lo < n; lo += per_shard) j.stream_cut.push_back(lo);
    j.stream_cut.push_back(n);
    if (!j.quiet)
      std::cerr << "Derivation lattices of " << n << " pairs would take about " << (uint64_t)(per_pair * (double)n) << " bytes of GPU memory; with "
                << (uint64_t)cap << " allowed they are rebuilt every iteration in " << j.stream_cut.size() - 1 << " shards of " << per_shard << " pairs\n";
  }
}
// the streamed first pass: which pairs have a derivation, and the statistics of all shards
static void build_streamed(Job& j, std::vector<uint8_t>& has, carmel_hip_lattice_stats& ls) {
  std::memset(&ls, 0, sizeof ls);
  for (size_t k = 0; k + 1 < j.stream_cut.size(); ++k) {
    j.set_corpus_range(j.stream_cut[k], j.stream_cut[k + 1]);
    carmel_hip_lattice_stats ps;
    hip_check(carmel_hip_build_lattices(j.t, j.stream_prune ? 1 : 0, 0, has.data() + j.stream_cut[k], &ps), "carmel_hip_build_lattices");
    ls.n_pairs += ps.n_pairs;
    ls.n_pairs_kept += ps.n_pairs_kept;
    ls.explored_states += ps.explored_states;
    ls.explored_arcs += ps.explored_arcs;
    ls.kept_states += ps.kept_states;
    ls.kept_arcs += ps.kept_arcs;
    ls.n_cyclic_pairs += ps.n_cyclic_pairs;
    ls.n_bundles += ps.n_bundles;
    ls.max_levels = std::max(ls.max_levels, ps.max_levels);
    ls.device_bytes = std::max(ls.device_bytes, ps.device_bytes);
    ls.build_seconds += ps.build_seconds;
    ls.last_pair_explored_states = ps.last_pair_explored_states;
    if (ps.n_pairs_kept) {
      ls.last_pair_kept_states = ps.last_pair_kept_states;
      ls.last_pair_kept_arcs = ps.last_pair_kept_arcs;
    }
    ls.n_windowed_pairs += ps.n_windowed_pairs;
  }
}
// every rank must hold its lattices in the same layout (a shard with one over-long pair would keep explicit lattices
// while the others unroll, and the count buffers being summed would mean different things): agree, or rebuild all
// with explicit lattices
static void agree_on_layout(Job& j, const Options& o, std::vector<uint8_t>& has, carmel_hip_lattice_stats& ls) {
  carmel_hip_trainer* t = j.t;
  double lay[2] = {(double)carmel_hip_lattice_layout(t), -(double)carmel_hip_lattice_layout(t)};
  hip_check(carmel_hip_comm_allreduce_host(j.comm, lay, 2, 1), "carmel_hip_comm_allreduce_host");
  if (lay[0] != -lay[1]) {
    if (!j.quiet) std::cerr << "The ranks' shards chose different lattice layouts; rebuilding every rank with explicit lattices\n";
    hip_check(carmel_hip_set_layout_policy(t, 0), "carmel_hip_set_layout_policy");
    hip_check(carmel_hip_build_lattices(t, o.cache_no_prune ? 0 : 1, 0, has.data(), &ls), "carmel_hip_build_lattices");
  }
}
// plan the exchange (sharded where the model allows it, csrc/exchange.cpp).  The direct form rests on the transport's
// point-to-point groups: one such group between all ranks, checked, before the plan is made (carmel_hip_comm_selftest); a
// transport that fails it on any rank keeps the ring collectives
static void plan_exchange(Job& j, const Options& o) {
  int form = o.exchange_form;
  if (form == 0 || form == 3) {
    double bad[1] = {carmel_hip_comm_selftest(j.comm, 0) == CARMEL_HIP_OK ? 0.0 : 1.0};
    hip_check(carmel_hip_comm_allreduce_host(j.comm, bad, 1, 1), "carmel_hip_comm_allreduce_host");
    if (bad[0] != 0.0) {
      if (form == 3) throw std::runtime_error("--exchange=direct: the transport's point-to-point self-test failed");
      if (j.rank == 0) std::cerr << "carmel: the transport's point-to-point self-test failed; planning the exchange over the collectives\n";
      form = 2;
    }
  }
  hip_check(carmel_hip_exchange_plan(j.t, j.comm, (uint32_t)o.exchange_chunks, form), "carmel_hip_exchange_plan");
}
// the lattices of this rank's pairs, resident or (beyond the budget) streamed; has[p]: pair p has a derivation
static void prepare_lattices(Job& j, const Options& o, std::vector<uint8_t>& has, carmel_hip_lattice_stats& ls) {
  carmel_hip_trainer* t = j.t;
  j.stream_cut.clear();
  j.streaming = false;
  j.stream_prune = !o.cache_no_prune;
  const bool probed = may_stream(j, o);
  if (probed) decide_streaming(j, o);
  if (j.streaming)
    build_streamed(j, has, ls);
  else {
    if (probed) {  // (the probe left its own corpus and layout policy behind)
      hip_check(carmel_hip_set_layout_policy(t, 1), "carmel_hip_set_layout_policy");
      j.set_whole_corpus();
    }
    hip_check(carmel_hip_build_lattices(t, o.cache_no_prune ? 0 : 1, 0, has.data(), &ls), "carmel_hip_build_lattices");
  }
  if (timing_on())
    std::cerr << "timing: lattices pairs_kept=" << ls.n_pairs_kept << " states=" << ls.kept_states << " arcs=" << ls.kept_arcs
              << " layout=" << (carmel_hip_lattice_layout(t) == 2 ? "unrolled_dense" : carmel_hip_lattice_layout(t) == 1 ? "unrolled" : "explicit") << " device_bytes=" << ls.device_bytes
              << " build_seconds=" << ls.build_seconds << std::endl;
  if (j.comm && !o.crp && !j.streaming) agree_on_layout(j, o, has, ls);
  if (o.matrix_fb) {  // train.cc:381-383
    if (j.rank == 0) std::cerr << "Using (input,state,output) full matrix, not derivation lattice.  Usually slower.\n";
    hip_check(carmel_hip_set_matrix_fb(t, 1), "carmel_hip_set_matrix_fb");
  }
  // (after --matrix-fb: the matrix E-step leaves no arc-range-ordered count pass to hang reduce-scatters on, so its exchange is
  // planned as the one all-reduce; csrc/exchange.cpp)
  // (streamed lattices: every shard has its own buckets, so the exchange stays the plain all-reduce of the summed buffer)
  if (j.comm && !o.crp && !j.streaming) plan_exchange(j, o);
  if (o.flags[(unsigned)'?'] || o.flags[(unsigned)':']) log_lattice_stats(ls, j.pairs.size());
}

static CorpusStats corpus_stats(Job& j, const Options& o, const std::vector<uint8_t>& has, const carmel_hip_lattice_stats& ls) {
  const HostPairs& pairs = j.pairs;
  CorpusStats cs;
  for (size_t p = 0; p < pairs.size(); ++p) {
    if (!has[p]) {
      std::cerr << "No derivations in transducer for input/output #" << (p + 1) << "\n";  // cached_derivs.h:54-58
      continue;
    }
    cs.n_pairs += 1;
    cs.total_weight += pairs.weight[p];
    cs.n_input += (double)(pairs.in_off[p + 1] - pairs.in_off[p]);
    cs.n_output += (double)(pairs.out_off[p + 1] - pairs.out_off[p]);
  }
  if (ls.n_cyclic_pairs)
    std::cerr << "Warning: at least one cycle in derivations for " << ls.n_cyclic_pairs
              << " example(s).  Forward/backward will miss some paths.\n";  // derivations.h:726-728
  if (j.comm && !o.crp) {  // the counters of training_corpus over ALL ranks' surviving pairs (--crp: every rank has the whole corpus)
    double v[5] = {cs.n_pairs, cs.total_weight, cs.n_input, cs.n_output, (double)ls.n_cyclic_pairs};
    hip_check(carmel_hip_comm_allreduce_host(j.comm, v, 5, 0), "carmel_hip_comm_allreduce_host");
    cs.n_pairs = v[0];
    cs.total_weight = v[1];
    cs.n_input = v[2];
    cs.n_output = v[3];
  }
  if (cs.n_pairs == 0) throw std::runtime_error("No training example had a derivation - aborting training.");
  return cs;
}

static void print_ppx(const CorpusStats& cs, double ln_p) {  // weight.h:314-329 print_ppx_symbol
  double n_sym = std::max(cs.n_output, cs.n_input);
  std::cerr << "probability=" << base2(ln_p);
  if (n_sym) std::cerr << " per-symbol-perplexity(N=" << n_sym << ")=" << base2(ppxper(ln_p, n_sym));
  if (cs.n_pairs) std::cerr << " per-example-perplexity(N=" << cs.n_pairs << ")=" << base2(ppxper(ln_p, cs.n_pairs));
}

// "-M" alone: just the corpus perplexity (train.cc:516-517); -M 0, and -M 1 without restarts: one E-step (train.cc:520-538)
static void train_at_most_once(Job& j, const Options& o, const CorpusStats& cs) {
  carmel_hip_estimate_result er;
  if (o.max_iter == 0)
    std::cerr << "0 iterations specified for training; output weights will be unnormalized fractional counts (except locked "
           "arcs).\n";
  estimate_all(j, &er);
  std::cerr << "Corpus ";
  print_ppx(cs, er.sum_logprob);
  if (o.max_iter == 0)  // prep_new_weights(1.0) + cascade.distribute_counts()
    hip_check(carmel_hip_fractional_counts(j.t), "carmel_hip_fractional_counts");
  else if (o.max_iter != -1) {
    double mc;
    hip_check(carmel_hip_maximize(j.t, 1.0, &mc), "carmel_hip_maximize");
  }
  std::cerr << "\n";
}

struct EmRun {  // what the random restarts of one training run share (train.cc:540-551)
  const CorpusStats& cs;
  bool timing;  // per-iteration wall clock on stderr
  double best = std::numeric_limits<double>::infinity(), best_start = best;
  bool have_good = false;
  double growth = 1.0;
};
struct EmStart {  // one start's iteration state (train.cc:553-560)
  double last_ppx = std::numeric_limits<double>::infinity(), last_change = 10.0;
  bool last_was_reset = false;
  long iter = 0;
  double learning_rate = 1.0;
};

// random_restart_acceptor::accept (fst.h:1017-1040)
static bool accept_restart(const Options& o, unsigned restart_no, double new_ppx, double best_start) {
  const double inf = std::numeric_limits<double>::infinity();
  const double tol = o.restart_tolerance > 0 ? std::log(o.restart_tolerance) : inf;  // ln domain
  const double fin = o.final_restart_tolerance > 0 ? std::log(o.final_restart_tolerance) : tol;
  const double N = o.final_restart ? (double)o.final_restart : (double)o.restarts;
  const double lr = restart_no >= N ? fin : tol == inf ? tol : tol + (fin - tol) * ((restart_no - 1) / (N - 1));
  const double ppr = (new_ppx - best_start) / std::fabs(new_ppx);  // weight.h:247-249
  const bool ok = lr > ppr;
  std::cerr << "For restart " << restart_no << ", " << (ok ? "accepting" : "rejecting") << " worse random start of "
      << base2(new_ppx) << " compared to " << base2(best_start) << " with relative ppx ratio="
      << format_weight(ppr, W_SOMETIMES_LOG) << " compared to target of "
      << (lr == inf ? std::string("inf") : format_weight(lr, W_SOMETIMES_LOG)) << "\n";
  if (!ok) std::cerr << "Random start was insufficiently promising; trying another." << std::endl;
  return ok;
}

enum Next { GO_ON, AGAIN, STOP };  // to the M-step; straight to the next E-step; this start is over
// the convergence test on the perplexity ratio, and the learning rate of over-relaxed EM (train.cc:630-650)
static Next test_convergence(Job& j, const Options& o, const EmRun& run, EmStart& s, double ratio_ln) {
  if (s.last_was_reset) {
    s.last_was_reset = false;
    return GO_ON;
  }
  if (ratio_ln >= std::log(o.converge_ppx_ratio)) {
    if (s.learning_rate > 1) {  // train.cc:639-643
      std::cerr << "Failed to improve (relaxation rate too high); starting again at learning rate 1" << std::endl;
      s.learning_rate = 1;
      hip_check(carmel_hip_keep_em_weights(j.t), "carmel_hip_keep_em_weights");
      s.last_was_reset = true;
      return AGAIN;
    }
    std::cerr << "Converged - per-example perplexity ratio exceeds "
        << format_weight(std::log(o.converge_ppx_ratio), W_SOMETIMES_LOG) << " after " << s.iter << " iterations.\n";
    if (!run.have_good)
      std::cerr << "Because of the --train-cascade implementation, we need another iteration even though we've "
             "converged.\n";
    else
      return STOP;
  } else if (s.learning_rate < 20) {  // MAX_LEARNING_RATE_EXP (train.cc:647)
    s.learning_rate *= run.growth;
  }
  return GO_ON;
}

// one iteration (train.cc:562-657): E-step, log line, best-so-far, convergence, M-step; false: this start is over
static bool em_iteration(Job& j, const Options& o, EmRun& run, EmStart& s, unsigned restart_no) {
  carmel_hip_trainer* t = j.t;
  const CorpusStats& cs = run.cs;
  carmel_hip_estimate_result er;
  const bool first_time = s.iter == 0;
  ++s.iter;
  const long iter = s.iter;
  const bool cascade_counts = j.cascade && !first_time;
  if (cascade_counts) hip_check(carmel_hip_save_counts(t), "carmel_hip_save_counts");
  if (iter > o.max_iter && run.have_good) {
    std::cerr << "Maximum number of iterations (" << o.max_iter
        << ") reached before convergence criteria was met - greatest arc weight change was "
        << format_weight(std::log(s.last_change), W_SOMETIMES_LOG) << "\n";
    return false;
  }
  const auto t_e0 = std::chrono::steady_clock::now();
  if (iter > 2 * o.max_iter + 2 && !run.have_good) {
    // the reference keeps iterating until some iteration was accepted as best (train.cc:577); with a corpus
    // probability of zero or NaN that never happens: stop instead of spinning
    throw std::runtime_error("no iteration produced a usable corpus probability; giving up after " + std::to_string(iter - 1) + " iterations");
  }
  estimate_all(j, &er);
  if (run.timing) {
    double sweep_ms = 0;
    carmel_hip_last_sweep_ms(t, &sweep_ms);
    std::cerr << "timing: i=" << iter << " estimate " << std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_e0).count()
        << " ms (kernels " << sweep_ms << " ms)" << std::endl;
  }
  const double new_ppx = ppxper(er.sum_weighted_logprob, cs.total_weight);  // ln p.ppxper(totalEmpiricalWeight)
  std::cerr << "i=" << iter << " (rate=" << s.learning_rate << "): ";
  print_ppx(cs, er.sum_logprob);
  if (new_ppx < run.best && (!j.cascade || cascade_counts)) {
    std::cerr << " (new best)";
    run.best = new_ppx;
    run.have_good = true;
    hip_check(carmel_hip_save_best(t), "carmel_hip_save_best");
  }
  double ratio_ln = kNegInf;
  if (first_time) {
    std::cerr << std::endl;
    if (restart_no == 0) {
      run.best_start = new_ppx;
      std::cerr << "Initial best start point ppx=" << base2(new_ppx) << "\n";
    } else if (!accept_restart(o, restart_no, new_ppx, run.best_start))
      return false;  // to the next random restart
  } else {
    ratio_ln = (new_ppx - s.last_ppx) / std::fabs(new_ppx);  // weight.h:247-249
    std::cerr << " (relative-perplexity-ratio=" << format_weight(ratio_ln, W_SOMETIMES_LOG) << ")";
    if (s.last_change < 1) std::cerr << ", max {d(weight)}=" << format_weight(std::log(s.last_change), W_SOMETIMES_LOG);
    std::cerr << std::endl;
  }
  const Next next = test_convergence(j, o, run, s, ratio_ln);
  if (next != GO_ON) return next == AGAIN;
  const auto t_m0 = std::chrono::steady_clock::now();
  hip_check(carmel_hip_maximize(t, s.learning_rate, &s.last_change), "carmel_hip_maximize");
  if (run.timing)
    std::cerr << "timing: i=" << iter << " maximize " << std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_m0).count() << " ms" << std::endl;
  if (s.last_change <= o.converge && run.have_good) {
    std::cerr << "Converged - maximum weight change less than " << format_weight(std::log(o.converge), W_SOMETIMES_LOG)
        << " after " << iter << " iterations.\n";
    return false;
  }
  s.last_ppx = new_ppx;
  return true;
}

// the starts of one training run: the given weights, then -! random restarts (train.cc:540-678)
static void train_with_restarts(Job& j, const Options& o, const CorpusStats& cs) {
  EmRun run{cs, timing_on()};
  run.growth = o.rate_growth;
  if (j.cascade && run.growth != 1.0) {  // train.cc:545-549
    std::cerr << "Overrelaxed EM not supported for --train-cascade (compose with -a and train, instead?).  Disabling (growth factor=1)." << std::endl;
    run.growth = 1.0;
  }
  long restarts_left = o.restarts;
  for (unsigned restart_no = 0;; ++restart_no) {  // train.cc:552-667
    EmStart s;
    while (em_iteration(j, o, run, s, restart_no)) {}
    if (restarts_left > 0) {  // train.cc:660-663
      --restarts_left;
      hip_check(carmel_hip_random_restart(j.t, o.seed, restart_no + 1), "carmel_hip_random_restart");
      std::cerr << "\nRandom restart - " << restarts_left << " remaining.\n";
    } else
      break;
  }
  std::cerr << "Setting weights to model with lowest per-example-perplexity ( = "
         "prod[modelprob(example)]^(-1/num_examples) = 2^(-log_2(p_model(corpus))/N) = "
      << base2(run.best) << std::endl;
  hip_check(carmel_hip_load_best(j.t), "carmel_hip_load_best");
}

// WFST::train (train.cc:503-678) over the trainer with the iteration controls of `o` -- the job's own options, or those of the
// --init-em pass of the sampler (gibbs.cc:411-416), which is why they are a parameter
void train_em(Job& j, const Options& o) {
  std::vector<uint8_t> has(j.pairs.size(), 0);
  carmel_hip_lattice_stats ls;
  prepare_lattices(j, o, has, ls);
  const CorpusStats cs = corpus_stats(j, o, has, ls);
  if (o.max_iter == -1 || o.max_iter == 0 || (o.max_iter == 1 && o.restarts == 0))
    train_at_most_once(j, o, cs);
  else
    train_with_restarts(j, o, cs);
}
