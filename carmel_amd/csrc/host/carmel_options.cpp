// carmel_options.cpp — the command line of the `carmel` front end: one flat table of switches and options (carmel.cc:929-1066).
#include <cctype>
#include "carmel_cli.hpp"
using namespace carmel_host;

Options parse_args(int argc, char** argv) {
  Options o;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    if (a.rfind("--", 0) == 0) {
      std::string k = a.substr(2), v;
      size_t e = k.find('=');
      if (e != std::string::npos) {
        v = k.substr(e + 1);
        k = k.substr(0, e);
      }
      if (k == "train-cascade")
        o.train_cascade = true;
      else if (k == "normby")
        o.normby = v;
      else if (k == "priors")
        o.priors = v;
      else if (k == "gpu")
        o.gpu = std::atoi(v.c_str());
      else if (k == "gpus")
        o.gpus = std::max(1, std::atoi(v.c_str()));
      else if (k == "comm-plugin")
        o.comm_plugin = v;
      else if (k == "random-set")
        o.random_set = true;
      else if (k == "exchange") {
        const char* names[] = {"auto", "allreduce", "collectives", "direct"};
        o.exchange_form = -1;
        for (int f = 0; f < 4; ++f)
          if (v == names[f]) o.exchange_form = f;
        if (o.exchange_form < 0) throw UsageError("--exchange is auto, allreduce, collectives or direct");
      } else if (k == "exchange-chunks")
        o.exchange_chunks = std::max(0, std::atoi(v.c_str()));
      else if (k == "crp") {
        o.crp = true;
        if (!v.empty() && std::atol(v.c_str()) > 1) o.crp_iters = std::atol(v.c_str());
      } else if (k == "burnin")
        o.burnin = std::atol(v.c_str());
      else if (k == "high-temp")
        o.high_temp = std::atof(v.c_str());
      else if (k == "low-temp")
        o.low_temp = std::atof(v.c_str());
      else if (k == "uniform-p0")
        o.uniform_p0 = true;
      else if (k == "dirichlet-p0")
        o.dirichlet_p0 = true;
      else if (k == "fem-forest") {
        o.fem_forest = v;
        o.train_cascade = true;  // force_cascade_derivs (carmel.cc:230-233, 764-767)
        o.flags[(unsigned)'t'] = true;
      } else if (k == "fem-norm")
        o.fem_norm = v;
      else if (k == "fem-param")
        o.fem_param = v;
      else if (k == "fem-alpha")
        o.fem_alpha = v;
      else if (k == "fem-early-param")
        o.fem_early_param = v;
      else if (k == "print-from")
        o.print_from = std::atol(v.c_str());
      else if (k == "print-to")
        o.print_to = std::atol(v.c_str());
      else if (k == "print-every")  // gibbs_opts.hpp:78-79, gibbs.hpp:959-968
        o.print_every = std::atol(v.c_str());
      else if (k == "print-counts-from")
        o.print_counts_from = std::strtoul(v.c_str(), 0, 10);
      else if (k == "print-counts-to")
        o.print_counts_to = std::strtoul(v.c_str(), 0, 10);
      else if (k == "print-norms-from")
        o.print_norms_from = std::strtoul(v.c_str(), 0, 10);
      else if (k == "print-norms-to")
        o.print_norms_to = std::strtoul(v.c_str(), 0, 10);
      else if (k == "print-counts-sparse")
        o.print_counts_sparse = std::atof(v.c_str());
      else if (k == "print-counts-rich")
        o.rich_counts = true;
      else if (k == "norm-order")
        o.norm_order = true;
      else if (k == "width") {
        o.width = std::atol(v.c_str());
        if (o.width < 4) o.width = 20;  // gibbs_opts.hpp:255
      }
      else if (k == "sample-prob" || k == "no-prob" || k == "cache-prob" || k == "cheap-prob" || k == "progress-every") {
        // (--progress-every: the dots gibbs.hpp:845-848 writes into the log while a sweep runs; a sweep is one launch here)
        // inert in carmel itself: gibbs_opts::cache_prob is true and never cleared (carmel.cc:296-298, gibbs_opts.hpp:240,
        // 255-258), so the cache-model probability is what is logged whatever these say
      }
      else if (k == "load-fem-param")
        o.load_fem_param = v;
      else if (k == "restart-tolerance")
        o.restart_tolerance = std::atof(v.c_str());
      else if (k == "final-restart-tolerance")
        o.final_restart_tolerance = std::atof(v.c_str());
      else if (k == "final-restart")
        o.final_restart = std::atol(v.c_str());
      else if (k == "final-counts")
        o.final_counts = true;
      else if (k == "expectation")
        o.expectation = true;
      else if (k == "init-em")
        o.init_em = std::atol(v.c_str());
      else if (k == "em-p0")
        o.em_p0 = true;
      else if (k == "init-from-p0")
        o.init_from_p0 = true;
      else if (k == "gpu-compose")
        o.gpu_compose = true;
      else if (k == "kbest") {  // not a carmel option: -k n with n > 1 (carmel_hip_decode_kbest)
        o.kbest = std::atol(v.c_str());
        o.have_kbest = true;
      }
      else if (k == "sample-paths") {  // not a carmel option: N posterior samples of every line's derivations (carmel_hip_decode_sample)
        o.sample_paths = std::atol(v.c_str());
        o.have_sample = true;
      }
      else if (k == "posterior-counts") {  // not a carmel option: every arc's expected count over the lines (carmel_hip_decode_posterior)
        o.posterior_counts = v;
        o.have_posterior = true;
      }
      else if (k == "pair-lines") {  // carmel's --post-b=FILE under another name (carmel.cc:569-597): --post-b itself stays refused
        o.pair_lines = v;
        o.have_pair_lines = true;
      }
      else if (k == "pair-alignments") {  // not a carmel option: every pair's best path as in:out symbol pairs
        o.pair_alignments = v;
        o.have_pair_alignments = true;
      }
      else if (k == "pair-counts") {  // not a carmel option: every arc's expected count over the pairs (carmel_hip_decode_pairs_posterior)
        o.pair_counts = v;
        o.have_pair_counts = true;
      }
      else if (k == "pair-samples") {  // not a carmel option: N posterior samples of every pair's derivations (carmel_hip_decode_pairs_sample)
        o.pair_samples = std::atol(v.c_str());
        o.have_pair_samples = true;
      }
      else if (k == "pair-kbest") {  // not a carmel option: the N best derivations of every pair (carmel_hip_decode_pairs_kbest)
        o.pair_kbest = std::atol(v.c_str());
        o.have_pair_kbest = true;
      }
      else if (k == "best-paths") {  // carmel's -k N without -b / -i under another name: -k alone stays refused (carmel_main.cpp)
        o.best_paths = std::atol(v.c_str());
        o.have_best_paths = true;
      }
      else if (k == "prune-paths") {  // carmel's -w w under another name (carmel.cc:951-952): -w itself stays refused, below
        if (v.empty() || !parse_weight_token(v, o.prune_log_ratio) || o.prune_log_ratio != o.prune_log_ratio)
          throw UsageError("--prune-paths=W needs a weight (the ratio to the best path's weight: carmel's -w W)");
        if (!(o.prune_log_ratio >= 0.0)) o.prune_log_ratio = 0.0;  // a ratio below 1 becomes 1
        o.have_prune_paths = true;
      }
      else if (k == "prune-states") {  // carmel's -z n (carmel.cc:955)
        char* end = nullptr;
        o.prune_states = std::strtol(v.c_str(), &end, 10);
        if (v.empty() || *end || o.prune_states < 1) throw UsageError("--prune-states=N needs a number N >= 1 (carmel's -z N)");
        o.have_prune_states = true;
      }
      else if (k == "prune-arcs") {  // carmel's -p w (carmel.cc:979)
        if (v.empty() || !parse_weight_token(v, o.prune_min_arc_logw) || o.prune_min_arc_logw != o.prune_min_arc_logw)
          throw UsageError("--prune-arcs=W needs a weight (arcs below it are discarded: carmel's -p W)");
        o.have_prune_arcs = true;
      }
      else if (k == "consolidate-max")  // carmel's own (carmel.cc:1752): with -C, the largest weight of the duplicates, not their sum
        o.consolidate_max = true;
      else if (k == "consolidate-unclamped")  // carmel's own (carmel.cc:1753): with -C, a sum may exceed 1
        o.consolidate_unclamped = true;
      else if (k == "generate-paths") {  // carmel's -G N under another name (carmel.cc:1446-1458): -G itself stays refused, below
        o.generate_paths = std::atol(v.c_str());
        o.have_generate_paths = true;
      }
      else if (k == "generate-pairs") {  // carmel's -g N (carmel.cc:1459-1482)
        o.generate_pairs = std::atol(v.c_str());
        o.have_generate_pairs = true;
      }
      else if (k == "generate-max-arcs") {  // carmel's -L n: here the most arcs a generated path may have, in both modes
        o.generate_max_arcs = std::atol(v.c_str());
        o.have_generate_max_arcs = true;
      }
      else if (k == "generate-tries") {  // not a carmel option: the attempts a path may take (the reference retries for ever)
        o.generate_tries = std::atol(v.c_str());
        o.have_generate_tries = true;
      }
      else if (k == "sum-paths")  // not a carmel option: carmel's --sum with batch decoding (carmel.cc:555-599), every line's sum
        o.sum = true;             // of all paths (carmel_hip_decode_sum); --sum itself stays refused, below
      else if (k == "sum")
        throw UsageError("option --sum is not implemented under that name; with -b or -i use --sum-paths, for the sum over all paths of the composed machine itself --machine-sums");
      else if (k == "machine-sums")  // carmel's --sum without -b / -i (carmel.cc:555-599) and the third line of -c (carmel.cc:841-855)
        o.machine_sums = true;
      else if (k == "machine-counts") {  // not a carmel option: every arc's expected count over the machine's own paths
        o.machine_counts = v;
        o.have_machine_counts = o.machine_sums = true;
      }
      else if (k == "disk-cache-derivations") {
        // carmel.cc:243-246, fst.h:1057-1076: the reference spills its derivation cache to disk when it outgrows memory (and
        // without -? rebuilds every pair's derivations in every iteration, cached_derivs.h:60-101).  Here: when the lattices of
        // the corpus would take more than --disk-cache-bufsize of GPU memory they are NOT kept resident -- every iteration walks
        // the corpus in shards, each shard's lattices rebuilt on the GPU (0.15 s per million pairs), swept and dropped, the
        // shards' counts added up on the device (carmel_hip_accumulate_counts).  No file is created; same results.
        o.stream_lattices = true;
      } else if (k == "disk-cache-bufsize") {
        char* end = nullptr;
        double x = std::strtod(v.c_str(), &end);
        if (end && (*end == 'K' || *end == 'k')) x *= 1024.0;
        else if (end && (*end == 'M' || *end == 'm')) x *= 1024.0 * 1024.0;
        else if (end && (*end == 'G' || *end == 'g')) x *= 1024.0 * 1024.0 * 1024.0;
        if (!(x > 0)) throw UsageError("--disk-cache-bufsize needs a positive size (bytes; K, M, G suffixes)");
        o.resident_bytes = (uint64_t)x;
      } else if (k == "matrix-fb") {
        // carmel.cc:238, train.cc:254-266, 698-860: forward/backward over the dense (input position x output position x
        // state) matrix instead of derivation lattices (carmel_hip_set_matrix_fb, csrc/matrix_fb.hip)
        o.matrix_fb = true;
      } else if (k == "cache-no-prune")  // carmel.cc:241: keep states that cannot reach the goal in the cached lattices
        o.cache_no_prune = true;
      else if (k == "sample-prob-after")  // not a carmel option (its old builds logged this as "sample prob")
        o.sample_prob_after = true;
      else if (k == "crp-restarts")
        o.crp_restarts = std::atol(v.c_str());
      else if (k == "crp-argmax-final")
        o.crp_argmax_final = true;
      else if (k == "crp-argmax-sum")
        o.crp_argmax_sum = true;
      else if (k == "include-self")
        o.include_self = true;
      else if (k == "random-start")
        o.random_start = true;
      else if (k == "crp-exclude-prior")
        o.exclude_prior = true;
      else if (k == "crp-parallel")  // not a carmel option: the stale-count parallel sweep (gibbs.hip mode 1)
        o.crp_parallel = true;
      else if (k == "prior-inference-stddev")
        o.pi_stddev = std::atof(v.c_str());
      else if (k == "prior-inference-global")
        o.pi_global = true;
      else if (k == "prior-inference-restart-fresh")
        o.pi_restart_fresh = true;
      else if (k == "prior-inference-show")
        o.pi_show = true;
      else if (k == "prior-groupby")
        o.prior_groupby = v;
      else if (k == "number-from")
        o.number_from = std::atol(v.c_str());
      else if (k == "write-loaded") {
        o.write_loaded = v;
        o.have_write_loaded = true;
      }
      else if (k == "prior-inference-start" || k == "prior-inference-end" || k == "prior-inference-local")
        // gibbs_opts.hpp:85-89 documents them and forest-em reads them; carmel.cc:291-294 never does, so carmel runs as
        // if they were not given.  Same here (the library has them: carmel_hip_gibbs_set_prior_inference).
        std::cerr << "--" << k << " is not read by carmel (carmel.cc:291-294); ignored\n";
      else if (k == "digamma") {
        o.digamma = v;
        o.have_digamma = true;
      } else if (k == "help") {
        o.flags[(unsigned)'h'] = true;
      } else
        throw UsageError("option --" + k + " is not implemented by the GPU training front end");
      continue;
    }
    if (a.size() > 1 && a[0] == '-') {
      for (size_t j = 1; j < a.size(); ++j) {
        unsigned char c = (unsigned char)a[j];
        o.flags[c] = true;
        if (c == 'j') o.norm = CARMEL_HIP_NORM_JOINT;
        if (c == 'u') o.norm = CARMEL_HIP_NORM_NONE;
        if (c == 'M') o.max_iter = -1;
      }
      // a switch that takes a value consumes the next argument (carmel.cc:929-1000)
      auto value = [&]() -> const char* {
        if (i + 1 >= argc) throw std::runtime_error("missing value after " + a);
        return argv[++i];
      };
      for (size_t j = 1; j < a.size(); ++j) switch (a[j]) {
          case 'M':  // "-M n"; a bare -M means "report the corpus perplexity only" (train.cc:516-517)
            if (i + 1 < argc && (std::isdigit((unsigned char)argv[i + 1][0]) || argv[i + 1][0] == '-') &&
                std::strspn(argv[i + 1], "-0123456789") == std::strlen(argv[i + 1]))
              o.max_iter = std::atol(value());
            break;
          case 'e': o.converge = std::atof(value()); break;
          case 'X': o.converge_ppx_ratio = std::atof(value()); break;
          case 'f': o.smooth_floor = std::atof(value()); break;
          case 'T': o.index_threshold = std::atoi(value()); break;
          case 'F': o.out_file = value(); break;
          case 'R': o.seed = std::strtoull(value(), 0, 10); break;
          case '!':  // random restarts (carmel.cc:944-946)
            o.restarts = std::atol(value());
            break;
          case 'o':  // learning rate growth factor of over-relaxed EM (carmel.cc:940-943)
            o.rate_growth = std::max(1.0, std::atof(value()));
            break;
          case 'k': o.kpaths = std::atol(value()); break;
          case '+':  // pseudo-Dirichlet-process normalisation exp(digamma(alpha + w)) (carmel.cc:1009-1013)
            o.plus_alpha = std::atof(value());
            o.plus_alpha_set = true;
            break;
          case 'g': throw UsageError("switch -g n is not implemented under that name; use --generate-pairs=n");
          case 'G': throw UsageError("switch -G n is not implemented under that name; use --generate-paths=n");
          case 'L': throw UsageError("switch -L n is not implemented under that name; use --generate-max-arcs=n");
          case 'w': throw UsageError("switch -w w is not implemented under that name; use --prune-paths=w");
          case 'z': throw UsageError("switch -z n is not implemented under that name; use --prune-states=n");
          case 'p': throw UsageError("switch -p w is not implemented under that name; use --prune-arcs=w");
          default:
            // switches without a value that this front end implements; everything else carmel knows (k-best, generation,
            // projection, pruning, OpenFst, ...) is outside the training path
            // (O I Q W E @: WFST::path_print, fst.h:60-160 -- how --print-to writes the sampled paths; b s r i: batch decoding;
            // C: consolidating the composed machine's duplicate arcs)
            if (!std::strchr("tUujnlqdKmHJZDB2?:caShOIQWE@1bsriC", a[j]))
              throw UsageError(std::string("switch -") + a[j] + " is not implemented by the GPU training front end");
            break;
        }
      continue;
    }
    o.files.push_back(argv[i]);
  }
  if (o.crp) {  // force_cascade_derivs (carmel.cc:230-233)
    o.train_cascade = true;
    if (o.crp_iters > 1) o.max_iter = o.crp_iters;
  }
  if (o.train_cascade) o.flags[(unsigned)'t'] = true;
  return o;
}
