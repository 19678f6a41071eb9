// carmel_main.cpp — `carmel`-compatible command line for the training path, running on the GPU through the C-ABI
// (include/carmel_hip.h).  Accepts the training subset of carmel's switches (carmel.cc:929-1066):
//
//   carmel [-t] [--train-cascade] [-M n] [-e d] [-X r] [-f w] [-U] [-u | -j] [-? | -:] [-q] [-d] [-K] [-m] [-T n] [-a]
//          [-F out] [-H] [-J] [-Z] [-D] [-B] [-2] [-+ alpha] [--normby=JCN..] [--priors=a,b,..] [--digamma=a,,b] [--gpu=n]
//          corpus transducer [transducer ...]
//   carmel -S pairs transducer [transducer ...]      sum-of-paths probability of every pair (carmel.cc:1393-1410)
//
// A switch or option this front end does not implement is REFUSED (exit -12, like carmel's "No inputs supplied",
// carmel.cc:1137) rather than accepted and ignored: a drop-in that silently computes something else is worse than one
// that says no.
//
// With one transducer the trained transducer goes to stdout (or -F file); with --train-cascade every member is
// written to <file>.trained (cascade.h:23-32).  EM log lines on stderr have the reference's wording
// (train.cc:587-613, 639-657, 669-671).  Exit codes follow carmel.cc (-2 bad transducer, -9 unreadable file,
// -11 on an error caught at top level).
//
// run() is the list of stages; carmel_cli.hpp says which file holds which.
#include "carmel_cli.hpp"
#include "env_options.hpp"
using namespace carmel_host;

static int print_help() {
  std::cout << "carmel (MI355X training front end): -t / --train-cascade / --crp / -S over carmel's transducer and corpus "
               "files; switches: -t -M -e -X -f -U -u -j -n -o -! -1 -a -S -q -d -K -m -T -F -R -H -J -Z -D -B -2 -+ -? -: -c; "
               "options: --train-cascade --normby= --priors= --digamma= --random-set --disk-cache-derivations= --matrix-fb; "
               "the sampler: --crp[=N] --burnin= --crp-restarts= --print-every= --print-from= --print-to= --print-counts-from= "
               "--print-counts-to= --print-norms-from= --print-norms-to= --width= ... ; several GPUs: --gpus=N --exchange=; "
               "batch 1-best decoding: -b -i -s -r -k 1 with -I / -O / -@ (-Q -W -E); "
               "k-best decoding: --kbest=N (N <= 1024) in place of -k 1; "
               "posterior path samples: --sample-paths=N (N <= 65536) in place of -k 1, seeded by -R (not carmel's -G; no epsilon cycles); "
               "all-paths sums in the decoding report: --sum-paths with -b / -i (carmel's --sum; no epsilon cycles); "
               "arc posteriors: --posterior-counts=FILE with -b / -i writes the composed machine with every arc's expected count "
               "over all derivations of the lines as its weight (no epsilon cycles); "
               "pair decoding: --pair-lines=FILE with -b / -i and -k 1 (carmel's --post-b=FILE: line k of FILE is the other side of line k) "
               "prints every pair's best derivation, --sum-paths then multiplies the pairs' sums, --pair-alignments=OUT writes "
               "the best paths as in:out symbol pairs, --pair-counts=FILE writes the composed machine with every arc's expected "
               "count over all derivations of the pairs as its weight (no cycles of *e*:*e* arcs), --pair-samples=N (N <= 65536) "
               "prints N alignments of every pair drawn from the posterior over its derivations in place of the best one, seeded "
               "by -R, and --pair-alignments=OUT then gets one line per sample, --pair-kbest=N (N <= 1024) prints every pair's N best "
               "alignments best first in place of the best one (--kbest=N for the pairs), and --pair-alignments=OUT then gets N "
               "lines a pair; "
               "generation from the composed machine itself, seeded by -R: --generate-paths=N (carmel's -G N) prints N random paths, "
               "one line each, with -I / -O (-Q -W -E) or two lines each with -@; --generate-pairs=N (carmel's -g N) prints N random "
               "input/output pairs, two lines each; --generate-max-arcs=L (carmel's -L, default 1000) bounds a path's arcs and "
               "--generate-tries=T (default 256) the attempts a path may take; "
               "--best-paths=N (carmel's -k N without -b / -i, N <= 1024) prints the N best paths of the composed machine itself, best "
               "first, one line each: with -I / -O (-Q -W -E), two lines each with -@, or else arc by arc (src -> dst in : out / w); "
               "pruning the composed machine before it is printed (also with -c or -F): --prune-paths=W (carmel's -w W) keeps the states "
               "and arcs on a path at most W times worse than the best path, --prune-states=N (carmel's -z N) at most N states, those "
               "of the best paths through them, --prune-arcs=W (carmel's -p W) no arc of a weight below W; "
               "-C consolidates the composed machine first (before pruning, --best-paths=N or printing): arcs with the same source, "
               "destination, input and output become one arc of their summed weight, at most 1; --consolidate-max keeps the largest "
               "weight instead of the sum, --consolidate-unclamped lets a sum exceed 1; "
               "--machine-sums prints, in place of the composed machine (after -C and --prune-*), the number of its paths and the sum of "
               "their weights (carmel's --sum without -b / -i; no cycles among the states on a path; to the -F file if one is named, after "
               "-c's two lines with -c); --machine-counts=FILE also writes "
               "the machine with every arc's expected count over its own paths as its weight; "
               "the full list and what each replaces: INTEGRATION.md\n";
  return 0;
}

// batch decoding (-b / -i with -k 1): what is not implemented is refused here, before any device call; true: decoding
static bool validate_decoding(const Options& o, bool with_pairs) {
  const bool decoding =
      !o.have_best_paths && (o.flags[(unsigned)'b'] || o.flags[(unsigned)'i'] || o.kpaths != 0 || o.have_kbest || o.have_sample);
  if (o.have_posterior) {
    if (o.posterior_counts.empty()) throw UsageError("--posterior-counts=FILE needs a file name");
    if (!o.flags[(unsigned)'b'] && !o.flags[(unsigned)'i'])
      throw UsageError("--posterior-counts=FILE applies to batch decoding (-b or -i)");
    if (with_pairs) throw UsageError("--posterior-counts=FILE with -t / --train-cascade / -S is not implemented");
  }
  if (o.have_pair_counts) {
    if (o.pair_counts.empty()) throw UsageError("--pair-counts=FILE needs a file name");
    if (with_pairs || o.train_cascade) throw UsageError("--pair-counts=FILE with -t / --train-cascade / -S is not implemented");
    if (!o.have_pair_lines) throw UsageError("--pair-counts=FILE needs --pair-lines=FILE");
  }
  if (o.have_pair_samples) {
    if (with_pairs || o.train_cascade) throw UsageError("--pair-samples=N with -t / --train-cascade / -S is not implemented");
    if (!o.have_pair_lines) throw UsageError("--pair-samples=N needs --pair-lines=FILE");
    if (!o.flags[(unsigned)'b'] && !o.flags[(unsigned)'i']) throw UsageError("--pair-samples=N applies to batch decoding (-b or -i)");
    if (o.have_kbest) throw UsageError("--pair-samples=N and --kbest=N exclude each other");
    if (o.have_sample) throw UsageError("--pair-samples=N and --sample-paths=N exclude each other");
    if (o.pair_samples < 1 || o.pair_samples > 65536) throw UsageError("--pair-samples=N needs 1 <= N <= 65536");
    if (o.kpaths != 0 && o.kpaths != 1 && o.kpaths != o.pair_samples) throw UsageError("--pair-samples=N with -k m: m must be 1 or N");
  }
  if (o.have_pair_kbest) {
    if (with_pairs || o.train_cascade) throw UsageError("--pair-kbest=N with -t / --train-cascade / -S is not implemented");
    if (!o.have_pair_lines) throw UsageError("--pair-kbest=N needs --pair-lines=FILE");
    if (!o.flags[(unsigned)'b'] && !o.flags[(unsigned)'i']) throw UsageError("--pair-kbest=N applies to batch decoding (-b or -i)");
    if (o.have_kbest) throw UsageError("--pair-kbest=N and --kbest=N exclude each other (--pair-kbest=N is --kbest=N for the pairs of --pair-lines)");
    if (o.have_sample) throw UsageError("--pair-kbest=N and --sample-paths=N exclude each other");
    if (o.have_pair_samples) throw UsageError("--pair-kbest=N and --pair-samples=N exclude each other");
    if (o.pair_kbest < 1 || o.pair_kbest > 1024) throw UsageError("--pair-kbest=N needs 1 <= N <= 1024");
    if (o.kpaths != 0 && o.kpaths != 1 && o.kpaths != o.pair_kbest) throw UsageError("--pair-kbest=N with -k m: m must be 1 or N");
  }
  if (o.have_pair_alignments && !o.have_pair_lines) throw UsageError("--pair-alignments=OUT needs --pair-lines=FILE");
  if (o.have_pair_lines) {
    if (o.pair_lines.empty()) throw UsageError("--pair-lines=FILE needs a file name");
    if (o.have_pair_alignments && o.pair_alignments.empty()) throw UsageError("--pair-alignments=OUT needs a file name");
    if (!o.flags[(unsigned)'b'] && !o.flags[(unsigned)'i']) throw UsageError("--pair-lines=FILE applies to batch decoding (-b or -i with -k 1)");
    if (with_pairs) throw UsageError("--pair-lines=FILE with -t / --train-cascade / -S is not implemented");
    if (o.have_kbest || o.have_sample || o.have_posterior)
      throw UsageError("--pair-lines=FILE with --kbest=N, --sample-paths=N or --posterior-counts=FILE is not implemented (the pairs' "
                       "k best alignments: --pair-kbest=N, their arc posteriors: --pair-counts=FILE)");
  }
  if (decoding) {
    if (o.have_sample) {
      if (o.have_kbest) throw UsageError("--sample-paths=N and --kbest=N exclude each other");
      if (o.sample_paths < 1 || o.sample_paths > 65536) throw UsageError("--sample-paths=N needs 1 <= N <= 65536");
      if (o.kpaths != 0 && o.kpaths != 1 && o.kpaths != o.sample_paths) throw UsageError("--sample-paths=N with -k m: m must be 1 or N");
      if (!o.flags[(unsigned)'b'] && !o.flags[(unsigned)'i']) throw UsageError("--sample-paths=N applies to batch decoding (-b or -i)");
    } else if (o.have_kbest) {
      if (o.kbest < 1 || o.kbest > 1024) throw UsageError("--kbest=N needs 1 <= N <= 1024");
      if (o.kpaths != 0 && o.kpaths != 1 && o.kpaths != o.kbest) throw UsageError("--kbest=N with -k m: m must be 1 or N");
    } else if (!o.have_pair_samples && !o.have_pair_kbest) {  // (--pair-samples=N, --pair-kbest=N: -k is absent, 1 or N, checked above)
      if (o.kpaths > 1 && !o.flags[(unsigned)'b'] && !o.flags[(unsigned)'i'])
        throw UsageError("-k n without -b or -i (k-best paths of the whole cascade) is not implemented under that name; use --best-paths=n");
      if (o.kpaths > 1)
        throw UsageError("-k n with n > 1 (k-best paths) is not implemented; -k 1 with -b or -i is; use --kbest=n");
      if (o.kpaths < 1) throw UsageError("-b / -i without -k 1 (printing each line's composition) is not implemented");
    }
    if (!o.flags[(unsigned)'b'] && !o.flags[(unsigned)'i'])
      throw UsageError("-k without -b or -i (k-best paths of the whole cascade) is not implemented under that name; use --best-paths=n");
    if (with_pairs) throw UsageError("-k with -t / --train-cascade / -S is not implemented");
    if (!o.flags[(unsigned)'I'] && !o.flags[(unsigned)'O'] && !o.flags[(unsigned)'@'])
      throw UsageError("-k without -I, -O or -@ (the arc path form: state names of a per-line composition) is not implemented");
  } else if (o.flags[(unsigned)'s'] || o.flags[(unsigned)'r'])
    throw UsageError("-s / -r apply to batch decoding (-b or -i with -k 1)");
  else if (o.sum)
    throw UsageError("--sum-paths applies to batch decoding (-b or -i with -k 1, --kbest=N or --sample-paths=N)");
  return decoding;
}

// the N best paths of the composed machine (--best-paths=N: carmel's -k N without -b / -i): usage errors name the option, before
// any device call; true: listing them
static bool validate_best_paths(const Options& o) {
  if (!o.have_best_paths) return false;
  if (o.best_paths < 1 || o.best_paths > 1024) throw UsageError("--best-paths=N needs 1 <= N <= 1024");
  auto with = [&](bool on, const char* what) {
    if (on) throw UsageError(std::string("--best-paths=N with ") + what + " is not implemented: it lists the paths of the composed machine, without lines or a corpus");
  };
  with(o.flags[(unsigned)'b'], "-b");
  with(o.flags[(unsigned)'i'], "-i");
  with(o.flags[(unsigned)'s'], "-s");
  with(o.flags[(unsigned)'r'], "-r");
  with(o.crp, "--crp");  // (which sets --train-cascade, which sets -t)
  with(o.train_cascade, "--train-cascade");
  with(o.flags[(unsigned)'t'], "-t");
  with(o.flags[(unsigned)'S'], "-S");
  with(o.flags[(unsigned)'F'], "-F");
  with(o.have_pair_lines, "--pair-lines=FILE");
  with(o.have_kbest, "--kbest=N");
  with(o.have_sample, "--sample-paths=N");
  with(o.have_generate_paths, "--generate-paths=N");
  with(o.have_generate_pairs, "--generate-pairs=N");
  with(o.have_generate_max_arcs, "--generate-max-arcs=L");
  with(o.have_generate_tries, "--generate-tries=T");
  if (o.kpaths != 0 && o.kpaths != 1 && o.kpaths != o.best_paths) throw UsageError("--best-paths=N with -k m: m must be 1 or N");
  return true;
}

// pruning (--prune-paths=W / --prune-states=N / --prune-arcs=W: carmel's -w / -z / -p) applies to the compose-and-print path only:
// usage errors name the option, before any device call; true: pruning
static bool validate_pruning(const Options& o) {
  if (!o.have_prune_paths && !o.have_prune_states && !o.have_prune_arcs) return false;
  const char* sw = o.have_prune_paths ? "--prune-paths=W" : o.have_prune_states ? "--prune-states=N" : "--prune-arcs=W";
  auto with = [&](bool on, const char* what) {
    if (on) throw UsageError(std::string(sw) + " with " + what + " is not implemented: it prunes the composed machine that is printed, without lines or a corpus");
  };
  with(o.flags[(unsigned)'b'], "-b");
  with(o.flags[(unsigned)'i'], "-i");
  with(o.crp, "--crp");  // (which sets --train-cascade, which sets -t)
  with(o.train_cascade, "--train-cascade");
  with(o.flags[(unsigned)'t'], "-t");
  with(o.flags[(unsigned)'S'], "-S");
  with(o.have_best_paths, "--best-paths=N");
  with(o.have_generate_paths, "--generate-paths=N");
  with(o.have_generate_pairs, "--generate-pairs=N");
  with(o.kpaths != 0, "-k");
  return true;
}

// consolidation (-C with --consolidate-max / --consolidate-unclamped: carmel's own names) applies to the composed machine that is
// printed, pruned or listed: usage errors name the option, before any device call; true: consolidating
static bool validate_consolidation(const Options& o) {
  if (!o.flags[(unsigned)'C']) {
    if (o.consolidate_max) throw UsageError("--consolidate-max applies to -C");
    if (o.consolidate_unclamped) throw UsageError("--consolidate-unclamped applies to -C");
    return false;
  }
  auto with = [&](bool on, const char* what) {
    if (on) throw UsageError(std::string("-C with ") + what + " is not implemented: it consolidates the composed machine that is printed, pruned or listed, without lines or a corpus");
  };
  with(o.crp, "--crp");  // (which sets --train-cascade, which sets -t)
  with(o.train_cascade, "--train-cascade");
  with(o.flags[(unsigned)'t'], "-t");
  with(o.flags[(unsigned)'S'], "-S");
  with(o.flags[(unsigned)'b'], "-b");
  with(o.flags[(unsigned)'i'], "-i");
  with(o.have_generate_paths, "--generate-paths=N");
  with(o.have_generate_pairs, "--generate-pairs=N");
  return true;
}

// the sums over all paths of the composed machine (--machine-sums, --machine-counts=FILE): usage errors name the option, before any
// device call; true: summing
static bool validate_machine_sums(const Options& o) {
  if (!o.machine_sums) return false;
  const char* sw = o.have_machine_counts ? "--machine-counts=FILE" : "--machine-sums";
  if (o.have_machine_counts && o.machine_counts.empty()) throw UsageError("--machine-counts=FILE needs a file name");
  auto with = [&](bool on, const char* what) {
    if (on) throw UsageError(std::string(sw) + " with " + what + " is not implemented: it sums over the paths of the composed machine, without lines or a corpus");
  };
  with(o.flags[(unsigned)'b'], "-b");
  with(o.flags[(unsigned)'i'], "-i");
  with(o.flags[(unsigned)'s'], "-s");
  with(o.flags[(unsigned)'r'], "-r");
  with(o.crp, "--crp");  // (which sets --train-cascade, which sets -t)
  with(o.train_cascade, "--train-cascade");
  with(o.flags[(unsigned)'t'], "-t");
  with(o.flags[(unsigned)'S'], "-S");
  with(o.kpaths != 0, "-k");
  with(o.have_best_paths, "--best-paths=N");
  with(o.have_generate_paths, "--generate-paths=N");
  with(o.have_generate_pairs, "--generate-pairs=N");
  with(o.have_generate_max_arcs, "--generate-max-arcs=L");
  with(o.have_generate_tries, "--generate-tries=T");
  with(o.have_pair_lines, "--pair-lines=FILE");
  return true;
}

// generation (--generate-paths=N / --generate-pairs=N: carmel's -G / -g): usage errors name the switch, before any device call;
// true: generating
static bool validate_generation(const Options& o) {
  const bool generating = o.have_generate_paths || o.have_generate_pairs;
  if (!generating) {
    if (o.have_generate_max_arcs) throw UsageError("--generate-max-arcs=L applies to --generate-paths=N or --generate-pairs=N");
    if (o.have_generate_tries) throw UsageError("--generate-tries=T applies to --generate-paths=N or --generate-pairs=N");
    return false;
  }
  if (o.have_generate_paths && o.have_generate_pairs) throw UsageError("--generate-paths=N and --generate-pairs=N exclude each other");
  const char* sw = o.have_generate_paths ? "--generate-paths=N" : "--generate-pairs=N";
  const long n = o.have_generate_paths ? o.generate_paths : o.generate_pairs;
  if (n < 1 || (unsigned long long)n > (1ull << 32)) throw UsageError(std::string(sw) + " needs 1 <= N <= 2^32");
  if (o.generate_max_arcs < 1 || o.generate_max_arcs > (1l << 20))
    throw UsageError(std::string(sw) + ": --generate-max-arcs=L needs 1 <= L <= 2^20 (1048576)");
  if (o.generate_tries < 1 || o.generate_tries > 65536) throw UsageError(std::string(sw) + ": --generate-tries=T needs 1 <= T <= 65536");
  if ((unsigned long long)o.generate_max_arcs * (unsigned long long)o.generate_tries > (1ull << 24))
    throw UsageError(std::string(sw) + ": --generate-max-arcs=L times --generate-tries=T must be at most 2^24 (16777216)");
  auto with = [&](bool on, const char* what) {
    if (on) throw UsageError(std::string(sw) + " with " + what + " is not implemented: it generates from the composed machine, without lines or a corpus");
  };
  with(o.flags[(unsigned)'b'], "-b");
  with(o.flags[(unsigned)'i'], "-i");
  with(o.flags[(unsigned)'s'], "-s");
  with(o.kpaths != 0, "-k");
  with(o.have_kbest, "--kbest=N");
  with(o.have_sample, "--sample-paths=N");
  with(o.have_pair_lines, "--pair-lines=FILE");
  with(o.crp, "--crp");
  with(o.train_cascade, "--train-cascade");
  with(o.flags[(unsigned)'t'], "-t");
  with(o.flags[(unsigned)'S'], "-S");
  if (o.have_generate_paths && !o.flags[(unsigned)'I'] && !o.flags[(unsigned)'O'] && !o.flags[(unsigned)'@'])
    throw UsageError("--generate-paths=N without -I, -O or -@ (the arc path form) is not implemented");
  return true;
}

// the line stream: stdin with -s, else the first file (the last with -r) (carmel.cc:1099-1115, 1186-1191)
static std::string read_line_stream(Options& o) {
  if (o.flags[(unsigned)'s']) {
    std::stringstream ss;
    ss << std::cin.rdbuf();
    return ss.str();
  }
  if (o.files.size() < 2) throw UsageError("-b / -i without -s need a file of lines and a transducer");
  const size_t at = o.flags[(unsigned)'r'] ? o.files.size() - 1 : 0;
  std::string line_text = slurp(o.files[at]);
  o.files.erase(o.files.begin() + at);
  return line_text;
}

// weight output (carmel.cc:76-101): -Z always / -D never in log form; a weight in log form is e^x, `x ln` (-2) or
// `x log` base 10 (-B)
static int weight_style(const Options& o) {
  int wstyle = o.flags[(unsigned)'Z'] ? W_ALWAYS_LOG : W_SOMETIMES_LOG;
  if (o.flags[(unsigned)'D']) wstyle = W_NEVER_LOG;
  if (o.flags[(unsigned)'B'])
    wstyle |= W_BASE_LOG10;
  else if (o.flags[(unsigned)'2'])
    wstyle |= W_BASE_LN;
  return wstyle;
}

// plain `carmel a b ...`: print the (reduced) composition — no GPU involved; after pruning, to the -F file if one is named
static int print_composition(const Job& j, bool to_file = false) {
  const Options& o = j.o;
  std::ofstream of;
  if (to_file) {
    of.open(o.out_file.c_str());
    if (!of) {
      std::cerr << "Could not create file " << o.out_file << ".\n";
      return -8;
    }
  }
  std::ostream& os = to_file ? static_cast<std::ostream&>(of) : std::cout;
  if (o.flags[(unsigned)'c'])
    os << "Number of states in result: " << j.result->states.size() << "\nNumber of arcs in result: "
       << j.result->num_arcs() << "\n";
  else
    os << j.result->to_text(o.flags[(unsigned)'J'], o.flags[(unsigned)'H'], j.wstyle);
  return 0;
}

static int run(int argc, char** argv) {
  Job j;
  Options& o = j.o;
  o = parse_args(argc, argv);
  const bool training = o.flags[(unsigned)'t'];
  const bool scoring = !training && o.flags[(unsigned)'S'];  // carmel.cc:1134: -t overrides -S
  const bool with_pairs = training || scoring;
  if (o.flags[(unsigned)'h']) return print_help();
  const bool summing = validate_machine_sums(o);
  const bool consolidating = validate_consolidation(o);
  const bool pruning = validate_pruning(o);
  const bool listing = validate_best_paths(o);
  const bool generating = validate_generation(o);
  const bool decoding = validate_decoding(o, with_pairs);
  const std::string line_text = decoding ? read_line_stream(o) : std::string();
  if (o.files.empty() || (with_pairs && o.files.size() < 2)) {
    std::cerr << "usage: carmel -t [--train-cascade] [-M n] [-e d] [-X r] [-f w] [-U] [-u|-j] [-HJZD] [-F out] "
                 "corpus transducer [transducer ...]\n"
                 "       carmel [-HJZD] transducer [transducer ...]     (compose and print; host only)\n";
    return -12;
  }
  j.world = training ? ((o.crp && o.crp_restarts <= 0) ? 1 : o.gpus) : 1;
  if (!fork_ranks(j)) return -11;
  j.quiet = o.flags[(unsigned)'q'] || j.rank > 0;
  if (!with_pairs) o.files.insert(o.files.begin(), (const char*)0);  // no corpus argument
  j.nw = o.files.size() - 1;
  const std::string corpus_text = with_pairs ? slurp(o.files[0]) : std::string();
  j.wstyle = weight_style(o);
  if (int rc = load_members(j)) return rc;
  if (int rc = compose_members(j)) return rc;
  if (consolidating)  // (the reference's order: consolidate, reduce, prune -- carmel_main::minimize before prune, carmel.cc:638-642)
    if (int rc = consolidate_composition(o, *j.result, j.quiet, o.gpu)) return rc;
  if (decoding) return decode_batch(o, *j.result, line_text, j.wstyle, j.quiet, o.gpu);
  if (generating) return generate_batch(o, *j.result, j.wstyle, o.gpu);
  if (listing) return best_paths_batch(o, *j.result, j.wstyle, o.gpu);
  if (pruning) {
    if (int rc = prune_composition(o, *j.result, j.quiet, o.gpu)) return rc;
    if (!summing) return print_composition(j, !o.out_file.empty());
  }
  if (summing) return machine_sums_composition(o, *j.result, j.wstyle, o.gpu);
  if (!with_pairs) return print_composition(j, consolidating && !o.out_file.empty());
  read_corpus(j, corpus_text, /*weight_lines=*/!scoring);
  create_trainer(j);
  if (scoring) return score_pairs(j);
  begin_training(j);
  if (o.crp) return train_gibbs(j);
  train_em(j, o);
  if (j.rank > 0) return 0;  // the results are identical on every rank; rank 0 writes them
  write_fem_side_files(j);
  // output (carmel.cc:1435-1437, 1485-1496; cascade.h:23-32)
  if (!j.cascade) return write_single(j);
  std::vector<double> pw(j.params.logw.size());
  hip_check(carmel_hip_get_weights(j.t, pw.data()), "carmel_hip_get_weights");
  write_trained_members(j, pw.data());
  return 0;
}

int main(int argc, char** argv) {
  int rc;
  carmel_host::import_env_options();  // (CARMEL_HIP_<KEY> / CARMEL_TIMING: the library takes them as options, not from the environment)
  try {
    rc = run(argc, argv);
  } catch (UsageError& e) {
    std::cerr << "carmel: " << e.what() << "\n";
    rc = -12;
  } catch (std::exception& e) {
    report_error(e.what());
    rc = -11;
  }
  return wait_for_ranks(rc);
}
