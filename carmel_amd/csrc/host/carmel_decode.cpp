// carmel_decode.cpp — batch 1-best decoding: carmel -b -k 1 (carmel.cc:1266-1384, report_batch :355-376, print_kbest :378-398).
// The reference composes every line with the cascade and searches the result; here the cascade is composed ONCE and every
// line is decoded against it on the GPU (carmel_hip_decode, csrc/decode.hip), all lines in one call.  A path prints as
// WFST::path_print does (fst.h:60-160) in its -I / -O / -@ forms (-Q -W -E apply); the arc form needs the state names of a
// per-line composition, which is never built, and is refused before this is reached.
// --kbest=N prints, for every line, its N best derivations best first and then print_kbest's fill lines up to N
// (carmel_hip_decode_kbest, csrc/decode_kbest.hip); the summary multiplies each line's first path, as with -k 1.
// --sample-paths=N prints, for every line, N derivations drawn from the posterior over its derivations, in sample order
// (carmel_hip_decode_sample, csrc/decode_sample.hip, seeded by -R), in the same format and with the same fill lines; no best path
// is computed, so the report has no Viterbi line.  It is not carmel's -G, which generates from the whole machine: that is
// --generate-paths=N, at the end of this file.
// --sum-paths (carmel's --sum) adds every line's sum of all paths (post_compose's sum_acyclic_paths, carmel.cc:555-599; carmel_hip_decode_sum,
// csrc/decode_sum.hip) to the report on stderr; what goes to stdout does not change.
// --posterior-counts=FILE writes the composed machine to FILE as Transducer::to_text does (-H / -J apply), every arc's weight
// replaced by its expected number of uses over all derivations of the lines, every line weighing 1 (carmel_hip_decode_posterior,
// csrc/decode_posterior.hip: the E-step of carmel -t for these lines); every arc is written, one never used with weight 0.
// Nothing on stdout or stderr changes.
// --pair-lines=FILE (carmel's --post-b=FILE, carmel.cc:569-597): line k of FILE is the OTHER side's line of line k, and what is
// decoded is the pair -- its best derivation (carmel_hip_decode_pairs, csrc/decode_pairs.hip) in place of the line's, and with
// --sum-paths the sum of the pair's derivations (carmel_hip_decode_pairs_sum) in the "Sum (all paths)" line, the one-sided sums
// staying in the block before it.  Every pair prints exactly one line, its best path or the fill line: the reference prints
// nothing for a line that has a derivation alone but none as a pair (carmel.cc:588-591, 1367), which would leave stdout without a
// line-to-pair correspondence; this is a deliberate deviation.  --pair-alignments=OUT writes every pair's best path as
// space-separated in:out symbol names (*e* for epsilon), an empty line for a pair without a derivation: the -I / -O / -@ forms
// of a pair's path only spell the two lines again.  --pair-counts=FILE is --posterior-counts=FILE for the pairs: the composed
// machine, every arc's weight replaced by its expected number of uses over all derivations of the pairs, every pair weighing 1
// (carmel_hip_decode_pairs_posterior, csrc/decode_pairs_posterior.hip: the E-step of carmel -t for these pairs).
// --pair-samples=N is --sample-paths=N for the pairs: N derivations of every pair drawn from the posterior over the pair's
// derivations, in sample order (carmel_hip_decode_pairs_sample, csrc/decode_pairs_sample.hip, seeded by -R), printed in place
// of the best one with print_kbest's fill lines, N lines a pair; no Viterbi line is reported.  --pair-alignments=OUT then gets
// one line per sample, N lines a pair (N empty lines for a pair without a derivation): sample s of pair l is line l N + s.
// --pair-kbest=N is --kbest=N for the pairs (carmel's --post-b=FILE with -k n): every pair's N best derivations, best first
// (carmel_hip_decode_pairs_kbest, csrc/decode_pairs_kbest.hip), printed in place of the best one with print_kbest's fill lines, N
// lines a pair; the Viterbi line multiplies each pair's first path, as --kbest does, so N = 1 is plain --pair-lines -k 1 to the
// byte.  --pair-alignments=OUT then gets N lines a pair: rank r of pair l is line l N + r, a missing rank an empty line.
#include <cctype>
#include "carmel_cli.hpp"
using namespace carmel_host;

namespace {
struct Batch {  // the lines of one call and what the four steps below make of them
  const Options& o;
  Transducer& M;
  const int ws;
  std::vector<std::string> lines;
  // WFST::WFST(const char*) (wfstio.cc:152-172): the line's symbols; a symbol the machine never saw gets an id no arc carries
  std::vector<uint64_t> off = std::vector<uint64_t>(1, 0);
  std::vector<uint32_t> sym;
  double n_symbols = 0;  // carmel.cc:1277-1283: the sum of the lines' lengths
  // --pair-lines: the other side's line of every line, in the same form
  std::vector<uint64_t> off2 = std::vector<uint64_t>(1, 0);
  std::vector<uint32_t> sym2;
  // line l's paths are line_paths[l] .. line_paths[l + 1]; path p has the search's cost best[p] and the arcs
  // path[path_off[p] .. path_off[p + 1])
  std::vector<double> best;
  std::vector<uint64_t> path_off, line_paths;
  std::vector<uint32_t> path;
  std::vector<const HArc*> arc_of;
  std::vector<uint32_t> arc_src;  // the arc form of --best-paths=N: every arc's source state
  size_t n_0prob = 0;
  double n_prob = 0, prod_viterbi = 0;
  // --sum-paths (post_compose, carmel.cc:555-599): the lines whose sum of all paths is not zero, and the product of those sums
  // (with --pair-lines the block before the report keeps the one-sided sums, prod_pre; prod_sum multiplies the pairs' sums)
  double pre_n_prob = 0, prod_sum = 0, prod_pre = 0;

  int read_lines(const std::string& text, bool side_out);
  int read_pair_lines(const std::string& text, bool side_out);
  void pair_alignments() const;
  void decode(carmel_hip_decoder* d, size_t kbest);
  void sum_paths(carmel_hip_decoder* d);
  void posterior_counts(carmel_hip_decoder* d) const;
  void pair_counts(carmel_hip_decoder* d) const;
  void write_counts(std::vector<double>& count, const char* option, const std::string& file) const;
  void format_path(uint64_t p, std::string& buf, bool pair_form = false, bool arc_form = false) const;
  void print_paths(size_t kbest, bool quiet);
  void log_ppx(double n_pairs, double prod, size_t n_0) const;
  void report() const;
};

int Batch::read_lines(const std::string& text, bool side_out) {
  for (size_t p = 0; p < text.size();) {  // getline: an empty line is the empty string (Carmel 6.9, carmel.cc:1269-1270)
    size_t e = text.find('\n', p);
    if (e == std::string::npos) e = text.size();
    lines.push_back(text.substr(p, e - p));
    p = e + 1;
    if (!o.flags[(unsigned)'b']) break;  // -i without -b: one line (carmel.cc:1380)
  }
  for (size_t l = 0; l < lines.size(); ++l) {
    std::string& ln = lines[l];
    if (!ln.empty() && ln.back() == '\r') ln.pop_back();  // (getString drops a DOS CR)
    std::vector<uint32_t> ids;
    M.symbols_of_line(ln, side_out, ids);
    const SymbolTable& tab = side_out ? M.out_syms : M.in_syms;
    for (uint32_t id : ids)
      if (std::isdigit((unsigned char)tab.names[id][0])) {
        std::cerr << "Couldn't handle input line: " << ln << "\n";
        return -3;
      }
    sym.insert(sym.end(), ids.begin(), ids.end());
    off.push_back(sym.size());
    n_symbols += (double)ids.size();
  }
  return 0;
}

// --pair-lines: line k of the file, in the alphabet of the side the lines are not on (carmel.cc:569-582)
int Batch::read_pair_lines(const std::string& text, bool side_out) {
  size_t p = 0;
  for (size_t l = 0; l < lines.size(); ++l) {  // (lines beyond the last line are ignored)
    if (p >= text.size()) {
      std::cerr << "--pair-lines file didn't have as many lines as -b file.\n";
      return -3;
    }
    size_t e = text.find('\n', p);
    if (e == std::string::npos) e = text.size();
    std::string ln = text.substr(p, e - p);
    p = e + 1;
    if (!ln.empty() && ln.back() == '\r') ln.pop_back();
    std::vector<uint32_t> ids;
    M.symbols_of_line(ln, !side_out, ids);
    const SymbolTable& tab = side_out ? M.in_syms : M.out_syms;
    for (uint32_t id : ids)
      if (std::isdigit((unsigned char)tab.names[id][0])) {
        std::cerr << "For --pair-lines=" << o.pair_lines << ", couldn't handle input line: " << ln << "\n";
        return -3;
      }
    sym2.insert(sym2.end(), ids.begin(), ids.end());
    off2.push_back(sym2.size());
  }
  return 0;
}

void Batch::decode(carmel_hip_decoder* d, size_t kbest) {
  const size_t n = lines.size();
  line_paths.assign(n + 1, 0);
  const auto t0 = std::chrono::steady_clock::now();
  if (o.have_kbest || o.have_sample || o.have_pair_samples || o.have_pair_kbest) {
    if (o.have_pair_kbest)
      hip_check(carmel_hip_decode_pairs_kbest(d, (uint32_t)kbest, n, off.data(), sym.data(), off2.data(), sym2.data(),
                                              line_paths.data()),
                "carmel_hip_decode_pairs_kbest");
    else if (o.have_pair_samples)
      hip_check(carmel_hip_decode_pairs_sample(d, (uint32_t)kbest, o.seed, n, off.data(), sym.data(), off2.data(), sym2.data(),
                                               line_paths.data()),
                "carmel_hip_decode_pairs_sample");
    else if (o.have_sample)
      hip_check(carmel_hip_decode_sample(d, (uint32_t)kbest, o.seed, n, off.data(), sym.data(), line_paths.data()),
                "carmel_hip_decode_sample");
    else
      hip_check(carmel_hip_decode_kbest(d, (uint32_t)kbest, n, off.data(), sym.data(), line_paths.data()), "carmel_hip_decode_kbest");
    uint64_t n_paths = 0, n_path_arcs = 0;
    hip_check(carmel_hip_decoder_kbest_size(d, &n_paths, &n_path_arcs), "carmel_hip_decoder_kbest_size");
    best.resize(std::max<uint64_t>(n_paths, 1));
    path_off.resize(n_paths + 1);
    path.resize(std::max<uint64_t>(n_path_arcs, 1));
    hip_check(carmel_hip_decoder_get_kbest(d, best.data(), path_off.data(), path.data()), "carmel_hip_decoder_get_kbest");
  } else {
    std::vector<double> best1(n);
    std::vector<uint64_t> off1(n + 1);
    if (o.have_pair_lines)
      hip_check(carmel_hip_decode_pairs(d, n, off.data(), sym.data(), off2.data(), sym2.data(), best1.data(), off1.data()),
                "carmel_hip_decode_pairs");
    else
      hip_check(carmel_hip_decode(d, n, off.data(), sym.data(), best1.data(), off1.data()), "carmel_hip_decode");
    path.resize(std::max<uint64_t>(off1[n], 1));
    hip_check(carmel_hip_decoder_get_paths(d, path.data()), "carmel_hip_decoder_get_paths");
    path_off.assign(1, 0);
    for (size_t l = 0; l < n; ++l) {  // (a line without a derivation has no path)
      const bool has = best1[l] > kNegInf;
      if (has) {
        best.push_back(best1[l]);
        path_off.push_back(off1[l + 1]);
      }
      line_paths[l + 1] = line_paths[l] + (has ? 1 : 0);
    }
  }
  if (timing_on()) {
    double kms = 0;
    carmel_hip_decoder_last_ms(d, &kms);
    std::cerr << (o.have_pair_kbest     ? "timing: pairs kbest "
                  : o.have_pair_samples ? "timing: pairs sample "
                  : o.have_sample     ? "timing: sample "
                  : o.have_pair_lines ? "timing: pairs "
                                      : "timing: decode ")
              << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()
              << " s (kernels " << kms * 1e-3 << " s)\n";
  }
}

// every line's sum of all paths, multiplied in line order over the lines that have a derivation
void Batch::sum_paths(carmel_hip_decoder* d) {
  const size_t n = lines.size();
  std::vector<double> sums(n);
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = carmel_hip_decode_sum(d, n, off.data(), sym.data(), sums.data());
  if (o.have_pair_lines && rc == CARMEL_HIP_ERR_UNSUPPORTED) {  // an insertion loop *e*:y: an epsilon cycle for a line, none for a pair
    std::cerr << "The epsilon arcs of the lines' side have a cycle: no sum of all paths of the lines alone, before --pair-lines.\n";
    sums.assign(n, kNegInf);
  } else
    hip_check(rc, "carmel_hip_decode_sum");
  if (timing_on()) {
    double kms = 0;
    carmel_hip_decoder_last_ms(d, &kms);
    std::cerr << "timing: sum " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()
              << " s (kernels " << kms * 1e-3 << " s)\n";
  }
  for (size_t l = 0; l < n; ++l)
    if (sums[l] > kNegInf) {
      ++pre_n_prob;
      prod_pre += sums[l];
    }
  if (!o.have_pair_lines) {
    prod_sum = prod_pre;
    return;
  }
  const auto t1 = std::chrono::steady_clock::now();
  hip_check(carmel_hip_decode_pairs_sum(d, n, off.data(), sym.data(), off2.data(), sym2.data(), sums.data()),
            "carmel_hip_decode_pairs_sum");
  if (timing_on()) {
    double kms = 0;
    carmel_hip_decoder_last_ms(d, &kms);
    std::cerr << "timing: pairs sum " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count()
              << " s (kernels " << kms * 1e-3 << " s)\n";
  }
  for (size_t l = 0; l < n; ++l)  // carmel.cc:594-599: prod_sum *= the sum of the pair's composition
    if (sums[l] > kNegInf) prod_sum += sums[l];
}

// every pair's best path as in:out symbol names, one line a pair; with --pair-samples=N every sample, with --pair-kbest=N every
// rank, N lines a pair
void Batch::pair_alignments() const {
  const uint64_t per_pair = o.have_pair_samples ? (uint64_t)o.pair_samples : o.have_pair_kbest ? (uint64_t)o.pair_kbest : 1;
  std::string buf;
  for (size_t l = 0; l < lines.size(); ++l)
    for (uint64_t r = 0; r < per_pair; ++r) {  // (a pair without a derivation: empty lines)
      const uint64_t p = line_paths[l] + r;
      if (p < line_paths[l + 1])
        for (uint64_t k = path_off[p]; k < path_off[p + 1]; ++k) {
          const HArc& a = *arc_of[path[k]];
          if (k > path_off[p]) buf += ' ';
          buf += (a.in ? M.in_syms.names[a.in] : std::string("*e*")) + ":" + (a.out ? M.out_syms.names[a.out] : std::string("*e*"));
        }
      buf += '\n';
    }
  std::ofstream of(o.pair_alignments.c_str());
  of << buf;
  of.close();
  if (!of) throw std::runtime_error("--pair-alignments: cannot write " + o.pair_alignments);
}

// every arc's expected count over the derivations of all lines, as the weights of a copy of the machine, into the file
void Batch::posterior_counts(carmel_hip_decoder* d) const {
  std::vector<double> count(std::max<size_t>(M.num_arcs(), 1));
  const auto t0 = std::chrono::steady_clock::now();
  hip_check(carmel_hip_decode_posterior(d, lines.size(), off.data(), sym.data(), nullptr, nullptr, count.data()),
            "carmel_hip_decode_posterior");
  if (timing_on()) {
    double kms = 0;
    carmel_hip_decoder_last_ms(d, &kms);
    std::cerr << "timing: posterior " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()
              << " s (kernels " << kms * 1e-3 << " s)\n";
  }
  write_counts(count, "--posterior-counts", o.posterior_counts);
}

// the same over the derivations of all pairs
void Batch::pair_counts(carmel_hip_decoder* d) const {
  std::vector<double> count(std::max<size_t>(M.num_arcs(), 1));
  const auto t0 = std::chrono::steady_clock::now();
  hip_check(carmel_hip_decode_pairs_posterior(d, lines.size(), off.data(), sym.data(), off2.data(), sym2.data(), nullptr, nullptr,
                                              count.data()),
            "carmel_hip_decode_pairs_posterior");
  if (timing_on()) {
    double kms = 0;
    carmel_hip_decoder_last_ms(d, &kms);
    std::cerr << "timing: pairs posterior " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()
              << " s (kernels " << kms * 1e-3 << " s)\n";
  }
  write_counts(count, "--pair-counts", o.pair_counts);
}

// a copy of the machine with the counts as its weights, every arc written, into the file
void Batch::write_counts(std::vector<double>& count, const char* option, const std::string& file) const {
  for (double& c : count) c = c > 0 ? std::log(c) : kNegInf;
  Transducer counted(M);
  counted.set_weights(count.data());
  std::ofstream of(file.c_str());
  of << counted.to_text(o.flags[(unsigned)'J'], o.flags[(unsigned)'H'], ws, /*include_zero=*/true);
  of.close();
  if (!of) throw std::runtime_error(std::string(option) + ": cannot write " + file);
}

// one path of a line into buf, as path_print writes it; pair_form: the two lines of -@ whatever the switches say; arc_form:
// path_print's default (fst.h:60-160), (src -> dst in : out / w) per arc, which needs arc_src
void Batch::format_path(uint64_t p, std::string& buf, bool pair_form, bool arc_form) const {
  const bool fO = o.flags[(unsigned)'O'], fQ = o.flags[(unsigned)'Q'], fAT = o.flags[(unsigned)'@'] || pair_form, fW = o.flags[(unsigned)'W'],
             fE = o.flags[(unsigned)'E'];
  auto name = [&](bool output, uint32_t id) -> std::string {
    const std::string& x = output ? M.out_syms.names[id] : M.in_syms.names[id];
    return (!fQ || x.size() < 2 || x[0] != '"' || x[x.size() - 1] != '"') ? x : x.substr(1, x.size() - 2);  // outWithoutQuotes
  };
  bool first = true;
  auto sp = [&]() {
    if (!first) buf += ' ';
    first = false;
  };
  std::vector<uint32_t> outs;
  for (uint64_t k = path_off[p]; k < path_off[p + 1]; ++k) {
    const HArc& a = *arc_of[path[k]];
    if (fAT) {
      if (a.out != 0) outs.push_back(a.out);
      if (a.in != 0) {
        sp();
        buf += M.in_syms.names[a.in];
      }
    } else if (arc_form) {
      sp();
      buf += '(' + M.state_name(arc_src[path[k]]) + " -> " + M.state_name(a.dest) + ' ' + M.in_syms.names[a.in] + " : " +
             M.out_syms.names[a.out] + " / " + format_weight(a.logw, ws) + ")";
    } else {
      const uint32_t id = fO ? a.out : a.in;
      if (!(fE && id == 0)) {
        sp();
        buf += name(fO, id);
      }
    }
  }
  if (fAT) {
    buf += '\n';
    for (size_t j = 0; j < outs.size(); ++j) buf += (j ? " " : "") + M.out_syms.names[outs[j]];
  } else if (!fW) {  // path_print's own weight: the arcs multiplied in path order (fst.h path_print::arc)
    double lw_path = 0.0;
    for (uint64_t k = path_off[p]; k < path_off[p + 1]; ++k) lw_path += arc_of[path[k]]->logw;
    sp();
    buf += format_weight(lw_path, ws);
  }
  buf += '\n';
}

void Batch::print_paths(size_t kbest, bool quiet) {
  for (auto& st : M.states)
    for (auto& a : st) arc_of.push_back(&a);
  const bool fAT = o.flags[(unsigned)'@'], fW = o.flags[(unsigned)'W'];
  std::string buf;
  for (size_t l = 0; l < lines.size(); ++l) {
    if (!quiet) std::cerr << "Input line " << l + 1 << ": " << lines[l] << "\n";
    buf.clear();
    const uint64_t p0 = line_paths[l], p1 = line_paths[l + 1];
    if (p0 == p1)
      ++n_0prob;
    else {
      ++n_prob;
      prod_viterbi += best[p0];  // non0_viterbi_prob: prod_viterbi *= best_w (the search's cost, carmel_hip_decode), in line order
    }
    for (uint64_t p = p0; p < p1; ++p) format_path(p, buf);
    for (uint64_t f = p1 - p0; f < kbest; ++f) {  // print_kbest's fill lines
      if (!(fW || fAT)) buf += '0';
      buf += '\n';
    }
    std::cout << buf;
  }
  std::cout << std::flush;
}

// log_ppx (carmel.cc:306-318) with Weight::print_ppx (weight.h:321-329)
void Batch::log_ppx(double n_pairs, double prod, size_t n_0) const {
  std::cerr << "product of probs=" << format_weight(prod, ws) << ", probability=" << base2(prod);
  if (n_symbols) std::cerr << " per-input-symbol-perplexity(N=" << n_symbols << ")=" << base2(ppxper(prod, n_symbols));
  if (n_pairs) std::cerr << " per-line-perplexity(N=" << n_pairs << ")=" << base2(ppxper(prod, n_pairs));
  if (n_0) std::cerr << ", excluding " << n_0 << " 0 probabilities (i.e. real ppx is infinite).";
  std::cerr << std::endl;
}

// report_batch (carmel.cc:354-377)
void Batch::report() const {
  const size_t n = lines.size();
  if (o.sum && pre_n_prob) {  // the lines post_compose saw: those with a derivation (the name passed is " inputs", carmel.cc:361)
    std::cerr << "Derivations found for all " << pre_n_prob << "  inputs.\n";
    log_ppx(pre_n_prob, prod_pre, 0);
  }
  if (n_0prob)
    std::cerr << "No derivations found for " << n_0prob << " of " << n << " inputs.\n";
  else
    std::cerr << "Derivations found for all " << n << " inputs.\n";
  if (!o.have_sample && !o.have_pair_samples) {  // (sampling computes no best path)
    std::cerr << "Viterbi (best path) ";
    log_ppx(n_prob, prod_viterbi, n_0prob);
  }
  if (o.sum) {
    std::cerr << "Sum (all paths) ";
    log_ppx(n_prob, prod_sum, n_0prob);
  }
}
}  // namespace

int decode_batch(const Options& o, Transducer& M, const std::string& text, int ws, bool quiet, int device) {
  const bool side_out = o.flags[(unsigned)'r'];
  Batch b{o, M, ws};
  if (int rc = b.read_lines(text, side_out)) return rc;
  if (b.lines.empty()) {
    std::cerr << "No lines of input provided.\n";
    return 0;
  }
  if (o.have_pair_lines)
    if (int rc = b.read_pair_lines(slurp(o.pair_lines.c_str()), side_out)) return rc;
  std::vector<uint32_t> src, dst, in, out, group;
  std::vector<double> logw;
  M.flatten(src, dst, in, out, logw, group);
  carmel_hip_decoder* d = 0;
  hip_check(carmel_hip_decoder_create(&d, device, (uint32_t)M.states.size(), M.final_state, logw.size(), src.data(), dst.data(),
                                      in.data(), out.data(), logw.data(), side_out ? 1 : 0),
            "carmel_hip_decoder_create");
  struct Guard {
    carmel_hip_decoder* d;
    ~Guard() { carmel_hip_decoder_destroy(d); }
  } guard{d};
  const size_t kbest = o.have_pair_kbest     ? (size_t)o.pair_kbest
                       : o.have_pair_samples ? (size_t)o.pair_samples
                       : o.have_sample     ? (size_t)o.sample_paths
                       : o.have_kbest      ? (size_t)o.kbest
                                           : 1;  // output lines per input line
  b.decode(d, kbest);
  if (o.sum) b.sum_paths(d);
  if (o.have_posterior) b.posterior_counts(d);
  if (o.have_pair_counts) b.pair_counts(d);
  b.print_paths(kbest, quiet);
  if (o.have_pair_alignments) b.pair_alignments();
  b.report();
  return 0;
}

// --generate-paths=N (carmel's -G N, carmel.cc:1446-1458) and --generate-pairs=N (carmel's -g N, carmel.cc:1459-1482): N random
// walks through the composed machine (carmel_hip_decoder_generate, csrc/decode_generate.hip, seeded by -R; --generate-max-arcs=L
// and --generate-tries=T are its limits).  There is no line stream.  A path prints as a decoded one does, one line in the -I / -O
// forms (-Q -W -E apply) or, with -@, as the pair it spells (print_training_pair, fst.h:941); a pair prints as printSeq does
// (carmel.cc:118-124): a line of input symbols and a line of output symbols, epsilons dropped.
int generate_batch(const Options& o, Transducer& M, int ws, int device) {
  Batch b{o, M, ws};
  std::vector<uint32_t> src, dst, in, out, group;
  std::vector<double> logw;
  M.flatten(src, dst, in, out, logw, group);
  carmel_hip_decoder* d = 0;
  hip_check(carmel_hip_decoder_create(&d, device, (uint32_t)M.states.size(), M.final_state, logw.size(), src.data(), dst.data(),
                                      in.data(), out.data(), logw.data(), 0),
            "carmel_hip_decoder_create");
  struct Guard {
    carmel_hip_decoder* d;
    ~Guard() { carmel_hip_decoder_destroy(d); }
  } guard{d};
  const bool pairs = o.have_generate_pairs;
  const uint64_t n = (uint64_t)(pairs ? o.generate_pairs : o.generate_paths);
  const auto t0 = std::chrono::steady_clock::now();
  hip_check(carmel_hip_decoder_generate(d, pairs ? CARMEL_HIP_GENERATE_CONDITIONAL : CARMEL_HIP_GENERATE_JOINT, n, 0, o.seed,
                                        (uint32_t)o.generate_max_arcs, (uint32_t)o.generate_tries, nullptr),
            "carmel_hip_decoder_generate");
  uint64_t n_paths = 0, n_path_arcs = 0;
  hip_check(carmel_hip_decoder_kbest_size(d, &n_paths, &n_path_arcs), "carmel_hip_decoder_kbest_size");
  b.best.resize(std::max<uint64_t>(n_paths, 1));
  b.path_off.resize(n_paths + 1);
  b.path.resize(std::max<uint64_t>(n_path_arcs, 1));
  hip_check(carmel_hip_decoder_get_kbest(d, b.best.data(), b.path_off.data(), b.path.data()), "carmel_hip_decoder_get_kbest");
  if (timing_on()) {
    double kms = 0;
    carmel_hip_decoder_last_ms(d, &kms);
    std::cerr << "timing: generate " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " s (kernels "
              << kms * 1e-3 << " s)\n";
  }
  for (auto& st : M.states)
    for (auto& a : st) b.arc_of.push_back(&a);
  std::string buf;
  for (uint64_t p = 0; p < n_paths; ++p) {
    b.format_path(p, buf, pairs);
    if (buf.size() >= (1u << 20)) {
      std::cout << buf;
      buf.clear();
    }
  }
  std::cout << buf << std::flush;
  return 0;
}

// --best-paths=N (carmel's -k N without -b / -i: print_kbest(kPaths, result), carmel.cc:1380-1381, 379-397): the N best paths of
// the composed machine itself (carmel_hip_decoder_best_paths, csrc/decode_best_paths.hip), best first, then print_kbest's fill
// lines.  There is no line stream, and no transducer is written (carmel.cc:1485).  A path prints in the -I / -O forms (-Q -W -E
// apply), as the pair it spells with -@, or else in path_print's arc form.
int best_paths_batch(const Options& o, Transducer& M, int ws, int device) {
  Batch b{o, M, ws};
  std::vector<uint32_t> src, dst, in, out, group;
  std::vector<double> logw;
  M.flatten(src, dst, in, out, logw, group);
  carmel_hip_decoder* d = 0;
  hip_check(carmel_hip_decoder_create(&d, device, (uint32_t)M.states.size(), M.final_state, logw.size(), src.data(), dst.data(),
                                      in.data(), out.data(), logw.data(), 0),
            "carmel_hip_decoder_create");
  struct Guard {
    carmel_hip_decoder* d;
    ~Guard() { carmel_hip_decoder_destroy(d); }
  } guard{d};
  const auto t0 = std::chrono::steady_clock::now();
  uint64_t n_paths = 0, n_path_arcs = 0;
  hip_check(carmel_hip_decoder_best_paths(d, (uint32_t)o.best_paths, &n_paths), "carmel_hip_decoder_best_paths");
  hip_check(carmel_hip_decoder_kbest_size(d, &n_paths, &n_path_arcs), "carmel_hip_decoder_kbest_size");
  b.best.resize(std::max<uint64_t>(n_paths, 1));
  b.path_off.resize(n_paths + 1);
  b.path.resize(std::max<uint64_t>(n_path_arcs, 1));
  hip_check(carmel_hip_decoder_get_kbest(d, b.best.data(), b.path_off.data(), b.path.data()), "carmel_hip_decoder_get_kbest");
  if (timing_on()) {
    double kms = 0;
    uint32_t rounds = 0;
    uint64_t selected = 0;
    carmel_hip_decoder_last_ms(d, &kms);
    carmel_hip_decoder_best_paths_stats(d, &rounds, &selected);
    std::cerr << "timing: best paths " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " s (kernels "
              << kms * 1e-3 << " s, " << rounds << " rounds, " << selected << " states selected)\n";
  }
  for (auto& st : M.states)
    for (auto& a : st) b.arc_of.push_back(&a);
  b.arc_src = src;
  const bool fAT = o.flags[(unsigned)'@'], fW = o.flags[(unsigned)'W'];
  const bool arc_form = !o.flags[(unsigned)'I'] && !o.flags[(unsigned)'O'] && !fAT;
  std::string buf;
  for (uint64_t p = 0; p < n_paths; ++p) b.format_path(p, buf, false, arc_form);
  for (uint64_t f = n_paths; f < (uint64_t)o.best_paths; ++f) {  // print_kbest's fill lines
    if (!(fW || fAT)) buf += '0';
    buf += '\n';
  }
  std::cout << buf << std::flush;
  return 0;
}

// --prune-paths=W / --prune-states=N / --prune-arcs=W (carmel's -w / -z / -p: carmel_main::prune in shrink, carmel.cc:633-636,
// 674-677): the composed and reduced machine is flattened, carmel_hip_decoder_prune (csrc/decode_prune.hip) marks what stays, and
// Transducer::keep applies the masks.  A state cap can leave dead ends: unless -d is given the machine is reduced once more (the
// reference leaves them in place).  Without -q the shrink_monitor note ` prune-> states/arcs` goes to stderr if anything went.
int prune_composition(const Options& o, Transducer& M, bool quiet, int device) {
  if (M.states.empty()) return 0;  // (nothing to prune)
  std::vector<uint32_t> src, dst, in, out, group;
  std::vector<double> logw;
  M.flatten(src, dst, in, out, logw, group);
  carmel_hip_decoder* d = 0;
  hip_check(carmel_hip_decoder_create(&d, device, (uint32_t)M.states.size(), M.final_state, logw.size(), src.data(), dst.data(),
                                      in.data(), out.data(), logw.data(), 0),
            "carmel_hip_decoder_create");
  struct Guard {
    carmel_hip_decoder* d;
    ~Guard() { carmel_hip_decoder_destroy(d); }
  } guard{d};
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> state_keep(M.states.size()), arc_keep(std::max<size_t>(logw.size(), 1));
  const uint32_t cap = o.have_prune_states ? (uint32_t)std::min<long>(o.prune_states, 0xffffffffl) : 0xffffffffu;
  uint64_t n_states = 0, n_arcs = 0;
  hip_check(carmel_hip_decoder_prune(d, o.prune_log_ratio, cap, o.prune_min_arc_logw, state_keep.data(), arc_keep.data(), &n_states,
                                     &n_arcs),
            "carmel_hip_decoder_prune");
  if (timing_on()) {
    double kms = 0;
    uint32_t fr = 0, br = 0;
    carmel_hip_decoder_last_ms(d, &kms);
    carmel_hip_decoder_prune_stats(d, &fr, &br);
    std::cerr << "timing: prune " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " s (kernels "
              << kms * 1e-3 << " s, " << fr << " F rounds, " << br << " R rounds)\n";
  }
  const size_t st = M.states.size(), ar = M.num_arcs();
  M.keep(state_keep, arc_keep);
  if (!o.flags[(unsigned)'d']) M.prune_useless();
  if (!quiet && (M.states.size() != st || M.num_arcs() != ar))
    std::cerr << "\t(" << st << " states / " << ar << " arcs prune-> " << M.states.size() << "/" << M.num_arcs() << ")" << std::endl;
  return 0;
}

// -C with --consolidate-max / --consolidate-unclamped (carmel_main::minimize, carmel.cc:638-642: consolidate, then reduce, before
// any pruning): the composed machine is flattened, carmel_hip_consolidate (csrc/consolidate.hip) names every segment's first arc
// and its weight, and Transducer::consolidate keeps those.  A segment of arcs of weight zero disappears, which can leave a dead
// end: unless -d is given the machine is reduced once more.  Only the final result of a chain of transducers is consolidated.
// Without -q the shrink_monitor note ` consolidate-> states/arcs` goes to stderr if anything went.
int consolidate_composition(const Options& o, Transducer& M, bool quiet, int device) {
  if (M.states.empty()) return 0;  // (nothing to consolidate)
  std::vector<uint32_t> src, dst, in, out, group;
  std::vector<double> logw;
  M.flatten(src, dst, in, out, logw, group);
  const auto t0 = std::chrono::steady_clock::now();
  const size_t n = logw.size();
  std::vector<uint32_t> arc_map(std::max<size_t>(n, 1)), kept_id(std::max<size_t>(n, 1));
  std::vector<double> kept_logw(std::max<size_t>(n, 1));
  uint64_t n_kept = 0;
  double kms = 0;
  hip_check(carmel_hip_consolidate(device, n, src.data(), dst.data(), in.data(), out.data(), logw.data(), o.consolidate_max ? 1 : 0,
                                   o.consolidate_unclamped ? 0 : 1, arc_map.data(), kept_id.data(), kept_logw.data(), &n_kept, &kms),
            "carmel_hip_consolidate");
  if (timing_on())
    std::cerr << "timing: consolidate " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " s (kernels "
              << kms * 1e-3 << " s)\n";
  const size_t st = M.states.size(), ar = M.num_arcs();
  kept_id.resize(n_kept);
  kept_logw.resize(n_kept);
  M.consolidate(kept_id, kept_logw);
  if (!o.flags[(unsigned)'d']) M.prune_useless();
  if (!quiet && (M.states.size() != st || M.num_arcs() != ar))
    std::cerr << "\t(" << st << " states / " << ar << " arcs consolidate-> " << M.states.size() << "/" << M.num_arcs() << ")" << std::endl;
  return 0;
}

// --machine-sums / --machine-counts=FILE (carmel's --sum without -b / -i: sum_acyclic_paths on the result, carmel.cc:555-599, and the
// third line of -c, carmel.cc:841-855): the composed machine, consolidated and pruned if that was asked for, is flattened and
// carmel_hip_decoder_machine_sums (csrc/decode_machine_sums.hip) sums over all its paths.  Two lines go to stdout, or to the -F
// file, in place of the transducer; with -c they follow -c's own two lines.  --machine-counts=FILE writes the machine as --posterior-counts does (-H / -J apply, every arc written), every arc's
// weight replaced by its expected number of uses on a path drawn with probability weight / sum; an arc on no path gets 0.  A cycle
// among the states on a path is the library's error (exit -11).
int machine_sums_composition(const Options& o, Transducer& M, int ws, int device) {
  double total = kNegInf, n_paths = 0;
  std::vector<double> post(std::max<size_t>(M.num_arcs(), 1), kNegInf);
  if (!M.states.empty()) {  // (an empty machine has no path)
    std::vector<uint32_t> src, dst, in, out, group;
    std::vector<double> logw;
    M.flatten(src, dst, in, out, logw, group);
    carmel_hip_decoder* d = 0;
    hip_check(carmel_hip_decoder_create(&d, device, (uint32_t)M.states.size(), M.final_state, logw.size(), src.data(), dst.data(),
                                        in.data(), out.data(), logw.data(), 0),
              "carmel_hip_decoder_create");
    struct Guard {
      carmel_hip_decoder* d;
      ~Guard() { carmel_hip_decoder_destroy(d); }
    } guard{d};
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t n_useful = 0;
    hip_check(carmel_hip_decoder_machine_sums(d, &total, &n_paths, &n_useful), "carmel_hip_decoder_machine_sums");
    if (o.have_machine_counts) hip_check(carmel_hip_decoder_machine_sums_arcs(d, post.data()), "carmel_hip_decoder_machine_sums_arcs");
    if (timing_on()) {
      double kms = 0;
      uint32_t fl = 0, bl = 0;
      carmel_hip_decoder_last_ms(d, &kms);
      carmel_hip_decoder_machine_sums_stats(d, &fl, &bl);
      std::cerr << "timing: machine sums " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() << " s (kernels "
                << kms * 1e-3 << " s, " << n_useful << " useful states, " << fl << " forward levels, " << bl << " backward levels)\n";
    }
  }
  char count[64];
  if (n_paths < 9007199254740992.0)  // (exact below 2^53)
    std::snprintf(count, sizeof count, "%llu", (unsigned long long)n_paths);
  else
    std::snprintf(count, sizeof count, "%.17g", n_paths);
  std::ofstream of;
  if (!o.out_file.empty()) {  // -F names where the result goes, as for the transducer these lines stand in for
    of.open(o.out_file.c_str());
    if (!of) {
      std::cerr << "Could not create file " << o.out_file << ".\n";
      return -8;
    }
  }
  std::ostream& os = o.out_file.empty() ? static_cast<std::ostream&>(std::cout) : of;
  if (o.flags[(unsigned)'c'])  // -c's two lines come first, unchanged
    os << "Number of states in result: " << M.states.size() << "\nNumber of arcs in result: " << M.num_arcs() << "\n";
  os << "Number of paths in result: " << count << "\nSum of all paths in result: " << format_weight(total, ws) << "\n" << std::flush;
  if (o.have_machine_counts) {
    Transducer counted(M);
    counted.set_weights(post.data());
    std::ofstream of(o.machine_counts.c_str());
    of << counted.to_text(o.flags[(unsigned)'J'], o.flags[(unsigned)'H'], ws, /*include_zero=*/true);
    of.close();
    if (!of) throw std::runtime_error("--machine-counts: cannot write " + o.machine_counts);
  }
  return 0;
}
