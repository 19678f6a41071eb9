// carmel_load.cpp — from the files to a trainer: the input transducers and their normalisation methods (carmel.cc:488-499,
// 785-808), the composition chain (carmel.cc:1287-1355), the corpus, the GPU trainer; and carmel -S, which needs no more.
#include "carmel_cli.hpp"
using namespace carmel_host;

// ---- Job's members ----
std::vector<const Transducer*> Job::members() const {
  std::vector<const Transducer*> mem;
  if (cascade)
    for (size_t i = 0; i < nw; ++i) mem.push_back(&member[i]);
  else
    mem.push_back(result);
  return mem;
}
void Job::set_methods(const std::vector<double>& add) {
  if (cascade)
    hip_check(carmel_hip_set_cascade(t, params.logw.size(), params.logw.data(), params.group.data(),
                                     params.member.data(), params.src.data(), params.in.data(), (uint32_t)nw,
                                     norms.data(), add.data(), chains.chains.size(), coff.data(), cpar.data()),
              "carmel_hip_set_cascade");
  else
    hip_check(carmel_hip_set_norm(t, norms[0], add[0]), "carmel_hip_set_norm");
  if (any_digamma)
    hip_check(carmel_hip_set_digamma(t, (uint32_t)(cascade ? nw : 1), dig_alpha.data(), dig_on.data()), "carmel_hip_set_digamma");
}
void Job::set_corpus_range(size_t lo, size_t hi) {
  std::vector<uint64_t> io(1, 0), oo(1, 0);
  for (size_t p = lo; p < hi; ++p) {
    io.push_back(pairs.in_off[p + 1] - pairs.in_off[lo]);
    oo.push_back(pairs.out_off[p + 1] - pairs.out_off[lo]);
  }
  hip_check(carmel_hip_set_corpus(t, hi - lo, io.data(), pairs.in_sym.data() + pairs.in_off[lo], oo.data(),
                                  pairs.out_sym.data() + pairs.out_off[lo], pairs.weight.data() + lo),
            "carmel_hip_set_corpus");
}
void Job::set_whole_corpus() {
  hip_check(carmel_hip_set_corpus(t, pairs.size(), pairs.in_off.data(), pairs.in_sym.data(), pairs.out_off.data(),
                                  pairs.out_sym.data(), pairs.weight.data()),
            "carmel_hip_set_corpus");
}

std::string slurp(const char* fn) {
  std::ifstream f(fn, std::ios::binary);
  if (!f) throw std::runtime_error(std::string("File ") + fn + " could not be opened for input.");
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

// fem_in (carmel.cc:790-799): the members' weights, one after the other, from a file
static void load_fem_param(Job& j) {
  const Options& o = j.o;
  std::cerr << "Reading cascade weights from --load-fem-param=" << o.load_fem_param << std::endl;
  std::ifstream in(o.load_fem_param.c_str());
  if (!in) throw std::runtime_error("Missing --load-fem-param file.\n");
  for (size_t i = 0; i < j.nw; ++i) {
    std::vector<double> w;
    for (auto& st : j.member[i].states)
      for (size_t k = 0; k < st.size(); ++k) {
        std::string tok;
        double lw;
        if (!(in >> tok) || !parse_weight_token(tok, lw))
          throw std::runtime_error("--load-fem-param file doesn't have enough params; make sure it was --fem-param saved for "
                                   "the same cascade");
        w.push_back(lw);
      }
    j.member[i].set_weights(w.data());
  }
}

// normalisation methods per member (carmel.cc:488-499)
static void parse_methods(Job& j) {
  const Options& o = j.o;
  const size_t nw = j.nw;
  j.norms.assign(nw, o.norm);
  j.addc.assign(nw, o.pi_stddev != 0 ? 1.0 : 0.0);  // carmel.cc:491-492: inferred priors start from 1
  j.priorgroup.assign(nw, 1);
  for (size_t i = 0; i < o.prior_groupby.size() && i < nw; ++i) {  // fst.h:586-598
    const char ch = o.prior_groupby[i];
    if (ch < '0' || ch > '2')
      throw std::runtime_error("prior-groupby characters must be 0 (no scaling), 1 (same scaling for whole xdcr), or 2 "
                               "(separate scaling for each normgroup)");
    j.priorgroup[i] = ch - '0';
  }
  for (size_t i = 0; i < o.normby.size() && i < nw; ++i) {
    char ch = o.normby[i];
    j.norms[i] = (ch == 'J' || ch == 'j') ? CARMEL_HIP_NORM_JOINT
                 : (ch == 'N' || ch == 'n') ? CARMEL_HIP_NORM_NONE
                                            : CARMEL_HIP_NORM_CONDITIONAL;
  }
  {
    std::stringstream ss(o.priors);
    std::string tok;
    size_t i = 0;
    while (std::getline(ss, tok, ',') && i < nw) j.addc[i++] = std::atof(tok.c_str());
  }
  // --digamma=0,,0.5: one component per member, empty = the usual linear normalisation (carmel.cc:495); -+ a sets it for
  // the single method (carmel.cc:1009-1013)
  std::vector<double>& dig_alpha = j.dig_alpha;
  std::vector<uint8_t>& dig_on = j.dig_on;
  dig_alpha.assign(nw, 0.0);
  dig_on.assign(nw, 0);
  if (o.plus_alpha_set)
    for (size_t i = 0; i < nw; ++i) {
      dig_alpha[i] = o.plus_alpha;
      dig_on[i] = 1;
    }
  if (o.have_digamma) {
    size_t i = 0, p0 = 0;
    const std::string& d = o.digamma;
    while (i < nw) {  // split on ',' keeping empty fields
      size_t c = d.find(',', p0);
      std::string tok = d.substr(p0, c == std::string::npos ? std::string::npos : c - p0);
      if (!tok.empty()) {
        dig_alpha[i] = std::atof(tok.c_str());
        dig_on[i] = 1;
      }
      ++i;
      if (c == std::string::npos) break;
      p0 = c + 1;
    }
  }
  j.any_digamma = std::find(dig_on.begin(), dig_on.end(), (uint8_t)1) != dig_on.end();
}

// fem_in (carmel.cc:785-808).  --random-set (:786-789, cascade.h:398-401; -1 below is WFST::randomScale, fst.h:973-975, on the
// same draws): every unlocked arc of every member not normalised by NONE gets a new weight on (0..1] -- drawn from this
// build's counter-based generator, numbered member by member in arc order as the random restarts number them (the
// reference's Boost stream is not pinned by anything it holds); training starts by normalising (train.cc:509).
static void randomize_members(Job& j) {
  const Options& o = j.o;
  std::cerr << "Using random seed -R " << o.seed << std::endl;  // show_seed, carmel.cc:65-69
  uint32_t p = 0;
  for (size_t i = 0; i < j.nw; ++i)
    for (auto& st : j.member[i].states)
      for (auto& a : st) {
        if (a.group != kLocked && j.norms[i] != CARMEL_HIP_NORM_NONE) {
          const double lu = std::log(1.0 - carmel_hip_gibbs_uniform(o.seed, 0, p, 0));
          a.logw = o.random_set ? lu : a.logw + lu;
        }
        ++p;
      }
}

// the members as the files give them, then what the options do to them before anything is composed; != 0: an exit code
int load_members(Job& j) {
  const Options& o = j.o;
  const size_t nw = j.nw;
  std::vector<Transducer>& member = j.member;
  member.resize(nw);
  for (size_t i = 0; i < nw; ++i) {
    try {
      member[i].parse(slurp(o.files[i + 1]), !o.flags[(unsigned)'K']);  // carmel.cc:1197
    } catch (std::exception& e) {
      std::cerr << e.what() << "\nBad format of transducer file: " << o.files[i + 1] << "\n";
      return -2;
    }
    if (!o.flags[(unsigned)'m'] && nw > 1) member[i].drop_state_names();
  }
  if (!o.load_fem_param.empty()) load_fem_param(j);
  parse_methods(j);
  if (o.random_set || o.flags[(unsigned)'1']) randomize_members(j);
  // with --normby the INPUT transducers are normalised before anything is composed
  if (!o.normby.empty()) {
    std::cerr << "Normalizing input transducers by --normby=" << o.normby << std::endl;
    for (size_t i = 0; i < nw; ++i) member[i].normalize(j.norms[i], j.addc[i], j.dig_on[i] != 0, j.dig_alpha[i]);
  }
  if (!o.fem_early_param.empty()) {  // fem_out_param(fem_early_outparam), carmel.cc:801, 810-817
    std::cerr << "Writing cascade weights to --fem-param=" << o.fem_early_param << std::endl;
    std::ofstream of(o.fem_early_param.c_str());
    for (size_t i = 0; i < nw; ++i)
      for (auto& st : member[i].states)
        for (auto& a : st) of << format_weight(a.logw, W_SOMETIMES_LOG) << "\n";
  }
  if (o.number_from > 0) {
    std::cerr << "Assigning unique group ids to each arc in input cascade starting at " << o.number_from << ".\n";
    uint32_t label = (uint32_t)o.number_from;
    for (size_t i = 0; i < nw; ++i) label = member[i].number_arcs_from(label);
  }
  if (o.have_write_loaded) write_loaded(j);
  return 0;
}

// composition chain, left to right (carmel.cc:1287-1355); != 0: an exit code
int compose_members(Job& j) {
  const Options& o = j.o;
  const size_t nw = j.nw;
  std::vector<Transducer>& member = j.member;
  ParamTable& params = j.params;
  if (!o.flags[(unsigned)'d']) member[0].prune_useless();
  j.result = &member[0];
  j.cascade = o.train_cascade && nw > 1;
  if (nw > 1) {
    for (size_t i = 0; i < nw; ++i) params.add_member(member[i]);
    Composer comp(params, j.chains, (unsigned)o.index_threshold, /*trivial=*/!o.train_cascade);
    Operand A, B;
    for (size_t i = 1; i < nw; ++i) {
      A.bind(j.result, i > 1, params.member_base[0]);
      B.bind(&member[i], false, params.member_base[i]);
      std::unique_ptr<Transducer> next(new Transducer());
      double dev_s = 0;
      const bool ok = o.flags[(unsigned)'a'] ? comp.run_a(A, B, *next)  // carmel.cc:1318
                      : o.gpu_compose        ? comp.run_device(A, B, *next, o.gpu + (o.comm_plugin.empty() ? j.rank : 0), &dev_s)
                                             : comp.run(A, B, *next);
      if (o.gpu_compose && !o.flags[(unsigned)'a'] && timing_on())
        std::cerr << "timing: composition on the GPU " << dev_s << " s\n";
      if (!ok) {
        std::cerr << ")\nEmpty or invalid result of composition with transducer \"" << o.files[i + 1] << "\".\n";
        return -3;
      }
      size_t st = next->states.size(), ar = next->num_arcs();
      if (!o.flags[(unsigned)'d']) next->prune_useless();
      if (!j.quiet) {
        std::cerr << "\n\t(" << st << " states / " << ar << " arcs";
        if (next->states.size() != st || next->num_arcs() != ar)
          std::cerr << " reduce-> " << next->states.size() << "/" << next->num_arcs();
        std::cerr << ")";
      }
      j.composed = std::move(next);
      j.result = j.composed.get();
    }
    if (!j.quiet) std::cerr << std::endl;
  }
  return 0;
}

void read_corpus(Job& j, const std::string& corpus_text, bool weight_lines) {
  HostPairs& pairs = j.pairs;
  std::string warn;
  parse_corpus(*j.result, corpus_text, pairs, &warn, weight_lines);
  std::cerr << warn;
  if (pairs.size() == 0) {  // corpus.set_null() (carmel.cc:1421)
    pairs.weight.push_back(1.0);
    pairs.in_off.push_back(0);
    pairs.out_off.push_back(0);
  }
}

// the GPU trainer over the composition, the communicator of the --gpus ranks, and this rank's shard of the corpus
void create_trainer(Job& j) {
  const Options& o = j.o;
  Transducer* result = j.result;
  result->flatten(j.src, j.dst, j.in, j.out, j.logw, j.group);
  // (--comm-plugin: the caller's transport carries the sums; every rank runs on the device --gpu names -- single-GPU boxes, tests)
  const bool one_device = !o.comm_plugin.empty();
  const int my_device = o.gpu + (one_device ? 0 : j.rank);
  hip_check(carmel_hip_create(&j.t, my_device, (uint32_t)result->states.size(), result->final_state, j.logw.size(), j.src.data(),
                              j.dst.data(), j.in.data(), j.out.data(), j.logw.data(), j.group.data()),
            "carmel_hip_create");
  create_communicator(j, my_device);
  j.comm_made = true;
  if (j.world > 1 && !o.crp) shard_pairs(j);
  j.coff.assign(1, 0);
  if (j.cascade) {
    for (auto& c : j.chains.chains) {
      j.cpar.insert(j.cpar.end(), c.begin(), c.end());
      j.coff.push_back(j.cpar.size());
    }
    if (j.cpar.empty()) j.cpar.push_back(0);
  }
}

// carmel -S (carmel.cc:1393-1410): for every pair the sum over all its derivations with the weights as they stand
// (WFST::sumOfAllPaths, train.cc:925-945 = derivations::init_and_compute + prob): one forward sweep per pair on the GPU
int score_pairs(Job& j) {
  const HostPairs& pairs = j.pairs;
  carmel_hip_trainer* t = j.t;
  const int wstyle = j.wstyle;
  j.set_whole_corpus();
  std::vector<uint8_t> has(pairs.size(), 0);
  carmel_hip_lattice_stats ls;
  hip_check(carmel_hip_build_lattices(t, 1, 0, has.data(), &ls), "carmel_hip_build_lattices");
  std::vector<double> lp(pairs.size(), kNegInf);
  if (ls.n_pairs_kept) {
    carmel_hip_estimate_result er;
    hip_check(carmel_hip_estimate(t, &er, lp.data()), "carmel_hip_estimate");
  }
  double prod = 0;
  for (size_t p = 0; p < pairs.size(); ++p) {
    std::cout << format_weight(has[p] ? lp[p] : kNegInf, wstyle) << std::endl;
    prod += has[p] ? lp[p] : kNegInf;
  }
  std::cerr << "-S corpus product of probs=" << format_weight(prod, wstyle) << ", probability=" << base2(prod);
  if (pairs.size()) std::cerr << " per-line-perplexity(N=" << pairs.size() << ")=" << base2(ppxper(prod, (double)pairs.size()));
  std::cerr << std::endl;
  return 0;
}

// what EM and the sampler both start from: the methods, the normalised weights, the prior counts, the corpus
void begin_training(Job& j) {
  const Options& o = j.o;
  carmel_hip_trainer* t = j.t;
  const bool cascade = j.cascade;
  j.set_methods(j.addc);
  // arcs_table priors (derivations.h:96-101) are captured when forward_backward is constructed (train.cc:513): after
  // cascade.normalize (train.cc:509), which for a real cascade normalises the MEMBERS only -- the composed arcs still
  // carry their composition-time products until the first cascade.update() (train.cc:576).  So -U on a cascade takes its
  // prior counts from the weights as composed; a single transducer is its own cascade and gives its normalised weights.
  const bool want_prior = !o.crp && (!cascade || o.smooth_floor > 0 || o.flags[(unsigned)'U']);
  if (want_prior && cascade) hip_check(carmel_hip_set_prior(t, o.smooth_floor, o.flags[(unsigned)'U'] ? 1 : 0), "carmel_hip_set_prior");
  if (!o.crp) hip_check(carmel_hip_normalize(t), "carmel_hip_normalize");  // train.cc:509 (not for --crp, gibbs.cc:403)
  if (want_prior && !cascade) hip_check(carmel_hip_set_prior(t, o.smooth_floor, o.flags[(unsigned)'U'] ? 1 : 0), "carmel_hip_set_prior");
  j.set_whole_corpus();
  if (!o.fem_forest.empty()) write_fem_forest(j);
}
