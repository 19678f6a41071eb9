// carmel_gibbs.cpp — --crp: WFST::train_gibbs (gibbs.cc:386-430) over the trainer of a Job.  The sampler runs in the library
// (carmel_hip_gibbs_*); here are its options, the first sample's weights, the tables and paths it prints, the merge of the
// --gpus ranks' runs, the log and the .trained files.
#include "carmel_cli.hpp"
using namespace carmel_host;

namespace {
carmel_hip_gibbs_opts pack_gibbs_opts(const Job& j) {
  const Options& o = j.o;
  carmel_hip_gibbs_opts go;
  std::memset(&go, 0, sizeof go);
  go.iter = (uint32_t)(o.max_iter > 0 ? o.max_iter : 0);
  go.burnin = (uint32_t)o.burnin;
  go.seed = o.seed;
  go.mode = o.crp_parallel ? 1 : 0;
  go.expectation = o.expectation;
  go.restarts = (uint32_t)std::max(0L, o.crp_restarts);
  go.argmax_final = o.crp_argmax_final;
  go.argmax_sum = o.crp_argmax_sum;
  go.include_self = o.include_self;
  go.random_start = o.random_start;
  go.uniform_p0 = o.uniform_p0;
  go.dirichlet_p0 = o.dirichlet_p0;
  go.final_counts = o.final_counts;
  go.exclude_prior = o.exclude_prior;
  go.min_prior = 1e-2;
  go.high_temp = o.high_temp;
  go.low_temp = o.low_temp;
  for (size_t i = 0; i < j.nw; ++i)
    if (j.addc[i] <= 0)
      std::cerr << "Gibbs sampling requires positive --priors for base model / initial sample.  Setting to 0.01\n";
  return go;
}

// the arc weights the first sample is drawn from (empty: the cache model's own)
std::vector<double> initial_weights(Job& j) {
  const Options& o = j.o;
  carmel_hip_trainer* t = j.t;
  std::vector<double> init_arc_logw;
  if (o.init_em > 0) {
    // gibbs.cc:400-423: EM without priors gives the weights the first sample is drawn from; the base distribution
    // stays the given one unless --em-p0
    std::vector<double> p0(j.n_params());
    hip_check(carmel_hip_get_weights(t, p0.data()), "carmel_hip_get_weights");
    std::vector<double> zero(j.nw, 0.0);
    j.set_methods(zero);
    hip_check(carmel_hip_normalize(t), "carmel_hip_normalize");
    hip_check(carmel_hip_set_prior(t, 0.0, 0), "carmel_hip_set_prior");
    Options em = o;
    em.max_iter = o.init_em;
    em.converge = 0;
    em.converge_ppx_ratio = 1;
    em.restarts = 0;
    em.rate_growth = 1;
    train_em(j, em);
    init_arc_logw.resize(j.logw.size());
    hip_check(carmel_hip_get_arc_weights(t, init_arc_logw.data()), "carmel_hip_get_arc_weights");
    std::vector<double> em_w(p0.size());
    hip_check(carmel_hip_get_weights(t, em_w.data()), "carmel_hip_get_weights");
    j.set_methods(j.addc);
    hip_check(carmel_hip_set_weights(t, o.em_p0 ? em_w.data() : p0.data()), "carmel_hip_set_weights");
  }
  if (o.init_from_p0 && o.init_em <= 0) {
    // gibbs.cc:405-421: the first sample comes from the composed transducer's own weights instead of the cache.  For a
    // real cascade those are the products made at composition time (cascade.normalize normalises the members, nothing
    // updates the composed arcs); a single transducer is its own cascade: its weights normalised without priors.
    init_arc_logw = j.logw;
    if (!j.cascade) {
      std::vector<double> p0(j.logw.size());
      hip_check(carmel_hip_get_weights(t, p0.data()), "carmel_hip_get_weights");
      std::vector<double> zero(j.nw, 0.0);
      j.set_methods(zero);
      hip_check(carmel_hip_normalize(t), "carmel_hip_normalize");
      hip_check(carmel_hip_get_arc_weights(t, init_arc_logw.data()), "carmel_hip_get_arc_weights");
      j.set_methods(j.addc);
      hip_check(carmel_hip_set_weights(t, p0.data()), "carmel_hip_set_weights");
    }
  }
  return init_arc_logw;
}

// --print-counts-from/-to, --print-norms-from/-to (gibbs.hpp:970-1078; carmel's order gibbs.cc:42-64): the tables are keyed by
// the ids define_param hands out (gibbs.cc:113-190): member by member, norm group by norm group in NormGroupIter's order (the
// order --fem-norm lists them in: refhash.hpp), a group's locked arcs first as they come, then its free arcs -- a CONDITIONAL
// group's in reversed list order --; a member normalised by NONE gets ids only.  Norm ids run on across the members, JOINT
// states without arcs included; the prior-scale group of a norm group as metanorm assigns it (gibbs.hpp:404-470).
struct GibbsTables {
  const Job& job;
  const Options& o;
  const size_t n_par;
  const bool want_counts, want_norms;
  const std::vector<const Transducer*> tmem;
  std::vector<uint32_t> ref_id, ref_meta;
  std::vector<int64_t> ref_norm;
  std::vector<std::vector<uint32_t> > norm_members;  // by reference norm id: the trainer's parameter ids
  // the trainer's parameter id -> (member, source state, arc)
  std::vector<uint32_t> p_src, p_mem;
  std::vector<const HArc*> p_arc;

  explicit GibbsTables(const Job& j);
  void number_member(size_t i, size_t base, uint32_t& gid, uint32_t& nexti);
  void print_param(size_t pp) const;
  void print_groupby(size_t pp) const;
  void print_norms(uint32_t iter, double time, const std::vector<double>& x) const;
  void print_counts(bool final, const char* name, uint32_t iter, double time, const std::vector<double>& x,
                    const std::vector<double>& sacc, const std::vector<double>& tm, const std::vector<double>& prior,
                    const std::vector<double>& prob, const std::vector<double>& touch) const;
  void print_paths(const std::vector<std::vector<uint32_t> >& smp, const std::vector<double>& plw, long a, long b) const;
};

GibbsTables::GibbsTables(const Job& j)
    : job(j), o(j.o), n_par(j.n_params()), want_counts(o.print_counts_to > o.print_counts_from),
      want_norms(o.print_norms_to > o.print_norms_from), tmem(j.members()), ref_id(n_par, 0), ref_norm(n_par, -1) {
  for (size_t i = 0; i < tmem.size(); ++i)
    for (uint32_t st = 0; st < tmem[i]->states.size(); ++st)
      for (auto& arc : tmem[i]->states[st]) {
        p_src.push_back(st);
        p_arc.push_back(&arc);
        p_mem.push_back((uint32_t)i);
      }
  if (want_counts || want_norms) {
    uint32_t gid = 0, nexti = 1;
    size_t p0 = 0;
    for (size_t i = 0; i < tmem.size(); ++i) {
      number_member(i, p0, gid, nexti);
      p0 += tmem[i]->num_arcs();
    }
    if (o.pi_global) std::fill(ref_meta.begin(), ref_meta.end(), 1u);  // finish_params: set_global (gibbs.hpp:572-579)
  }
}

// the reference's ids of member i's parameters (the trainer's: base ..) and of its norm groups
void GibbsTables::number_member(size_t i, size_t base, uint32_t& gid, uint32_t& nexti) {
  const Transducer& m = *tmem[i];
  const std::vector<int>& norms = job.norms;
  const int pg = job.priorgroup[i < job.priorgroup.size() ? i : 0];
  if (norms[i] == CARMEL_HIP_NORM_NONE) {
    size_t p0 = base;
    for (auto& st : m.states)
      for (size_t k = 0; k < st.size(); ++k) ref_id[p0++] = gid++;
    return;
  }
  for_each_norm_group(m, norms[i], [&](size_t first, const std::vector<size_t>& g) {
    const size_t p0 = base + first;
    std::vector<size_t> free_arcs;
    for (size_t k : g)
      if (p_arc[p0 + k]->group == kLocked)
        ref_id[p0 + k] = gid++;
      else
        free_arcs.push_back(k);
    if (norms[i] == CARMEL_HIP_NORM_CONDITIONAL) std::reverse(free_arcs.begin(), free_arcs.end());
    const uint32_t nid = (uint32_t)norm_members.size();
    norm_members.emplace_back();
    for (size_t k : free_arcs) {
      ref_id[p0 + k] = gid++;
      ref_norm[p0 + k] = nid;
      norm_members.back().push_back((uint32_t)(p0 + k));
    }
    ref_meta.push_back(pg == 0 ? 0u : nexti);  // gibbs.cc:132-137
    if (pg == 2) ++nexti;
  });
  if (pg == 1) ++nexti;  // gibbs.cc:184
}

// print_norms (gibbs.hpp:970-981): the norm sums of groups [from, to) -- a group's sum is the sum of its members' counts
void GibbsTables::print_norms(uint32_t iter, double time, const std::vector<double>& x) const {
  if (!want_norms) return;
  const unsigned long from = o.print_norms_from, to = std::min<unsigned long>(o.print_norms_to, norm_members.size());
  if (!(to > from)) return;
  std::cout << "\n# group\tnormalization group sums i=" << iter << " t=" << time << "\n(\n";
  for (unsigned long n = from; n < to; ++n) {
    double sum = 0;
    for (uint32_t pp : norm_members[n]) sum += x[pp];
    std::cout << ' ' << sum << "\n";
  }
  std::cout << ")\n";
}

// carmel_gibbs::print_param (gibbs.cc:206-212): member index, then WFST::printArc without the weight
void GibbsTables::print_param(size_t pp) const {
  const size_t mi = p_mem[pp];
  const Transducer& W = *tmem[mi];
  const HArc& arc = *p_arc[pp];
  std::cout << '\t' << mi << '(' << W.state_name(p_src[pp]) << " -> " << W.state_name(arc.dest) << ' ' << W.in_syms.names[arc.in]
            << " : " << W.out_syms.names[arc.out] << ')';
}

void GibbsTables::print_groupby(size_t pp) const {  // the prior-scale group of the parameter's norm group
  const uint32_t meta = ref_norm[pp] >= 0 ? ref_meta[(size_t)ref_norm[pp]] : 0u;
  std::cout << '\t';
  if (meta > 0)
    std::cout << meta;
  else
    std::cout << "FIXED";
}

// print_counts (gibbs.hpp:986-1064): x, s, tm = gibbs_param::sumcount; final: x holds the finalized counts, prob the weights
void GibbsTables::print_counts(bool final, const char* name, uint32_t iter, double time, const std::vector<double>& x,
                               const std::vector<double>& sacc, const std::vector<double>& tm, const std::vector<double>& prior,
                               const std::vector<double>& prob, const std::vector<double>& touch) const {
  if (!want_counts) return;
  const double ta = time + 1;
  std::cout << "\n#id\tgroup\tcount\tprob";
  if (!final) std::cout << "\tavg@" << ta << "\tlast@t\tprior\tgroupby";
  if (o.rich_counts) std::cout << "\tparam name";
  if (!final) std::cout << "\titer=" << iter;
  std::cout << "\t" << name << '\n';
  const unsigned long from = o.print_counts_from, to = std::min<unsigned long>(o.print_counts_to, n_par);
  auto field = [&](double d) {
    std::cout << '\t';
    print_width(std::cout, d, (int)o.width);
  };
  auto row = [&](size_t pp) {
    const uint32_t gi = ref_id[pp];
    if (!(gi >= from && gi < to)) return;
    // (a parameter without a norm group -- a locked arc, a member normalised by NONE -- never counts: its sumcount stays 0)
    const bool has = ref_norm[pp] >= 0;
    const double xx = has ? x[pp] : 0.0, sx_ = has ? sacc[pp] : 0.0, tx = has ? tm[pp] : 0.0;
    const double avg = final ? xx / ta : (ta > 0 ? (sx_ + xx * (ta - tx)) / ta : xx);  // delta_sum::avg(ta)
    if (!(o.print_counts_sparse == 0 || avg >= prior[pp] + o.print_counts_sparse)) return;
    std::cout << gi << '\t';
    if (ref_norm[pp] >= 0)
      std::cout << ref_norm[pp];
    else
      std::cout << "LOCKED";
    field(final ? avg : xx);
    field(prob[pp]);
    if (!final) {
      field(avg);
      field(has ? touch[pp] : 0.0);  // delta_sum::tmax as the reference keeps it: the last sweep that changed the count
      field(prior[pp]);
      print_groupby(pp);
    }
    if (o.rich_counts) print_param(pp);
    std::cout << '\n';
  };
  if (o.norm_order) {  // ids in order (gibbs.hpp:1050-1055)
    std::vector<uint32_t> by_id(n_par);
    for (size_t pp = 0; pp < n_par; ++pp) by_id[ref_id[pp]] = (uint32_t)pp;
    for (unsigned long gi = from; gi < to; ++gi) row(by_id[gi]);
  } else  // "print counts in fst file order, not normgroups order" (gibbs.cc:58-64)
    for (size_t pp = 0; pp < n_par; ++pp) row(pp);
  std::cout << "\n";
}

// gibbs_base::print_all -> carmel_gibbs::print_sample (gibbs.hpp:1066-1078; gibbs.cc:258-296): per block, for every input
// transducer in [a, b) the arcs of the sampled path that belong to it, through WFST::path_print; an arc's weight is
// proposal_prob of its parameter at the time of printing (plw: ln of it, per parameter)
void GibbsTables::print_paths(const std::vector<std::vector<uint32_t> >& smp, const std::vector<double>& plw, long a, long b) const {
  const int ws = job.wstyle;
  const bool fO = o.flags[(unsigned)'O'], fI = o.flags[(unsigned)'I'], fQ = o.flags[(unsigned)'Q'], fAT = o.flags[(unsigned)'@'],
             fW = o.flags[(unsigned)'W'], fE = o.flags[(unsigned)'E'];
  auto unquote = [](const std::string& x) {
    return (x.size() >= 2 && x[0] == '"' && x[x.size() - 1] == '"') ? x.substr(1, x.size() - 2) : x;
  };
  for (auto& blk : smp)
    for (long i = a; i < b; ++i) {
      const Transducer& W = *tmem[(size_t)i];
      bool first = true;
      double lw_path = 0.0;
      std::vector<uint32_t> outs;
      auto sp = [&]() {
        if (!first) std::cout << ' ';
        first = false;
      };
      for (uint32_t pid : blk) {
        if (pid >= p_mem.size() || p_mem[pid] != (uint32_t)i) continue;
        const HArc& arc = *p_arc[pid];
        lw_path += plw[pid];
        if (fAT) {
          if (arc.out != 0) outs.push_back(arc.out);
          if (arc.in != 0) {
            sp();
            std::cout << W.in_syms.names[arc.in];
          }
        } else if (fO || fI) {
          const uint32_t id = fO ? arc.out : arc.in;
          if (!(fE && id == 0)) {
            sp();
            const std::string& nm = fO ? W.out_syms.names[id] : W.in_syms.names[id];
            std::cout << (fQ ? unquote(nm) : nm);
          }
        } else {
          sp();
          std::cout << '(' << W.state_name(p_src[pid]) << " -> " << W.state_name(arc.dest) << ' ' << W.in_syms.names[arc.in] << " : "
                    << W.out_syms.names[arc.out] << " / " << format_weight(plw[pid], ws) << ")";
        }
      }
      if (fAT) {
        std::cout << std::endl;
        bool f2 = true;
        for (uint32_t id : outs) {
          if (!f2) std::cout << ' ';
          f2 = false;
          std::cout << W.out_syms.names[id];
        }
        std::cout << std::endl;
      } else {
        if (!fW) {
          sp();
          std::cout << format_weight(lw_path, ws);
        }
        std::cout << std::endl;
      }
    }
}

// every block's sample of the sampler's current state (parameter ids along the path, chain order)
std::vector<std::vector<uint32_t> > fetch_samples(carmel_hip_gibbs* gs, uint32_t nbk) {
  std::vector<uint32_t> buf(std::max<uint32_t>(1, carmel_hip_gibbs_max_sample(gs)));
  std::vector<std::vector<uint32_t> > smp(nbk);
  for (uint32_t bk = 0; bk < nbk; ++bk) {
    uint32_t n = 0;
    hip_check(carmel_hip_gibbs_get_sample(gs, bk, buf.data(), &n), "carmel_hip_gibbs_get_sample");
    smp[bk].assign(buf.begin(), buf.begin() + n);
  }
  return smp;
}

// [a, b) of --print-from / --print-to clipped to the input transducers; false: nothing of it is in range
bool print_range(const Job& j, long& a, long& b) {
  const size_t n_members = j.cascade ? j.nw : 1;
  a = j.o.print_from, b = j.o.print_to;
  if (!(b > a && a < (long)n_members)) return false;
  if (b > (long)n_members) b = (long)n_members;
  return true;
}

// --print-every=N (gibbs_opts.hpp:78-79; gibbs.hpp:959-968 maybe_print_periodic): after sweeps 0, N, 2N, ... a comment line
// and, with --print-to, every block's sampled path -- the arcs carry the proposal probabilities of that moment
// (gibbs.cc:272-286); the count / norm tables of --print-counts-* / --print-norms-* follow it.
// With --gpus the runs are spread over the ranks (replicas): every rank keeps what its runs print, run by run, and rank 0
// prints all of it in run order afterwards -- what one process running the runs one after the other prints.
struct PeriodicObserver {
  const Job& job;
  const GibbsTables& tab;
  const carmel_hip_gibbs_opts& go;
  carmel_hip_gibbs* gs;
  std::vector<std::string> text;  // --gpus: by run, what the run printed
  // the tables' state: counts as they stand, their time-weighted sums and stamps, the priors, the proposal probabilities
  std::vector<double> sx, ss, st_, sp, spr, stouch;

  void read_state();
  void print_prior_counts() const;
  void operator()(uint32_t run, uint32_t iter, double time);
  static void call(void* ctx, uint32_t run, uint32_t iter, double time) { (*(PeriodicObserver*)ctx)(run, iter, time); }
};
struct Redirect {  // std::cout into a stream while this lives (print_paths writes to std::cout)
  std::streambuf* old;
  bool on;
  Redirect(std::ostream& to, bool on_) : old(std::cout.rdbuf()), on(on_) {
    if (on) std::cout.rdbuf(to.rdbuf());
  }
  ~Redirect() {
    if (on) std::cout.rdbuf(old);
  }
};
struct Keep {  // what was captured, appended to its run's text at the end
  std::ostringstream& c;
  std::string* dst;
  ~Keep() {
    if (dst) *dst += c.str();
  }
};
struct TablesAtExit {  // print_all (gibbs.hpp:1066-1078): the sample, then the norm sums, then the counts
  const PeriodicObserver& ob;
  uint32_t iter;
  double time;
  ~TablesAtExit() {
    ob.tab.print_norms(iter, time, ob.sx);
    ob.tab.print_counts(false, "", iter, time, ob.sx, ob.ss, ob.st_, ob.sp, ob.spr, ob.stouch);
  }
};

void PeriodicObserver::read_state() {
  const size_t n_par = tab.n_par;
  for (std::vector<double>* v : {&sx, &ss, &st_, &sp, &spr, &stouch}) v->assign(n_par, 0.0);
  hip_check(carmel_hip_gibbs_get_state(gs, sx.data(), ss.data(), st_.data(), sp.data(), stouch.data()), "carmel_hip_gibbs_get_state");
  hip_check(carmel_hip_gibbs_current_probs(gs, spr.data()), "carmel_hip_gibbs_current_probs");
  for (size_t pp = 0; pp < n_par; ++pp)  // final_prob (gibbs.hpp:144-151): 0 for a count of 0
    if (tab.ref_norm[pp] >= 0 && !(sx[pp] > 0)) spr[pp] = 0;
}
void PeriodicObserver::print_prior_counts() const {  // gibbs_base::run's prologue (gibbs.hpp:811-814): the priors as counts
  std::vector<double> pprob(tab.n_par);
  for (size_t pp = 0; pp < tab.n_par; ++pp) {
    double ns = 0;
    if (tab.ref_norm[pp] >= 0)
      for (uint32_t q : tab.norm_members[(size_t)tab.ref_norm[pp]]) ns += sp[q];
    pprob[pp] = tab.ref_norm[pp] >= 0 ? (sp[pp] > 0 ? sp[pp] / ns : 0.0) : sp[pp];
  }
  tab.print_counts(true, "(prior counts)", 0, 0.0, sp, ss, st_, sp, pprob, stouch);
}
void PeriodicObserver::operator()(uint32_t run, uint32_t iter, double time) {
  const Options& o = job.o;
  const int world = job.world;
  std::ostringstream cap;
  Redirect redirect(cap, world > 1);
  Keep keep{cap, (world > 1 && run < text.size()) ? &text[run] : nullptr};
  if (tab.want_counts || tab.want_norms) read_state();
  if (iter == 0 && o.print_counts_sparse == 0) {
    std::cout << "# ";
    if (tab.want_counts) print_prior_counts();
  }
  std::cout << "# Gibbs i=" << iter << " ";
  if (go.high_temp != go.low_temp && (go.high_temp > 0 || go.low_temp > 0)) {  // gibbs.hpp:945-955 itername
    const double pw_ = carmel_hip_gibbs_power(go.high_temp, go.low_temp, go.iter, iter);
    std::cout << "temperature=" << 1.0 / pw_ << " power=" << pw_ << " ";
  }
  std::cout << "t=" << time << "\n";
  TablesAtExit tables{*this, iter, time};
  if (!(o.print_to > o.print_from)) return;
  if (go.expectation) throw std::runtime_error("can't print sample when using expectation because there is no single sample.\n");
  long a, b;
  if (!print_range(job, a, b)) return;
  const std::vector<std::vector<uint32_t> > smp = fetch_samples(gs, carmel_hip_gibbs_n_blocks(gs));
  std::vector<double> pr(job.n_params());
  hip_check(carmel_hip_gibbs_current_probs(gs, pr.data()), "carmel_hip_gibbs_current_probs");
  for (double& x : pr) x = x > 0 ? std::log(x) : -std::numeric_limits<double>::infinity();
  tab.print_paths(smp, pr, a, b);
}

struct GibbsRun {  // what the runs of this rank leave behind once the sampler is gone
  uint32_t n_runs = 0, per_run = 0, nblocks = 0, best_run = 0;
  std::vector<double> lp, lp_after;  // the log: per run and sweep
  double my_stats[3] = {0, 0, 0};
  int my_ran = 0;
  std::vector<double> ptrace, pcum;  // --prior-inference-*
  carmel_hip_lattice_stats gls;
  std::vector<std::vector<uint32_t> > final_sample;  // --print-to: the kept run's sample, block by block
  std::vector<double> final_x;  // the kept run's counts as finalize_cumulative_counts left them: the final table's
};

carmel_hip_gibbs* create_sampler(Job& j, const carmel_hip_gibbs_opts& go, const std::vector<double>& init_arc_logw, GibbsRun& r) {
  const Options& o = j.o;
  carmel_hip_gibbs* gs = 0;
  hip_check(carmel_hip_gibbs_create(&gs, j.t, &go), "carmel_hip_gibbs_create");
  std::memset(&r.gls, 0, sizeof r.gls);
  if (carmel_hip_gibbs_lattice_stats(gs, &r.gls) == CARMEL_HIP_OK) log_lattice_stats(r.gls, j.pairs.size());
  if (!init_arc_logw.empty())
    hip_check(carmel_hip_gibbs_set_init_weights(gs, init_arc_logw.data()), "carmel_hip_gibbs_set_init_weights");
  r.n_runs = go.restarts + 1, r.per_run = go.iter + 1;
  std::vector<uint32_t> member_states(j.nw, (uint32_t)j.result->states.size());
  if (j.cascade)
    for (size_t i = 0; i < j.nw; ++i) member_states[i] = (uint32_t)j.member[i].states.size();
  if (o.pi_stddev > 0)
    hip_check(carmel_hip_gibbs_set_prior_inference(gs, o.pi_stddev, o.pi_global, 0, o.pi_restart_fresh, 0, 0, j.priorgroup.data(),
                                                   member_states.data(), (uint32_t)j.nw),
              "carmel_hip_gibbs_set_prior_inference");
  r.lp.assign((size_t)r.per_run * r.n_runs, 0.0);
  r.lp_after.assign(o.sample_prob_after ? r.lp.size() : 0, 0.0);
  return gs;
}

// the runs, and everything that is read from the sampler before it is destroyed
void run_sampler(Job& j, const carmel_hip_gibbs_opts& go, carmel_hip_gibbs* gs, const GibbsTables& tab, GibbsRun& r) {
  const Options& o = j.o;
  const auto t_g0 = std::chrono::steady_clock::now();
  int rc = carmel_hip_gibbs_run_ex(gs, r.lp.data(), 0, o.sample_prob_after ? r.lp_after.data() : 0);
  r.nblocks = carmel_hip_gibbs_n_blocks(gs);
  if (timing_on() && rc == CARMEL_HIP_OK) {  // (bench.py --config crp)
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_g0).count();
    std::vector<uint32_t> buf(std::max<uint32_t>(1, carmel_hip_gibbs_max_sample(gs)));
    uint64_t sampled = 0;
    if (!go.expectation)
      for (uint32_t b = 0; b < r.nblocks; ++b) {  // (not fetch_samples: here a block that cannot be read counts as nothing)
        uint32_t n = 0;
        if (carmel_hip_gibbs_get_sample(gs, b, buf.data(), &n) == CARMEL_HIP_OK) sampled += n;
      }
    std::cerr << "timing: gibbs mode=" << (go.mode ? "parallel" : "exact") << " sweeps=" << (uint64_t)r.per_run * r.n_runs << " blocks=" << r.nblocks
              << " lattice_states=" << r.gls.kept_states << " lattice_arcs=" << r.gls.kept_arcs << " sampled_params=" << sampled
              << " seconds=" << sec << std::endl;
  }
  r.best_run = carmel_hip_gibbs_best_run(gs);
  if (rc == CARMEL_HIP_OK) hip_check(carmel_hip_gibbs_best_stats(gs, r.my_stats, &r.my_ran), "carmel_hip_gibbs_best_stats");
  r.ptrace.assign((size_t)r.per_run * r.n_runs * 6, 0.0);
  r.pcum.assign(carmel_hip_gibbs_n_prior_scales(gs), 1.0);
  if (o.pi_stddev > 0 && rc == CARMEL_HIP_OK)
    hip_check(carmel_hip_gibbs_prior_trace(gs, r.ptrace.data(), r.per_run * r.n_runs, r.pcum.data(), (uint32_t)r.pcum.size()),
              "carmel_hip_gibbs_prior_trace");
  if (o.print_to > o.print_from && rc == CARMEL_HIP_OK) {
    if (go.expectation) throw std::runtime_error("can't print sample when using expectation because there is no single sample.\n");
    r.final_sample = fetch_samples(gs, r.nblocks);
  }
  if ((tab.want_counts || tab.want_norms) && rc == CARMEL_HIP_OK) {
    r.final_x.resize(tab.n_par);
    hip_check(carmel_hip_gibbs_final_counts(gs, r.final_x.data()), "carmel_hip_gibbs_final_counts");
  }
  carmel_hip_gibbs_destroy(gs);
  hip_check(rc, "carmel_hip_gibbs_run");
}

// Every rank holds some of the slots (the others' are empty) and afterwards every rank holds the concatenation of all of
// them: the lengths first (len), then the values in pieces of 64 Ki (every rank fills its own slots' places of one vector of
// doubles -- carmel_hip_comm_allreduce_host is the host-side collective there is).  Rank 0 is who uses it.
std::vector<double> gather_to_rank0(carmel_hip_comm* comm, const std::vector<std::vector<double> >& mine, std::vector<double>& len) {
  len.assign(mine.size(), 0.0);
  for (size_t r = 0; r < len.size(); ++r) len[r] = (double)mine[r].size();
  hip_check(carmel_hip_comm_allreduce_host(comm, len.data(), (uint32_t)len.size(), 0), "carmel_hip_comm_allreduce_host");
  size_t total = 0;
  std::vector<size_t> at(len.size() + 1, 0);
  for (size_t r = 0; r < len.size(); ++r) at[r + 1] = (total += (size_t)len[r]);
  std::vector<double> all(total, 0.0);
  for (size_t r = 0; r < len.size(); ++r) std::copy(mine[r].begin(), mine[r].end(), all.begin() + at[r]);
  for (size_t k0 = 0; k0 < total; k0 += 1u << 16)
    hip_check(carmel_hip_comm_allreduce_host(comm, all.data() + k0, (uint32_t)std::min<size_t>(1u << 16, total - k0), 0),
              "carmel_hip_comm_allreduce_host");
  return all;
}

// the runs' periodic output to rank 0, in run order
void gather_periodic_text(const Job& j, const std::vector<std::string>& text) {
  std::vector<std::vector<double> > mine(text.size());
  for (size_t r = 0; r < text.size(); ++r)
    for (unsigned char c : text[r]) mine[r].push_back((double)c);
  std::vector<double> len;
  const std::vector<double> bytes = gather_to_rank0(j.comm, mine, len);
  if (j.rank == 0) {
    std::string all(bytes.size(), ' ');
    for (size_t k = 0; k < bytes.size(); ++k) all[k] = (char)(unsigned char)bytes[k];
    std::cout << all;
  }
}

// every rank's traces (zeros for the runs it did not take) add up to the whole log; the kept run is the best of the
// ranks' bests by gibbs_stats::better, the earlier run on a tie -- what the sequential loop would have kept.  Every rank
// ends up with the winner's weights, and its sample where --print-to asks for it.
void merge_ranks(Job& j, const carmel_hip_gibbs_opts& go, GibbsRun& g) {
  const Options& o = j.o;
  carmel_hip_comm* comm = j.comm;
  const int rank = j.rank, world = j.world;
  hip_check(carmel_hip_comm_allreduce_host(comm, g.lp.data(), (uint32_t)g.lp.size(), 0), "carmel_hip_comm_allreduce_host");
  if (!g.lp_after.empty())
    hip_check(carmel_hip_comm_allreduce_host(comm, g.lp_after.data(), (uint32_t)g.lp_after.size(), 0), "carmel_hip_comm_allreduce_host");
  if (o.pi_stddev > 0)
    hip_check(carmel_hip_comm_allreduce_host(comm, g.ptrace.data(), (uint32_t)g.ptrace.size(), 0), "carmel_hip_comm_allreduce_host");
  std::vector<double> all((size_t)world * 5, 0.0);
  all[(size_t)rank * 5] = g.my_ran;
  all[(size_t)rank * 5 + 1] = g.my_stats[0];
  all[(size_t)rank * 5 + 2] = g.my_stats[1];
  all[(size_t)rank * 5 + 3] = g.my_stats[2];
  all[(size_t)rank * 5 + 4] = g.best_run;
  hip_check(carmel_hip_comm_allreduce_host(comm, all.data(), (uint32_t)all.size(), 0), "carmel_hip_comm_allreduce_host");
  int winner = -1;
  for (int r = 0; r < world; ++r) {
    if (all[(size_t)r * 5] == 0) continue;
    if (winner < 0) {
      winner = r;
      continue;
    }
    const int k = go.argmax_final ? 2 : go.argmax_sum ? 3 : 1;
    const double mine = all[(size_t)r * 5 + k], best = all[(size_t)winner * 5 + k];
    if (mine > best || (mine == best && all[(size_t)r * 5 + 4] < all[(size_t)winner * 5 + 4])) winner = r;
  }
  g.best_run = (uint32_t)all[(size_t)winner * 5 + 4];
  std::vector<double> wts(j.n_params(), 0.0);
  if (rank == winner) hip_check(carmel_hip_get_weights(j.t, wts.data()), "carmel_hip_get_weights");
  // (ln weights: -inf from the winner plus 0 from the others stays -inf)
  hip_check(carmel_hip_comm_allreduce_host(comm, wts.data(), (uint32_t)wts.size(), 0), "carmel_hip_comm_allreduce_host");
  hip_check(carmel_hip_set_weights(j.t, wts.data()), "carmel_hip_set_weights");
  if (o.print_to > o.print_from) {  // --print-to: the kept run's sample lives on the rank that ran it; it travels to rank 0 the same way
    std::vector<std::vector<double> > mine(g.nblocks);
    if (rank == winner)
      for (uint32_t b = 0; b < g.nblocks; ++b) mine[b].assign(g.final_sample[b].begin(), g.final_sample[b].end());
    std::vector<double> bl;
    const std::vector<double> ids = gather_to_rank0(comm, mine, bl);
    g.final_sample.assign(g.nblocks, std::vector<uint32_t>());
    size_t k = 0;
    for (uint32_t b = 0; b < g.nblocks; ++b)
      for (size_t i = 0; i < (size_t)bl[b]; ++i) g.final_sample[b].push_back((uint32_t)ids[k++]);
  }
}

// the log of the runs (gibbs.hpp:897, 927-955; gibbs_opts.hpp:298-312)
void print_trace(const Job& j, const carmel_hip_gibbs_opts& go, const GibbsRun& g) {
  const Options& o = j.o;
  const HostPairs& pairs = j.pairs;
  const uint32_t nblocks = g.nblocks, per_run = g.per_run;
  double n_sym = 0;  // gibbs_base::init(derivs.n_output(), derivs.size())
  for (size_t p = 0; p < pairs.size(); ++p) n_sym += (double)(pairs.out_off[p + 1] - pairs.out_off[p]);
  for (uint32_t r = 0; r < g.n_runs; ++r) {
    if (go.restarts) std::cerr << "(random restart " << r << " of " << go.restarts << "): \n";  // gibbs.hpp:897
    for (uint32_t i = 0; i <= go.iter; ++i) {  // gibbs.hpp:927-955, gibbs_opts.hpp:298-312
      const double v = o.sample_prob_after ? g.lp_after[(size_t)r * per_run + i] : g.lp[(size_t)r * per_run + i];
      std::cerr << "Gibbs i=" << i << " ";
      const double* pt = g.ptrace.data() + ((size_t)r * per_run + i) * 6;
      if (pt[0] != 0)  // propose_new_priors' line (gibbs.hpp:539-547); the scales shown are the final ones
        std::cerr << (pt[1] != 0 ? "accepted" : "rejected") << " new priors with p1=" << base2(pt[2]) << " p2=" << base2(pt[3])
                  << " a1=p2/p1=" << std::exp(pt[3] - pt[2]) << " a2=q(1|2)/q(2|1)=" << pt[4] << " p_accept=" << pt[5] << ". ";
      std::cerr << (o.sample_prob_after ? "sample(after add-back)" : go.expectation ? "sum-all-derivations" : go.mode ? "cheap(proposal)" : "cache-model")
                << " prob=" << base2(v);
      if (n_sym) std::cerr << " per-point-ppx(N=" << n_sym << ")=" << base2(-v / n_sym);
      std::cerr << " per-block-ppx(N=" << nblocks << ")=" << base2(-v / nblocks) << "\n";
    }
  }
  if (o.pi_show) {  // gibbs.hpp:826-827
    std::cerr << "Final prior-scale=[";
    for (size_t k = 0; k < g.pcum.size(); ++k) std::cerr << (k ? " " : "") << g.pcum[k];
    std::cerr << "]\n";
  }
  if (go.restarts) std::cerr << "\nKept run " << g.best_run << " of " << go.restarts << " (gibbs_stats::better)\n";
}

// the kept run: its sample's paths (an arc's weight is its probability as trained: proposal_prob after the counts were
// finalised), then the norm sums and the counts (gibbs.hpp:1066-1078); pw: the trained weights
void print_final(const Job& j, const carmel_hip_gibbs_opts& go, const GibbsTables& tab, const GibbsRun& g, const std::vector<double>& pw) {
  const double final_t = (double)go.iter - (double)(go.final_counts ? go.iter : std::min(go.burnin, go.iter));
  bool final_header = false;
  if (j.o.print_to > j.o.print_from) {
    long a, b;
    if (!print_range(j, a, b)) {
      std::cerr << "--print-from,-to gibbs [" << a << "," << b << ") is out of range for " << (j.cascade ? j.nw : 1) << " input transducers.\n";
    } else {
      std::cout << "\n# final best gibbs run (start #" << g.best_run << " t=" << final_t << "):\n";
      final_header = true;
      tab.print_paths(g.final_sample, pw, a, b);
    }
  }
  if (tab.want_counts || tab.want_norms) {  // ... then the norm sums and the counts of the kept run (gibbs.hpp:1075-1076)
    if (!final_header) std::cout << "\n# final best gibbs run (start #" << g.best_run << " t=" << final_t << "):\n";
    std::vector<double> fprob(tab.n_par);
    for (size_t pp = 0; pp < tab.n_par; ++pp) fprob[pp] = std::exp(pw[pp]);  // final_prob: the weights (a locked arc's: its own)
    tab.print_norms(go.iter + 1, final_t, g.final_x);
    tab.print_counts(true, "", go.iter + 1, final_t, g.final_x, g.final_x, g.final_x, g.final_x, fprob, g.final_x);
  }
}
}  // namespace

int train_gibbs(Job& j) {
  const Options& o = j.o;
  const int world = j.world;
  const carmel_hip_gibbs_opts go = pack_gibbs_opts(j);
  const std::vector<double> init_arc_logw = initial_weights(j);
  GibbsRun g;
  carmel_hip_gibbs* gs = create_sampler(j, go, init_arc_logw, g);
  const GibbsTables tab(j);
  PeriodicObserver periodic{j, tab, go, gs, std::vector<std::string>(world > 1 ? (size_t)go.restarts + 1 : 0)};
  if (o.print_every > 0)
    hip_check(carmel_hip_gibbs_set_observer(gs, (uint32_t)o.print_every, &PeriodicObserver::call, &periodic), "carmel_hip_gibbs_set_observer");
  if (world > 1 && (tab.want_counts || tab.want_norms))
    throw UsageError("--print-counts-* / --print-norms-* with --gpus: the tables are one process's (the runs are spread over the ranks)");
  if (world > 1) hip_check(carmel_hip_gibbs_set_run_share(gs, (uint32_t)j.rank, (uint32_t)world), "carmel_hip_gibbs_set_run_share");
  run_sampler(j, go, gs, tab, g);
  if (world > 1 && o.print_every > 0) gather_periodic_text(j, periodic.text);
  if (world > 1) {
    merge_ranks(j, go, g);
    if (j.rank > 0) return 0;
  }
  print_trace(j, go, g);
  std::vector<double> pw(j.n_params());
  hip_check(carmel_hip_get_weights(j.t, pw.data()), "carmel_hip_get_weights");
  print_final(j, go, tab, g, pw);
  write_trained_members(j, pw.data());
  return 0;
}
