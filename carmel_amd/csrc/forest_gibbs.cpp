// forest_gibbs.cpp — forest-em's Gibbs sampler over the forests (carmel_hip_forests_gibbs, include/carmel_hip.h).
//
// FForests::run_gibbs (forest-em.hpp:714-734): to_gibbs (normalise, prior = alpha * p * |group|), gibbs_base::run,
// from_gibbs (rule weights = time-averaged probabilities).  opts->mode 0: forests strictly in order (the
// reference's chain); 1: all forests of a sweep in parallel against the previous sweep's counts with each forest's
// own previous sample taken out.
//
// One GibbsRun per call holds what the schedules share; each schedule is a function of its own:
//   mode 1  sweep_parallel2    the parallel sweep, second formulation (sample_class per launch class)
//           sweep_parallel1    ... first formulation (CARMEL_HIP_FOREST_SWEEP=1, kept as the A/B reference)
//   mode 0  sweep_exact_device the exact chain, one launch a sweep (forest_exact.hip)
//           sweep_exact_host   ... forest after forest from the host (annealing, locked parameters, forest_exact_host)
//           run_restarts       --crp-restarts: batches of device chains side by side
// The kernels and their launchers are forest.hip / forest.hpp, the handle forest_host.hpp.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include "forest_host.hpp"
#include "forest_exact.hpp"
#include "gibbs_exact.hpp"  // launch_gibbs_broadcast
#include "rng.hpp"

using namespace carmel_hip;

namespace {

#define RUN(x)                             \
  do {                                     \
    const int rc_ = (x);                   \
    if (rc_ != CARMEL_HIP_OK) return rc_;  \
  } while (0)

const double NEG_INF = -std::numeric_limits<double>::infinity();

// per-parameter alphas (forest-em.hpp:689-709): a locked parameter (alpha < 0) is defined without a norm group, i.e.
// with the fixed probability it has after normalisation; the host and device norm tables are switched for this run
struct NormGuard {
  carmel_hip_forests* F;
  std::vector<uint32_t> saved;
  bool changed = false;
  ~NormGuard() {
    if (!changed) return;
    F->h_norm = saved;
    (void)hipMemcpy(F->p_norm.p, F->h_norm.data(), F->h_norm.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
  }
};

bool opt_is(const char* v, int n) { return v && atoi(v) == n; }  // an option set and equal to n

const uint32_t STACK_LDS = 32u;  // stack words a lane of the one-forest-per-lane samplers keeps in LDS

struct GibbsRun {
  carmel_hip_forests* const F;
  const carmel_hip_gibbs_opts* const o;
  double* const iter_logprob;
  double* const iter_cheap_logprob;
  const hipStream_t s;
  const uint32_t nr;
  const uint64_t ng, nf;
  // gibbs_opts::validate (gibbs_opts.hpp:253-266): --final-counts makes every sweep but the last burn-in; burnin <= iter
  const uint32_t Ni, burnin;
  NormGuard guard;
  std::vector<double> lw, prior, pn;  // normalised ln weights; priors per rule and their sums per norm group
  std::vector<uint32_t> meta;         // prior-scale group by reference norm id (= group index + 1)
  uint32_t nexti = 1;                 // ... one past the last scale index
  ForestArgs A;                       // the arguments every sweep starts from
  // the option switches, read once
  // parallel mode, second formulation (CARMEL_HIP_FOREST_SWEEP=1 selects the first, kept as the A/B reference)
  const bool sweep2;
  // the walk of forest_sample_kernel over tables in LDS (CARMEL_HIP_FOREST_LDSWALK=0: over the global stream, the A/B reference)
  const bool lds_walk;
  // several lanes per forest in the parallel sweep (CARMEL_HIP_FOREST_MULTI=0: one forest per lane, the A/B reference -- and the
  // chain whose uniforms are keyed like the sequential walk's)
  const bool multi;
  const bool logdomain;    // the log domain at temperature 1 too
  const bool force_gcol;   // experiment: every class one forest per lane, columns in global memory
  const bool nohash;       // A/B of the first formulation: scan the previous sample instead of the own-sample tables
  const bool gather_opt;   // forest_gather=1: the counts gathered from the nodes' use counts (sweep_parallel2)
  const bool timing;
  bool exact_dev = false;  // mode 0 runs on the device (setup_exact_device)
  // scratch of the run
  DevBuf<double> gcol_exact;  // exact mode from the host: the inside column of one forest too large for LDS
  DevBuf<uint32_t> ghash;     // parallel mode: global own-sample tables, only when some derivation can overflow the LDS table
  DevBuf<unsigned long long> trace_buf;  // experiment: per-wave phase stamps of the last parallel sweep
  const char* trace_path = nullptr;
  FExactArgs XA;
  DevBuf<double> x_ccount, x_csum, x_idle;
  DevBuf<unsigned long long> x_clk;
  // parallel mode
  int cur = 0;               // the sample buffer the last sweep wrote
  DevBuf<double> iter_all;   // {-, ln proposal probability of the sweep's samples} per sweep
  std::vector<double> iter_host;
  uint32_t io_done = 0;
  bool side_pending = false;  // recounts still on the side streams (joined before anything reads what they write)
  // host mirror of counts for the exact schedule driven from the host (one forest at a time: the counts move between forests),
  // and of the device chain's state while a prior-scale proposal is made
  std::vector<double> hx, hs, ht, hn;
  std::vector<std::vector<uint32_t> > hsample;

  GibbsRun(carmel_hip_forests* F_, const carmel_hip_gibbs_opts* o_, double* lp, double* cheap)
      : F(F_), o(o_), iter_logprob(lp), iter_cheap_logprob(cheap), s(F_->stream), nr(F_->n_rules), ng(F_->n_groups),
        nf(F_->n_forests), Ni(o_->iter), burnin(o_->final_counts ? o_->iter : std::min(o_->burnin, o_->iter)), guard{F_, {}},
        sweep2(o_->mode == 1 && F_->sweep2_ok && !opt_is(lib_opt("forest_sweep"), 1)), lds_walk(!lib_opt_off("forest_ldswalk")),
        multi(sweep2 && F_->multi_ok && !lib_opt_off("forest_multi")), logdomain(lib_opt_set("forest_logdomain")),
        force_gcol(lib_opt_set("forest_gcol")), nohash(lib_opt_set("forest_nohash")), gather_opt(opt_is(lib_opt("forest_gather"), 1)),
        timing(lib_opt_set("timing")) {
    std::memset(&XA, 0, sizeof XA);
  }
  double sweep_time(uint32_t iter) const { return iter == 0 ? 0.0 : std::max(0.0, (double)iter - (double)burnin); }

  int setup_priors(double alpha);
  void setup_prior_scale();
  int setup_state();
  int setup_parallel();
  int setup_exact_device();
  void final_weights(std::vector<double>& x, std::vector<double>& sacc, const std::vector<double>& tm, std::vector<double>& out);
  int run_restarts();
  void parallel_args(uint32_t iter);
  int sample_class(size_t ci, bool ext, bool fold_proposal, bool gather_counts, uint32_t iter,
                   std::vector<std::function<hipError_t()> >& late_recounts);
  hipError_t recount_class(size_t ci, const ForestArgs& Ac, int cur_new, bool class_nodes, bool gather_counts);
  int sweep_parallel2(uint32_t iter);
  int sweep_parallel1(uint32_t iter);
  int commit(uint32_t iter, bool reset, bool gathered);
  int read_back_probabilities(uint32_t iter);
  int sweep_exact_device(uint32_t iter, double& cache_lp, double& cheap_lp);
  int sweep_exact_host(uint32_t iter, double& cache_lp, double& cheap_lp);
  bool infers_priors(uint32_t iter) const;
  int propose_new_priors(uint32_t iter);
  int finalise();
};

// define_gibbs(true): normalise the current weights (counts := weights), then priors
int GibbsRun::setup_priors(double alpha) {
  lw.resize(nr);
  HIPCHK(hipMemcpyAsync(lw.data(), F->rule_logw.p, nr * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  auto alpha_of = [&](uint32_t r) { return r < F->h_alphas.size() ? F->h_alphas[r] : alpha; };
  prior.assign(nr, 0.0);
  pn.assign(ng, 0.0);
  for (uint64_t gi = 0; gi < ng; ++gi) {
    double sum = 0;
    const uint64_t j0 = F->h_group_off[gi], j1 = F->h_group_off[gi + 1];
    for (uint64_t j = j0; j < j1; ++j) sum += std::exp(lw[F->h_group_rule[j]]);
    for (uint64_t j = j0; j < j1; ++j) {
      uint32_t r = F->h_group_rule[j];
      double p = sum > 0 ? std::exp(lw[r]) / sum : 1.0 / (double)(j1 - j0);
      lw[r] = p > 0 ? std::log(p) : NEG_INF;
      const double a = alpha_of(r);
      if (a < 0) {
        if (!guard.changed) {
          guard.saved = F->h_norm;
          guard.changed = true;
        }
        F->h_norm[r] = F_NONORM;
        continue;
      }
      prior[r] = o->uniform_p0 ? a : a * p * (double)(j1 - j0);
      pn[gi] += prior[r];
    }
  }
  setup_prior_scale();
  if (guard.changed) HIPCHK(hipMemcpyAsync(F->p_norm.p, F->h_norm.data(), nr * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  for (uint32_t r = 0; r < nr; ++r)
    if (F->h_norm[r] == F_NONORM) prior[r] = std::exp(lw[r]);
  return CARMEL_HIP_OK;
}

// prior-scale groups as forest-em builds them (forest-em.hpp:723-734 to_gibbs; normalize.hpp:194-210; gibbs.hpp:572-579):
// the norm ids given to define_param_id start at ONE while to_gibbs registers scale groups for ids 0 .. G-1, so norm group
// g is scaled by scale index g + 2, the first factor is drawn for nobody, and finish_params' resize(nnorm) leaves the LAST
// norm group with the never-scaled index 0; every drawn factor enters q(old|new)/q(new|old) all the same.
void GibbsRun::setup_prior_scale() {
  F->pi_trace.assign((size_t)(o->iter + 1) * 6, 0.0);
  F->pi_cumulative.clear();
  if (!(F->pi_stddev > 0)) return;
  uint32_t nnorm = 0;
  for (uint32_t r = 0; r < nr; ++r)
    if (F->h_norm[r] != F_NONORM) nnorm = std::max(nnorm, F->h_norm[r] + 2);
  meta.assign(nnorm, 0u);
  for (uint32_t i = 0; i < nnorm && i < ng; ++i) meta[i] = i + 1;
  nexti = (uint32_t)ng + 1;
  if (F->pi_global) {
    nexti = 2;
    std::fill(meta.begin(), meta.end(), 1u);
  }
  if (F->pi_local) {
    nexti = nnorm + 1;
    for (uint32_t i = 0; i < nnorm; ++i) meta[i] = i + 1;
  }
  F->pi_cumulative.assign(nexti - 1, 1.0);
}

// the sampler's state on the device: counts = priors, no sample, time 0; the base arguments
int GibbsRun::setup_state() {
  HIPCHK(F->p_prior.upload(prior, s));
  HIPCHK(F->prior_norm.upload(pn, s));
  HIPCHK(F->p_x.upload(prior, s));
  HIPCHK(F->normsum.upload(pn, s));
  HIPCHK(F->p_s.alloc(nr));
  HIPCHK(F->p_tmax.alloc(nr));
  HIPCHK(F->new_x.alloc(nr));
  HIPCHK(hipMemsetAsync(F->p_s.p, 0, nr * sizeof(double), s));
  HIPCHK(hipMemsetAsync(F->p_tmax.p, 0, nr * sizeof(double), s));
  for (int k = 0; k < 2; ++k) {
    HIPCHK(F->sample_len[k].alloc(nf));
    HIPCHK(F->sample_rules[k].alloc(F->h_sample_off.back() + 128));  // (+ forest_exact_kernel's staging reads a fixed number of words ahead)
    HIPCHK(hipMemsetAsync(F->sample_len[k].p, 0, nf * sizeof(uint32_t), s));
  }
  fill_args(F, A);
  A.p_prior = F->p_prior.p;
  A.seed = o->seed;
  A.counterfactual = 1;
  F->best_run = 0;
  return CARMEL_HIP_OK;
}

// mode 1: the buffers of the formulation that runs, the sweeps' probabilities (a slot per sweep, read back in batches)
int GibbsRun::setup_parallel() {
  if (sweep2) {
    // the classes' recounts run beside the classes still sampling: the norm sums being recounted have a buffer of their own
    HIPCHK(F->normsum2.alloc(ng));
    HIPCHK(F->sample_cls.alloc(F->h_sample_off.back() + 64));  // (+ the sampler's staging reads a fixed number of words ahead)
    HIPCHK(F->rec_logp.alloc(F->stream_total));
    HIPCHK(F->rec_p.alloc(F->stream_total));
    HIPCHK(hipMemsetAsync(F->rec_p.p, 0, F->rec_p.bytes(), s));  // the sample kernel reads every slot of its chunks
    HIPCHK(hipMemsetAsync(F->rec_logp.p, 0, F->rec_logp.bytes(), s));
    HIPCHK(F->sample_hdr.alloc(F->h_sample_off.back()));
    A.rec_cls = F->rec_cls.p;
    A.rec_logp = F->rec_logp.p;
    A.rec_p = F->rec_p.p;
    A.sample_hdr = F->sample_hdr.p;
    A.lane_of_forest = F->lane_of_forest_d.p;
  }
  (void)prepare_forest_recount();
  if (!sweep2 && (uint64_t)F->max_sample * 20 > 32 * 9 && !nohash) {
    HIPCHK(ghash.alloc((size_t)nf * FOREST_GHASH));
    A.ghash = ghash.p;
  }
  trace_path = lib_opt("forest_trace");
  if (trace_path) {
    HIPCHK(trace_buf.alloc(F->h_groups.size() * 8 * 8));  // (the several-lanes sampler: eight workgroups per lane group)
    HIPCHK(hipMemset(trace_buf.p, 0, trace_buf.bytes()));
    A.trace = trace_buf.p;
  }
  HIPCHK(iter_all.alloc(2 * ((size_t)Ni + 1)));
  HIPCHK(hipMemsetAsync(iter_all.p, 0, iter_all.bytes(), s));
  iter_host.assign(2 * ((size_t)Ni + 1), 0.0);
  return CARMEL_HIP_OK;
}

// exact mode on the device (forest_exact.hip): one persistent wavefront per sweep, every count in device memory.  It needs
// the per-forest height tables of the several-lanes sampler and runs at temperature 1; annealed runs and locked parameters keep
// the host-driven loop (prior-scale inference: the proposals between sweeps are made on the host either way).
int GibbsRun::setup_exact_device() {
  exact_dev = F->multi_ok && !guard.changed && (o->high_temp == 0 || o->high_temp == 1) && (o->low_temp == 0 || o->low_temp == 1) &&
              nf > 0 && !lib_opt("forest_exact_host");
  if (exact_dev) {
    for (auto& c : F->classes) {
      XA.max_n = std::max(XA.max_n, c.m_n);
      XA.max_tab = std::max(XA.max_tab, c.m_tab);
      XA.max_stack = std::max(XA.max_stack, c.max_kids + 2);
    }
    XA.max_sample = F->max_sample + 1;
    if (XA.max_stack > 0xffffu || XA.max_sample > 0xffffu ||
        forest_exact_lds_bytes(XA.max_n, XA.max_tab, XA.max_stack, XA.max_sample) > F_LDS_LIMIT)
      exact_dev = false;
  }
  if (!exact_dev) {  // the host keeps the counts
    hx = prior;
    hs.assign(nr, 0.0);
    ht.assign(nr, 0.0);
    hn = pn;
    hsample.assign(nf, {});
    return CARMEL_HIP_OK;
  }
  HIPCHK(x_ccount.alloc(nr));
  HIPCHK(x_csum.alloc(std::max<uint64_t>(ng, 1)));
  HIPCHK(F->sample_cls.alloc(F->h_sample_off.back() + 128));  // here: the norm group of every sample entry
  XA.xdesc = (const uint4*)F->x_desc.p;
  XA.xrec = (const uint4*)F->x_rec.p;
  XA.tab = F->mt_tab.p;
  XA.hdr = F->mt_hdr.p;
  XA.slots = (const uint4*)F->mt_slots.p;
  XA.lane_of_forest = F->lane_of_forest_d.p;
  XA.sample_len = F->sample_len[0].p;
  XA.sample_rules = F->sample_rules[0].p;
  XA.sample_nn = F->sample_cls.p;
  XA.p_x = F->p_x.p;
  XA.normsum = F->normsum.p;
  XA.p_prior = F->p_prior.p;
  XA.ccount = x_ccount.p;
  XA.csum = x_csum.p;
  XA.iter_out = F->iter_out.p;
  XA.seed = o->seed;
  XA.n_forests = (uint32_t)nf;
  HIPCHK(x_idle.alloc(256));
  HIPCHK(hipMemsetAsync(x_idle.p, 0, 256 * sizeof(double), s));
  XA.idle = x_idle.p;
  if (lib_opt("forest_exact_clk")) {
    HIPCHK(x_clk.alloc(8));
    HIPCHK(hipMemsetAsync(x_clk.p, 0, 64, s));
    XA.phase_clk = x_clk.p;
  }
  return CARMEL_HIP_OK;
}

// finalize_cumulative_counts + from_gibbs of one finished run (gibbs.hpp:629-640, forest-em.hpp:736-741): ln weights from its
// counts, their time-weighted sums and stamps
void GibbsRun::final_weights(std::vector<double>& x, std::vector<double>& sacc, const std::vector<double>& tm, std::vector<double>& out) {
  if (!(o->final_counts && !o->exclude_prior)) {
    const double tmax1 = ((double)Ni - (double)burnin) + 1.0;
    if (o->exclude_prior)  // --crp-exclude-prior (gibbs.hpp:629-631): addbase(-prior) before the counts are extended
      for (uint32_t r = 0; r < nr; ++r)
        if (F->h_norm[r] != F_NONORM) {
          sacc[r] += -prior[r] * tm[r];
          x[r] += -prior[r];
        }
    if (!o->final_counts)
      for (uint32_t r = 0; r < nr; ++r)
        if (F->h_norm[r] != F_NONORM) {
          sacc[r] += x[r] * (tmax1 - tm[r]);
          x[r] = sacc[r];
        }
  }
  std::vector<double> ns(ng, 0.0);
  for (uint32_t r = 0; r < nr; ++r)
    if (F->h_norm[r] != F_NONORM) ns[F->h_norm[r]] += x[r];
  for (uint32_t r = 0; r < nr; ++r) {
    double pr = F->h_norm[r] == F_NONORM ? prior[r] : (x[r] > 0 ? x[r] / ns[F->h_norm[r]] : 0.0);
    out[r] = pr > 0 ? std::log(pr) : NEG_INF;
  }
}

// ---- --crp-restarts (gibbs_base::run_starts, gibbs.hpp:880-914, which forest-em's sampler runs through like carmel's): every
// run starts from the priors and draws the uniforms of its own sweeps (run r, sweep i: those of sweep r * (iter + 1) + i), the
// run that is better by gibbs_stats::better gives the weights and the sample.  Independent chains: they run SIDE BY SIDE, chain c
// = workgroup c of forest_exact_kernel (one wavefront each; FExactArgs::n_chains), one launch per sweep for all of them, in
// batches of at most 64 chains / 8 GB of state.  The device chain only: temperature 1, no locked parameter, no prior inference.
int GibbsRun::run_restarts() {
  if (o->mode != 0 || !exact_dev || F->pi_stddev > 0)
    return fail(CARMEL_HIP_ERR_UNSUPPORTED, "--crp-restarts runs the exact chain on the device: no --crp-parallel, annealing, locked parameters (negative --alpha entries) or prior inference");
  const uint32_t n_runs = o->restarts + 1;
  const uint64_t S = F->sample_rules[0].n, ngs = std::max<uint64_t>(ng, 1);
  uint32_t cap = 64;
  if (const char* e = lib_opt("gibbs_chains")) cap = (uint32_t)std::max(1, atoi(e));  // 1: one run after the other (A/B)
  const uint64_t chain_bytes = ((uint64_t)nr * 4 + ngs * 2) * 8 + S * 8 + nf * 4 + 64;
  cap = (uint32_t)std::min<uint64_t>(cap, std::max<uint64_t>(1, (8ull << 30) / chain_bytes));
  DevBuf<double> mx, ms, mt, mn, mcc, mcs, mio;
  DevBuf<uint32_t> mlen, mrules, mnn;
  double best_all = 0, best_final = 0, best_sum = 0;
  bool ran_any = false;
  std::vector<double> best_lw(nr), clw(nr), x(nr), sacc(nr), tm(nr);
  std::vector<uint32_t> best_rules, best_len;
  for (uint32_t b0 = 0; b0 < n_runs; b0 += cap) {
    const uint32_t R = std::min(cap, n_runs - b0);
    if (mx.n < (size_t)R * nr) {
      HIPCHK(mx.alloc((size_t)R * nr));
      HIPCHK(ms.alloc((size_t)R * nr));
      HIPCHK(mt.alloc((size_t)R * nr));
      HIPCHK(mn.alloc((size_t)R * ngs));
      HIPCHK(mcc.alloc((size_t)R * nr));
      HIPCHK(mcs.alloc((size_t)R * ngs));
      HIPCHK(mio.alloc((size_t)R * 2));
      HIPCHK(mlen.alloc((size_t)R * nf));
      HIPCHK(mrules.alloc((size_t)R * S));
      HIPCHK(mnn.alloc((size_t)R * S));
    }
    // init_run for every chain: counts = priors, norm sums = their sums, no sample, time 0
    HIPCHK(launch_gibbs_broadcast(mx.p, F->p_prior.p, nr, R, s));
    if (ng) HIPCHK(launch_gibbs_broadcast(mn.p, F->prior_norm.p, ng, R, s));
    HIPCHK(hipMemsetAsync(ms.p, 0, (size_t)R * nr * sizeof(double), s));
    HIPCHK(hipMemsetAsync(mt.p, 0, (size_t)R * nr * sizeof(double), s));
    HIPCHK(hipMemsetAsync(mlen.p, 0, (size_t)R * nf * sizeof(uint32_t), s));
    FExactArgs XC = XA;
    XC.sample_len = mlen.p;
    XC.sample_rules = mrules.p;
    XC.sample_nn = mnn.p;
    XC.p_x = mx.p;
    XC.normsum = mn.p;
    XC.ccount = mcc.p;
    XC.csum = mcs.p;
    XC.iter_out = mio.p;
    XC.phase_clk = nullptr;
    XC.n_chains = R;
    XC.iter_stride = Ni + 1;
    XC.ch_rules = nr;
    XC.ch_norms = ng;
    XC.ch_sample = S;
    XC.ch_forests = nf;
    if (R == 1) {  // (a lone chain is the kernel's plain form: the strides do not apply, the base sweep does)
      XC.n_chains = 0;
    }
    std::vector<double> st_all(R, 0.0), st_final(R, 0.0), st_sum(R, NEG_INF), io((size_t)R * 2);
    for (uint32_t iter = 0; iter <= Ni; ++iter) {
      const double time = sweep_time(iter);
      HIPCHK(hipMemsetAsync(mio.p, 0, (size_t)R * 2 * sizeof(double), s));
      HIPCHK(launch_gibbs_broadcast(mcc.p, F->p_prior.p, nr, R, s));
      if (ng) HIPCHK(launch_gibbs_broadcast(mcs.p, F->prior_norm.p, ng, R, s));
      HIPCHK(launch_forest_fold(ms.p, mt.p, mx.p, time, (uint64_t)R * nr, s));
      XC.iter = b0 * (Ni + 1) + iter;
      HIPCHK(launch_forest_exact(XC, s));
      HIPCHK(hipMemcpyAsync(io.data(), mio.p, io.size() * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      for (uint32_t c = 0; c < R; ++c) {
        const uint32_t run = b0 + c;
        const double plog = io[(size_t)c * 2];
        if (iter_logprob) iter_logprob[(size_t)run * (Ni + 1) + iter] = plog;
        if (iter_cheap_logprob) iter_cheap_logprob[(size_t)run * (Ni + 1) + iter] = io[(size_t)c * 2 + 1];
        if (iter >= burnin) {  // gibbs.hpp:942-943: the statistics runs are compared by
          st_all[c] += plog;
          st_final[c] = plog;
          const double hi = std::max(st_sum[c], plog), lo = std::min(st_sum[c], plog);
          st_sum[c] = hi + (lo == NEG_INF ? 0.0 : std::log1p(std::exp(lo - hi)));
        }
      }
    }
    for (uint32_t c = 0; c < R; ++c) {  // the better run by gibbs_stats::better (gibbs_opts.hpp:313-316), in run order
      const bool better = !ran_any || (o->argmax_final ? st_final[c] > best_final : o->argmax_sum ? st_sum[c] > best_sum : st_all[c] > best_all);
      ran_any = true;
      if (!better) continue;
      HIPCHK(hipMemcpyAsync(x.data(), mx.p + (size_t)c * nr, nr * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(sacc.data(), ms.p + (size_t)c * nr, nr * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(tm.data(), mt.p + (size_t)c * nr, nr * sizeof(double), hipMemcpyDeviceToHost, s));
      best_rules.resize(S);
      best_len.resize(nf);
      HIPCHK(hipMemcpyAsync(best_rules.data(), mrules.p + (size_t)c * S, S * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(best_len.data(), mlen.p + (size_t)c * nf, nf * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      final_weights(x, sacc, tm, clw);
      F->h_final_x = x;
      best_lw = clw;
      F->best_run = b0 + c;
      best_all = st_all[c];
      best_final = st_final[c];
      best_sum = st_sum[c];
    }
  }
  // the kept run's sample is the sampler's sample (carmel_hip_forests_get_sample, --outsample-file)
  HIPCHK(hipMemcpyAsync(F->sample_rules[0].p, best_rules.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(F->sample_len[0].p, best_len.data(), nf * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  return carmel_hip_forests_set_weights(F, best_lw.data());
}

// a parallel sweep: all forests against the counts of the previous sweep, own previous sample taken out in-kernel
void GibbsRun::parallel_args(uint32_t iter) {
  A.iter = iter;
  A.power = gibbs_anneal_power(o->high_temp, o->low_temp, Ni, iter);
  A.iter_out = iter_all.p + 2 * (size_t)iter;  // a slot per sweep: the host runs ahead of the device, no round trip per sweep
  A.snap_x = F->p_x.p;
  A.snap_norm = F->normsum.p;
  A.old_len = F->sample_len[cur].p;
  A.old_rules = F->sample_rules[cur].p;
  A.sample_len = F->sample_len[cur ^ 1].p;
  A.sample_rules = F->sample_rules[cur ^ 1].p;
}

// second formulation: the sampler of one launch class and the recount of its samples, on the class's stream
int GibbsRun::sample_class(size_t ci, bool ext, bool fold_proposal, bool gather_counts, uint32_t iter,
                           std::vector<std::function<hipError_t()> >& late_recounts) {
  const auto& c = F->classes[ci];
  const hipStream_t cs = sweep_stream(F, s, ci);
  A.first_group = c.first;
  // temperature 1 (ext): mantissa / exponent arithmetic (12 bytes per node); annealing: the log domain
  FSampleLaunch L;
  L.gcol = forest_cols_exceed_lds(c.max_nodes) || force_gcol;
  L.ext = ext;
  L.n_groups = c.count;
  L.max_sample = F->max_sample;
  L.max_nodes = c.max_nodes;
  L.stack_lds = STACK_LDS;
  L.kid_rows = std::max(c.max_kids, 1u);
  L.lw = lds_walk && c.max_nodes < 0x8000u && c.max_kids < 0x8000u && c.maxlen <= 0x10000u && !forest_cols_exceed_lds(c.max_nodes) &&
         forest_sample_lw_lds_bytes(c.max_nodes, ext, L.kid_rows, STACK_LDS) <= F_LDS_LIMIT;
  bool class_nodes = false;  // the class's sample is written as node numbers (FMultiArgs::prob)
  // several lanes per forest (temperature 1, tables within LDS): forest_sample_multi_kernel
  if (multi && ext && forest_multi_lds_bytes(c.m_n, c.m_tab, c.m_front) * FM_FPW <= 64 * 1024 && !force_gcol) {
    FMultiArgs MA;
    MA.tab = F->mt_tab.p;
    MA.hdr = F->mt_hdr.p;
    MA.slots = (const uint4*)F->mt_slots.p;
    MA.lane_lo = c.first * 64u;
    MA.lane_hi = (uint32_t)std::min<uint64_t>((uint64_t)(c.first + c.count) * 64u, F->h_groups.size() * 64);
    MA.max_tab = c.m_tab;
    MA.max_n = c.m_n;
    MA.max_front = c.m_front;
    MA.own_proposal = fold_proposal ? 1 : 0;
    if (fold_proposal && !F->mt_prob.n) HIPCHK(F->mt_prob.alloc(F->mt_hdr.n / 4 + 8));
    MA.prob = F->mt_prob.p;
    MA.node_cnt = gather_counts ? F->mt_node_cnt.p : nullptr;
    class_nodes = fold_proposal;
    if (iter == 0 && timing)
      fprintf(stderr, "timing: forest sweep class %zu: %u wavefronts of %d forests, nodes <= %u, table <= %u words, frontier <= %u: %zu bytes of LDS a wavefront\n",
              ci, forest_multi_workgroups(MA), (int)FM_FPW, c.m_n, c.m_tab, c.m_front,
              forest_multi_lds_bytes(c.m_n, c.m_tab, c.m_front) * FM_FPW);
    HIPCHK(launch_forest_sample_multi(A, MA, F->max_sample, cs));
  } else {
    if (L.gcol) {
      A.gcol = F->gcol.p + F->gcol_off[ci];
      A.gcol_stride = (uint64_t)2 * c.max_nodes * 64;
    }
    HIPCHK(launch_forest_sample(A, L, cs));
  }
  // this class's new samples: rule ids, class words, ln proposal probability -- and, unless the counts are gathered, the
  // counts -- on its own stream, while the other classes still sample.  (With the counts in it, all samplers first and
  // the recounts behind them was 335 us against 316: bound by their atomics they take as long side by side.)
  const ForestArgs Ac = A;
  const int cur_new = cur ^ 1;
  if (gather_counts)  // (behind the commit: nothing the next sweep's counts need waits for them)
    late_recounts.push_back([=]() { return recount_class(ci, Ac, cur_new, class_nodes, true); });
  else
    HIPCHK(recount_class(ci, Ac, cur_new, class_nodes, false));
  return CARMEL_HIP_OK;
}

hipError_t GibbsRun::recount_class(size_t ci, const ForestArgs& Ac, int cur_new, bool class_nodes, bool gather_counts) {
  const auto& c = F->classes[ci];
  FRecount RC;
  RC.sample_off = F->sample_off.p;
  RC.sample_len = F->sample_len[cur_new].p;
  RC.rules = F->sample_rules[cur_new].p;
  RC.p_norm = F->p_norm.p;
  RC.x = F->new_x.p;
  RC.normsum = F->normsum2.p;
  RC.n_forests = (uint32_t)nf;
  RC.sweep2 = gather_counts ? 3 : 1;
  RC.slot_forest = F->lane_forest.p;
  RC.slot0 = c.first * 64u;
  RC.slot1 = (c.first + c.count) * 64u;
  RC.node_hdr = class_nodes ? (const uint32_t*)F->mt_hdr.p : nullptr;
  RC.node_prob = F->mt_prob.p;
  RC.node_slots = (const uint4*)F->mt_slots.p;
  return launch_forest_recount(RC, Ac, sweep_stream(F, s, ci));
}

int GibbsRun::sweep_parallel2(uint32_t iter) {
  parallel_args(iter);
  std::vector<std::function<hipError_t()> > late_recounts;  // (gathered counts: the recounts, launched behind the commit)
  A.sample_cls = F->sample_cls.p;
  // (the previous sample's class words, written by its recount: what the proposal kernel scans for the forest's own uses)
  A.and_list = F->and_list.p;
  A.n_and = F->n_and;
  const bool ext = A.power == 1.0 && !logdomain;
  A.p_only = ext ? 1 : 0;
  // every launch class on the several-lanes sampler: it computes the proposal probabilities itself (no kernel in front
  // of the classes, no rec_p round trip)
  bool fold_proposal = multi && ext;
  for (auto& c : F->classes)
    if (forest_multi_lds_bytes(c.m_n, c.m_tab, c.m_front) * FM_FPW > 64 * 1024) fold_proposal = false;
  if (force_gcol) fold_proposal = false;
  // the counts gathered from the nodes' use counts instead of added up by the recounts' atomics (forest_rule_gather_kernel)
  // (forest_gather = 1; measured on config 5: 348 us a sweep against 316 -- the gather is 2.5 M scattered two-byte reads, 47 us,
  // as many requests as the atomics it replaces, and the sweep gains two cross-stream waits; what it buys is counts that
  // are the same bits run after run)
  const bool gather_counts = fold_proposal && F->inv_off.n && F->mt_node_cnt.n && gather_opt;
  if (!fold_proposal) HIPCHK(launch_forest_proposal(A, s));
  if (iter == 0) {  // the new counts start from the priors; the norm sums go to the other buffer (this
                    // sweep reads the current one).  Later sweeps: prepared at the end of the previous one
    HIPCHK(hipMemcpyAsync(F->new_x.p, F->p_prior.p, nr * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(F->normsum2.p, F->prior_norm.p, ng * sizeof(double), hipMemcpyDeviceToDevice, s));
  }
  HIPCHK(fork_side(F, s));
  sweep_schedule(F);
  for (size_t ci : F->sweep_order) RUN(sample_class(ci, ext, fold_proposal, gather_counts, iter, late_recounts));
  if (gather_counts) {
    // the caller's stream waits for the SAMPLERS of the side streams only, gathers the counts and commits them; the recounts
    // follow on their streams and run into the next sweep (a class's next sampler is behind its recount on its own stream)
    for (int k = 0; k < n_side_for(F); ++k) {
      HIPCHK(hipEventRecord(F->ev_samp[k], F->side[k]));
      HIPCHK(hipStreamWaitEvent(s, F->ev_samp[k], 0));
    }
    HIPCHK(launch_forest_rule_gather(F->inv_off.p, F->inv_node.p, (const uint16_t*)F->mt_node_cnt.p, F->rule_cnt.p, nr, F->inv_pieces.p,
                                     F->n_inv_pieces, (uint32_t)F->inv_node.n, s));
    HIPCHK(launch_forest_group_sum(F->group_off.p, F->group_rule.p, ng, F->rule_cnt.p, F->prior_norm.p, F->normsum2.p, s));
    side_pending = true;
  } else
    HIPCHK(join_side(F, s));
  cur ^= 1;
  std::swap(F->normsum.p, F->normsum2.p);  // the sums the classes just recounted become the current ones
  // (the next sweep's count buffers start from the priors, reset by the commit itself)
  RUN(commit(iter, iter < Ni, gather_counts));
  for (auto& r : late_recounts) HIPCHK(r());
  return CARMEL_HIP_OK;
}

// first formulation: one forest per lane with its own previous sample in a hash table, one recount after all classes
int GibbsRun::sweep_parallel1(uint32_t iter) {
  parallel_args(iter);
  const uint32_t own_cap_max = 256u;
  for (size_t ci = 0; ci < F->classes.size(); ++ci) {
    const auto& c = F->classes[ci];
    A.first_group = c.first;
    // LDS: the inside column + up to own_cap {rule, norm group} pairs of the previous sample per lane
    uint32_t own_cap = own_cap_max;  // hash slots per lane, fewer when the inside column is large
    while (own_cap && forest_gibbs_lds_bytes(false, c.max_nodes, own_cap, STACK_LDS) > 156 * 1024) own_cap >>= 1;
    if (own_cap < 32) own_cap = 0;
    if (nohash) own_cap = 0;
    const bool gcol = forest_cols_exceed_lds(c.max_nodes);
    if (gcol) {
      own_cap = nohash ? 0 : own_cap_max;
      A.gcol = F->gcol.p + F->gcol_off[ci];
      A.gcol_stride = (uint64_t)2 * c.max_nodes * 64;
    }
    HIPCHK(launch_forest_gibbs(A, gcol, c.count, F->max_sample, c.max_nodes, own_cap, STACK_LDS, s));
  }
  cur ^= 1;
  HIPCHK(hipMemcpyAsync(F->new_x.p, F->p_prior.p, nr * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(F->normsum.p, F->prior_norm.p, ng * sizeof(double), hipMemcpyDeviceToDevice, s));
  FRecount RC;
  std::memset(&RC, 0, sizeof RC);  // (all forests, first formulation: no class, no node tables)
  RC.sample_off = F->sample_off.p;
  RC.sample_len = F->sample_len[cur].p;
  RC.rules = F->sample_rules[cur].p;
  RC.p_norm = F->p_norm.p;
  RC.x = F->new_x.p;
  RC.normsum = F->normsum.p;
  RC.n_forests = (uint32_t)nf;
  HIPCHK(launch_forest_recount(RC, A, s));
  return commit(iter, false, false);
}

// the sweep's counts (new_x, or the gathered use counts) become the current ones, their time-weighted sums move on
int GibbsRun::commit(uint32_t iter, bool reset, bool gathered) {
  FCommit C;
  C.new_x = F->new_x.p;
  C.p_x = F->p_x.p;
  C.p_s = F->p_s.p;
  C.p_tmax = F->p_tmax.p;
  C.p_norm = F->p_norm.p;
  C.time = sweep_time(iter);
  C.n = nr;
  C.reset_x = reset ? F->p_prior.p : nullptr;
  C.next_norm = reset ? F->normsum2.p : nullptr;
  C.reset_norm = F->prior_norm.p;
  C.n_norm = ng;
  C.rule_cnt = gathered ? F->rule_cnt.p : nullptr;
  C.prior = F->p_prior.p;
  HIPCHK(launch_forest_commit(C, s));
  return CARMEL_HIP_OK;
}

// the parallel sweeps' probabilities, 64 sweeps at a time
int GibbsRun::read_back_probabilities(uint32_t iter) {
  if (!(iter == Ni || (iter & 63u) == 63u)) return CARMEL_HIP_OK;
  if (side_pending) {  // (the side streams' recounts add to the sweeps' probabilities)
    HIPCHK(join_side(F, s));
    side_pending = false;
  }
  HIPCHK(hipMemcpyAsync(iter_host.data() + 2 * (size_t)io_done, iter_all.p + 2 * (size_t)io_done,
                        2 * (size_t)(iter + 1 - io_done) * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  for (uint32_t q = io_done; q <= iter; ++q) {
    if (iter_logprob) iter_logprob[q] = iter_host[2 * (size_t)q + 1];
    if (iter_cheap_logprob) iter_cheap_logprob[q] = iter_host[2 * (size_t)q + 1];
  }
  io_done = iter + 1;
  return CARMEL_HIP_OK;
}

// exact, on the device: the whole sweep is one launch (forest_exact.hip)
int GibbsRun::sweep_exact_device(uint32_t iter, double& cache_lp, double& cheap_lp) {
  HIPCHK(hipMemsetAsync(F->iter_out.p, 0, 2 * sizeof(double), s));
  HIPCHK(hipMemcpyAsync(x_ccount.p, F->p_prior.p, nr * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (ng) HIPCHK(hipMemcpyAsync(x_csum.p, F->prior_norm.p, ng * sizeof(double), hipMemcpyDeviceToDevice, s));
  XA.iter = iter;
  // delta_sum's fold for every parameter at once: at the start of a sweep every count is what the previous sweep left,
  // which is what the reference folds at a parameter's first touch in this sweep (delta_sum.hpp:74-84)
  HIPCHK(launch_forest_fold(F->p_s.p, F->p_tmax.p, F->p_x.p, sweep_time(iter), nr, s));
  HIPCHK(launch_forest_exact(XA, s));
  double io[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(io, F->iter_out.p, sizeof io, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  cache_lp = io[0];
  cheap_lp = io[1];
  return CARMEL_HIP_OK;
}

// exact: forest after forest; each launch resamples ONE forest on the GPU against the current counts
int GibbsRun::sweep_exact_host(uint32_t iter, double& cache_lp, double& cheap_lp) {
  const double time = sweep_time(iter);
  HIPCHK(hipMemsetAsync(F->iter_out.p, 0, 2 * sizeof(double), s));
  std::vector<double> ccount = prior, csum = pn;
  A.iter = iter;
  A.power = gibbs_anneal_power(o->high_temp, o->low_temp, Ni, iter);
  A.counterfactual = 0;
  A.snap_x = F->p_x.p;
  A.snap_norm = F->normsum.p;
  A.sample_len = F->sample_len[0].p;
  A.sample_rules = F->sample_rules[0].p;
  A.old_len = F->sample_len[0].p;
  A.old_rules = F->sample_rules[0].p;
  auto addc = [&](const std::vector<uint32_t>& b, double d) {  // gibbs.hpp:769-792 + delta_sum.hpp:74-84
    for (uint32_t r : b) {
      uint32_t n = F->h_norm[r];
      if (n == F_NONORM) continue;
      hn[n] += d;
      double moret = time - ht[r];
      if (moret > 0) {
        ht[r] = time;
        hs[r] += moret * hx[r];
      } else if (moret < 0)
        hs[r] += d * (-moret);
      hx[r] += d;
    }
  };
  auto push_counts = [&](const std::vector<uint32_t>& b) {  // upload only the (few) counts the sample touches
    for (uint32_t r : b) {
      uint32_t n = F->h_norm[r];
      if (n == F_NONORM) continue;
      HIPCHK(hipMemcpyAsync(F->p_x.p + r, &hx[r], sizeof(double), hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(F->normsum.p + n, &hn[n], sizeof(double), hipMemcpyHostToDevice, s));
    }
    return (int)CARMEL_HIP_OK;
  };
  std::vector<uint32_t> buf(F->max_sample);
  for (uint64_t f = 0; f < nf; ++f) {
    addc(hsample[f], -1.0);
    RUN(push_counts(hsample[f]));
    const uint32_t slot = F->lane_of_forest[f];
    A.serial_forest = slot;
    const uint32_t gidx = slot / 64;
    A.first_group = gidx;
    const FGroup& G = F->h_groups[gidx];
    const bool gcol = forest_gibbs_lds_bytes(false, G.max_nodes, 0u, 0u) > F_LDS_LIMIT;
    if (gcol) {
      if (!gcol_exact.n) HIPCHK(gcol_exact.alloc((size_t)F->max_nodes * 64));
      A.gcol = gcol_exact.p;
      A.gcol_stride = 0;
    }
    HIPCHK(launch_forest_gibbs(A, gcol, 1, F->max_sample, G.max_nodes, 0u, 0u, s));
    uint32_t len = 0;
    HIPCHK(hipMemcpyAsync(&len, F->sample_len[0].p + f, sizeof len, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (len) HIPCHK(hipMemcpyAsync(buf.data(), F->sample_rules[0].p + F->h_sample_off[f], len * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    hsample[f].assign(buf.begin(), buf.begin() + len);
    for (uint32_t r : hsample[f]) {  // cheap prob before re-adding; cache model (gibbs.hpp:712-742)
      uint32_t n = F->h_norm[r];
      cheap_lp += std::log(n == F_NONORM ? prior[r] : hx[r] / hn[n]);
      double q = prior[r];
      if (n != F_NONORM) {
        q = ccount[r] / csum[n];
        ccount[r] += 1.0;
        csum[n] += 1.0;
      }
      cache_lp += std::log(q);
    }
    addc(hsample[f], 1.0);
    RUN(push_counts(hsample[f]));
    HIPCHK(hipStreamSynchronize(s));
  }
  return CARMEL_HIP_OK;
}

// the sweeps that infer the prior scales (gibbs.hpp:559-563)
bool GibbsRun::infers_priors(uint32_t iter) const {
  const uint32_t pstart = F->pi_start ? F->pi_start : burnin;
  return o->mode == 0 && F->pi_stddev > 0 && nexti > 1 && iter > 0 && pstart <= iter && (!F->pi_end || iter < F->pi_end);
}

// propose_new_priors (gibbs.hpp:525-553), on the host: the proposal rescales every prior, count, norm sum and time-weighted
// sum and scores the whole sample twice.  The host-driven schedule keeps its counts there anyway; the device chain hands its
// state over for the proposal and takes it back (a few tens of MB per inferring sweep against a 0.5 s sweep).
int GibbsRun::propose_new_priors(uint32_t iter) {
  if (exact_dev) {
    hx.resize(nr);
    hs.resize(nr);
    ht.resize(nr);
    hn.resize(ng);
    std::vector<uint32_t> sl(nf), sr(F->h_sample_off.back());
    HIPCHK(hipMemcpyAsync(hx.data(), F->p_x.p, nr * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(hs.data(), F->p_s.p, nr * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ht.data(), F->p_tmax.p, nr * sizeof(double), hipMemcpyDeviceToHost, s));
    if (ng) HIPCHK(hipMemcpyAsync(hn.data(), F->normsum.p, ng * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sl.data(), F->sample_len[0].p, nf * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sr.data(), F->sample_rules[0].p, sr.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    hsample.resize(nf);
    for (uint64_t f = 0; f < nf; ++f) hsample[f].assign(sr.begin() + F->h_sample_off[f], sr.begin() + F->h_sample_off[f] + sl[f]);
  }
  const double sdev = F->pi_stddev;
  const double q0 = gibbs_norm_cdf((0.0 - 1.0) / sdev), qrem = 1.0 - q0;
  std::vector<double> sc(nexti, 1.0);
  double ln_a2 = 0.0;
  for (uint32_t k = 1; k < nexti; ++k) {
    sc[k] = 1.0 + sdev * gibbs_norm_quantile(q0 + gibbs_uniform(o->seed, iter, 0xfffffffeu, k) * qrem);
    const double d_old = 1.0 / sc[k] - 1.0, d_new = sc[k] - 1.0;
    ln_a2 += (d_new * d_new - d_old * d_old) / (2.0 * sdev * sdev);
  }
  auto cache_prob_all = [&]() {
    std::vector<double> cc = prior, cs = pn;
    double lp = 0.0;
    for (uint64_t f = 0; f < nf; ++f)
      for (uint32_t r : hsample[f]) {
        const uint32_t n = F->h_norm[r];
        double q = prior[r];
        if (n != F_NONORM) {
          q = cc[r] / cs[n];
          cc[r] += 1.0;
          cs[n] += 1.0;
        }
        lp += std::log(q);
      }
    return lp;
  };
  auto scale = [&](bool invert) {
    std::fill(pn.begin(), pn.end(), 0.0);
    for (uint32_t r = 0; r < nr; ++r) {
      const uint32_t n = F->h_norm[r];
      if (n == F_NONORM) continue;
      const uint32_t i = meta[n + 1];
      if (i > 0) {
        double fct = sc[i];
        if (invert) fct = 1.0 / fct;
        const double s2 = fct * prior[r], d = s2 - prior[r];
        hs[r] += d * ht[r];
        hx[r] += d;
        hn[n] += d;
        prior[r] = s2;
      }
      pn[n] += prior[r];
    }
  };
  const double p1 = cache_prob_all();
  scale(false);
  const double p2 = cache_prob_all();
  const double a = std::exp((p2 - p1) + ln_a2);
  const bool accept = gibbs_uniform(o->seed, iter, 0xffffffffu, 0) < a;
  if (!accept)
    scale(true);
  else
    for (uint32_t k = 1; k < nexti; ++k) F->pi_cumulative[k - 1] *= sc[k];
  HIPCHK(hipMemcpyAsync(F->p_prior.p, prior.data(), nr * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(F->prior_norm.p, pn.data(), ng * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(F->p_x.p, hx.data(), nr * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(F->normsum.p, hn.data(), ng * sizeof(double), hipMemcpyHostToDevice, s));
  if (exact_dev) HIPCHK(hipMemcpyAsync(F->p_s.p, hs.data(), nr * sizeof(double), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  double* tr = F->pi_trace.data() + (size_t)iter * 6;
  tr[0] = 1;
  tr[1] = accept ? 1 : 0;
  tr[2] = p1;
  tr[3] = p2;
  tr[4] = std::exp(ln_a2);
  tr[5] = a;
  return CARMEL_HIP_OK;
}

// finalize_cumulative_counts + from_gibbs
int GibbsRun::finalise() {
  std::vector<double> x(nr), sacc(nr), tm(nr);
  if (x_clk.n) {
    unsigned long long c[8];
    HIPCHK(hipMemcpy(c, x_clk.p, sizeof c, hipMemcpyDeviceToHost));
    fprintf(stderr, "[carmel_hip] forest_exact cycles per forest: wait+proposal %.0f, inside %.0f, walk %.0f, entries+counts %.0f (register path: %llu forests x sweeps, LDS path: %llu)\n",
            c[0] / (double)c[4], c[1] / (double)c[4], c[2] / (double)c[4], c[3] / (double)c[4], c[4], c[5]);
  }
  if (o->mode == 0 && !exact_dev) {
    x = hx;
    sacc = hs;
    tm = ht;
  } else {
    HIPCHK(hipMemcpyAsync(x.data(), F->p_x.p, nr * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(sacc.data(), F->p_s.p, nr * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(tm.data(), F->p_tmax.p, nr * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (cur != 0) {  // keep the final samples in buffer 0 for carmel_hip_forests_get_sample
      std::swap(F->sample_len[0].p, F->sample_len[1].p);
      std::swap(F->sample_rules[0].p, F->sample_rules[1].p);
    }
  }
  final_weights(x, sacc, tm, lw);
  F->h_final_x = x;
  if (trace_buf.n) {
    std::vector<unsigned long long> h(trace_buf.n);
    HIPCHK(hipMemcpy(h.data(), trace_buf.p, trace_buf.bytes(), hipMemcpyDeviceToHost));
    if (FILE* f = fopen(trace_path, "wb")) {
      fwrite(h.data(), 8, h.size(), f);
      fclose(f);
    }
  }
  return carmel_hip_forests_set_weights(F, lw.data());
}

}  // namespace

extern "C" int carmel_hip_forests_gibbs(carmel_hip_forests* F, const carmel_hip_gibbs_opts* o, double alpha, double* iter_logprob,
                                        double* iter_cheap_logprob) {
  if (!F || !o) return fail(CARMEL_HIP_ERR_ARG, "null argument");
  if (F->pi_stddev > 0 && o->mode != 0)
    return fail(CARMEL_HIP_ERR_UNSUPPORTED, "prior inference works with the cache-model probability of the exact blocked sampler only (gibbs.hpp:528-529)");
  if (o->include_self || o->random_start || o->expectation)
    return fail(CARMEL_HIP_ERR_UNSUPPORTED, "--include-self / --random-start / --expectation are carmel's (carmel_hip_gibbs_create), not the forest sampler's");
  HIPCHK(hipSetDevice(F->device));
  GibbsRun R(F, o, iter_logprob, iter_cheap_logprob);
  RUN(R.setup_priors(alpha));
  RUN(R.setup_state());
  if (o->mode == 1)
    RUN(R.setup_parallel());
  else if (o->mode == 0)
    RUN(R.setup_exact_device());
  if (o->restarts > 0) return R.run_restarts();
  for (uint32_t iter = 0; iter <= R.Ni; ++iter) {
    if (o->mode == 1) {
      RUN(R.sweep2 ? R.sweep_parallel2(iter) : R.sweep_parallel1(iter));
      RUN(R.read_back_probabilities(iter));
      continue;
    }
    double cache_lp = 0.0, cheap_lp = 0.0;
    RUN(R.exact_dev ? R.sweep_exact_device(iter, cache_lp, cheap_lp) : R.sweep_exact_host(iter, cache_lp, cheap_lp));
    if (R.infers_priors(iter)) RUN(R.propose_new_priors(iter));
    if (iter_logprob) iter_logprob[iter] = cache_lp;
    if (iter_cheap_logprob) iter_cheap_logprob[iter] = cheap_lp;
  }
  return R.finalise();
}
