// forest_host.hpp — the carmel_hip_forests handle (include/carmel_hip.h) as forest_host.cpp builds it and forest_gibbs.cpp
// runs the sampler over it; private to the two.
#pragma once
#include <algorithm>
#include <vector>
#include "engine.hpp"
#include "forest.hpp"

struct carmel_hip_forests {
  uint32_t best_run = 0;  // --crp-restarts: the run that was kept (carmel_hip_forests_best_run)
  std::vector<double> h_final_x;  // ... its counts as finalize_cumulative_counts left them (carmel_hip_forests_final_counts)
  // --prior-inference-* (gibbs_opts.hpp:82-89): carmel_hip_forests_set_prior_inference / _prior_trace
  double pi_stddev = 0;
  bool pi_global = false, pi_local = false;
  uint32_t pi_start = 0, pi_end = 0;
  std::vector<double> pi_trace, pi_cumulative;
  int device = 0;
  hipStream_t stream = nullptr;
  uint64_t n_forests = 0, n_groups = 0;
  uint32_t n_rules = 0, max_nodes = 0, max_sample = 0;
  uint64_t node_total = 0, stream_total = 0;
  static const int N_SIDE = 3;  // + the caller's stream (carmel_hip_forests_create: how they come by hardware queues of their own)
  std::vector<int> class_side;  // per launch class: -1 = the caller's stream, k = side[k] (dealt by load, largest class first)
  std::vector<int> sweep_side;     // ... for the several-lanes sampler's sweep (sweep_stream): dealt by the classes' LONGEST forest
  std::vector<size_t> sweep_order;  // ... and the order they are launched in (the class of the largest forests first)
  hipStream_t side[N_SIDE] = {};  // launch classes of one sweep run side by side
  hipEvent_t ev_fork = nullptr, ev_side[N_SIDE] = {}, ev_samp[N_SIDE] = {};  // (ev_samp: a side stream's samplers are done)
  bool sweep2_ok = false;  // the second formulation of the parallel sweep applies (class ids fit 16 bits)
  // several lanes per forest (forest_sample_multi_kernel): per-forest tables, per lane slot
  bool multi_ok = false;
  DevBuf<uint16_t> mt_tab;
  DevBuf<uint32_t> mt_hdr;
  DevBuf<uint32_t> mt_slots;  // FMultiArgs::slots
  DevBuf<double> mt_prob;     // FMultiArgs::prob
  DevBuf<uint16_t> mt_node_cnt;                         // FMultiArgs::node_cnt
  DevBuf<uint32_t> inv_off, inv_node, inv_pieces, rule_cnt;  // forest_rule_gather_kernel: rule -> its AND nodes (indices into mt_hdr / 4)
  uint32_t n_inv_pieces = 0;
  DevBuf<uint32_t> x_desc, x_rec;  // forest_exact_kernel's per-forest descriptors and per-node records (forest_exact.hpp)
  std::vector<FGroup> h_groups;
  struct Cls {
    uint32_t first, count, max_nodes;
    uint32_t max_kids = 0, maxlen = 0;  // child entries / records of the class's largest lane (LDS walk tables)
    uint32_t m_tab = 0, m_n = 0, m_front = 0;  // forest_sample_multi_kernel: table words / nodes / frontier entries of its largest forest
  };
  std::vector<Cls> classes;
  std::vector<uint32_t> h_norm, lane_of_forest;
  std::vector<double> h_alphas;  // --alpha=FILE: per-rule prior strength, negative = locked (empty: the scalar alpha)
  std::vector<uint64_t> h_group_off;
  std::vector<uint32_t> h_group_rule;
  std::vector<uint64_t> h_sample_off;
  DevBuf<FGroup> groups;
  DevBuf<uint2_t> ins_stream, out_stream;
  DevBuf<uint32_t> lane_forest, lane_nodes, hdr_pos, group_rule, p_norm, sample_len[2], sample_rules[2];
  DevBuf<uint32_t> rec_cls, sample_cls, sample_hdr, lane_of_forest_d;
  DevBuf<FAnd> and_list;
  uint64_t n_and = 0;
  DevBuf<double> gcol;               // columns of the launch classes whose forests do not fit LDS
  std::vector<uint64_t> gcol_off;    // per class: offset into gcol (doubles), room for two columns per group
  DevBuf<double> rec_logp, rec_p;
  DevBuf<uint64_t> group_off, arc_off, slot_pos, hot_chunks, sample_off;
  DevBuf<double> normsum2;  // the norm sums being recounted while a sweep still reads the current ones (carmel_hip_forests_gibbs)
  DevBuf<double> rule_logw, counts, post, forest_logprob, scalars, p_prior, p_x, p_s, p_tmax, normsum, prior_norm, new_x,
      iter_out;
  DevBuf<unsigned long long> maxbits;
};

namespace carmel_hip {
// side streams: the launch classes of one pass run side by side (each ends with a few slow waves; no class fills the
// chip).  fork_side(F, s) lets them start behind s, class_stream / sweep_stream(F, s, i) = the stream of class i,
// join_side(F, s) folds them back into s.
int n_side_for(const carmel_hip_forests* F);
hipError_t fork_side(carmel_hip_forests* F, hipStream_t s);
hipStream_t class_stream(carmel_hip_forests* F, hipStream_t s, size_t ci);
void sweep_schedule(carmel_hip_forests* F);  // fills sweep_order / sweep_side (once)
hipStream_t sweep_stream(carmel_hip_forests* F, hipStream_t s, size_t ci);
hipError_t join_side(carmel_hip_forests* F, hipStream_t s);
// the arguments every forest kernel takes, from the handle
void fill_args(carmel_hip_forests* F, ForestArgs& A);
}  // namespace carmel_hip
