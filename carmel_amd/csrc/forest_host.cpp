// forest_host.cpp — the host side of forest-em's forests (include/carmel_hip.h, carmel_hip_forests_*): the handle and
// carmel_hip_forests_create, which flattens the forests into forest.hip's streams and tables; EM (estimate, maximize),
// Viterbi, and the small accessors.  The sampler (carmel_hip_forests_gibbs) is forest_gibbs.cpp; the kernels and their
// launchers are forest.hip / forest.hpp.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <numeric>
#include <unordered_map>
#include "forest_host.hpp"
#include "forest_exact.hpp"  // FX_NODES, FX_KIDS, FX_STACK

using namespace carmel_hip;

namespace carmel_hip {

// side streams: the launch classes of one pass run side by side (each ends with a few slow waves; no class fills the
// chip).  (forest_host.hpp)
static hipError_t ensure_side(carmel_hip_forests* F) {
  return F->ev_fork ? hipSuccess : hipErrorNotInitialized;  // (created with the forests, carmel_hip_forests_create)
}
int n_side_for(const carmel_hip_forests* F) {
  return F->classes.size() < 2 ? 0 : (int)std::min<size_t>(carmel_hip_forests::N_SIDE, F->classes.size() - 1);
}
hipError_t fork_side(carmel_hip_forests* F, hipStream_t s) {
  if (!n_side_for(F)) return hipSuccess;
  hipError_t e = ensure_side(F);
  if (e == hipSuccess) e = hipEventRecord(F->ev_fork, s);
  for (int k = 0; k < n_side_for(F) && e == hipSuccess; ++k) e = hipStreamWaitEvent(F->side[k], F->ev_fork, 0);
  return e;
}
hipStream_t class_stream(carmel_hip_forests* F, hipStream_t s, size_t ci) {
  const int n = n_side_for(F);
  if (!n) return s;
  if (F->class_side.size() != F->classes.size()) {
    // longest class first onto the least loaded stream (load = lane groups x rows of the longest lane: the records a class reads)
    std::vector<size_t> order(F->classes.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    auto cost = [&](size_t i) { return (double)F->classes[i].count * (double)F->classes[i].maxlen; };
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return cost(a) > cost(b); });
    std::vector<double> load((size_t)n + 1, 0.0);
    F->class_side.assign(F->classes.size(), -1);
    for (size_t i : order) {
      const size_t k = (size_t)(std::min_element(load.begin(), load.end()) - load.begin());
      F->class_side[i] = (int)k - 1;
      load[k] += cost(i);
    }
  }
  const int k = F->class_side[ci];
  return k < 0 ? s : F->side[k];
}
// The several-lanes sampler's sweep: every wavefront of every class is resident at once, so a class takes what its LONGEST
// forests take (a wavefront's chain of dependent steps grows with the nodes of its forests), not what its records add up to
// (round 6, tools/c5_timeline.sh: by records the class of the largest forests -- 204 us -- shared a stream with the smallest and
// started 19 us after the first).  Classes by their largest forest, the largest on the caller's stream (it need not wait for
// the fork) and launched first; a stream takes a second class only after every stream has one.
hipStream_t sweep_stream(carmel_hip_forests* F, hipStream_t s, size_t ci) {
  const int n = n_side_for(F);
  if (!n) return s;
  const int k = F->sweep_side[ci];
  return k < 0 ? s : F->side[k];
}
void sweep_schedule(carmel_hip_forests* F) {
  if (F->sweep_order.size() == F->classes.size()) return;
  const int n = n_side_for(F);
  F->sweep_order.resize(F->classes.size());
  for (size_t i = 0; i < F->sweep_order.size(); ++i) F->sweep_order[i] = i;
  auto cost = [&](size_t i) { return (double)std::max(F->classes[i].m_n, F->classes[i].max_nodes); };
  std::stable_sort(F->sweep_order.begin(), F->sweep_order.end(), [&](size_t a, size_t b) { return cost(a) > cost(b); });
  std::vector<double> load((size_t)n + 1, 0.0);
  F->sweep_side.assign(F->classes.size(), -1);
  for (size_t i : F->sweep_order) {
    const size_t k = (size_t)(std::min_element(load.begin(), load.end()) - load.begin());
    F->sweep_side[i] = (int)k - 1;
    load[k] += cost(i);
  }
}
hipError_t join_side(carmel_hip_forests* F, hipStream_t s) {
  hipError_t e = hipSuccess;
  for (int k = 0; k < n_side_for(F) && e == hipSuccess; ++k) {
    e = hipEventRecord(F->ev_side[k], F->side[k]);
    if (e == hipSuccess) e = hipStreamWaitEvent(s, F->ev_side[k], 0);
  }
  return e;
}

void fill_args(carmel_hip_forests* F, ForestArgs& A) {
  std::memset(&A, 0, sizeof A);
  A.groups = F->groups.p;
  A.ins_stream = (const uint2*)F->ins_stream.p;
  A.out_stream = (const uint2*)F->out_stream.p;
  A.lane_forest = F->lane_forest.p;
  A.lane_nodes = F->lane_nodes.p;
  A.rule_logw = F->rule_logw.p;
  A.post = F->post.p;
  A.forest_logprob = F->forest_logprob.p;
  A.scalars = F->scalars.p;
  A.p_norm = F->p_norm.p;
  A.hdr_pos = F->hdr_pos.p;
  A.sample_off = F->sample_off.p;
  A.iter_out = F->iter_out.p;
  A.trace = nullptr;
  A.ghash = nullptr;
  A.serial_forest = 0xffffffffu;
}

}  // namespace carmel_hip

extern "C" {

int carmel_hip_forests_create(carmel_hip_forests** out, int device, uint64_t n_forests, const uint64_t* node_off,
                              const uint32_t* label, const int32_t* ref, const uint32_t* next, uint32_t n_rules,
                              const double* rule_logw, uint64_t n_groups, const uint64_t* group_off,
                              const uint32_t* group_rule) {
  if (!out || !node_off || !label || !ref || !next || !rule_logw) return fail(CARMEL_HIP_ERR_ARG, "null argument");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (ndev <= 0) return fail(CARMEL_HIP_ERR_HIP, "no HIP device: forest-em has no CPU fallback here");
  if (device < 0 || device >= ndev) return fail(CARMEL_HIP_ERR_ARG, "bad device index");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<carmel_hip_forests> F(new carmel_hip_forests());
  F->device = device;
  F->n_forests = n_forests;
  F->n_rules = n_rules;
  F->n_groups = n_groups;
  HIPCHK(hipStreamCreateWithFlags(&F->stream, hipStreamNonBlocking));
  // (the side streams right behind it: four streams created in a row land on four different hardware queues)
  HIPCHK(hipEventCreateWithFlags(&F->ev_fork, hipEventDisableTiming));
  // The side streams belong to the HIGH priority class -- not for the priority: the runtime keeps a pool of hardware queues per
  // priority class (four each), and streams of the default class share theirs with every other stream of the process (torch's,
  // a trainer's): in bench.py's full run two launch classes landed on one queue and ran one after the other, 0.41 ms per sweep
  // against 0.33 on its own.  In a class of their own the three get a queue each: 0.33 in both places.
  {
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    for (int k = 0; k < carmel_hip_forests::N_SIDE; ++k) {
      HIPCHK(hipStreamCreateWithPriority(&F->side[k], hipStreamNonBlocking, prio_hi));
      HIPCHK(hipEventCreateWithFlags(&F->ev_side[k], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&F->ev_samp[k], hipEventDisableTiming));
    }
  }
  hipStream_t s = F->stream;
  // ---- per forest: post-order over non-reference nodes, streams ----
  struct Flat {
    std::vector<uint2_t> ins, outs;
    std::vector<uint32_t> hdr;  // per post-order node: header position in ins
    uint32_t n = 0;
    uint64_t max_deriv = 0;     // rules in the largest derivation (shared sub-forests count once per use)
    std::vector<uint16_t> mt;   // forest_sample_multi_kernel's table block (FMultiArgs::tab); empty: the forest does not fit it
    std::vector<uint32_t> mh;   // ... header row | AND per node
    uint32_t m_front = 0;       // ... entries of its widest breadth-first frontier (bounded by the largest derivation)
    std::vector<uint16_t> m_ord;  // ... its nodes by height: sampler's node id -> node
  };
  std::vector<Flat> flat(n_forests);
  for (uint64_t f = 0; f < n_forests; ++f) {
    const uint64_t b = node_off[f], e = node_off[f + 1];
    const uint32_t N = (uint32_t)(e - b);
    if (!N) return fail(CARMEL_HIP_ERR_ARG, "empty forest");
    std::vector<uint32_t> pi(N, 0xffffffffu), order;
    // post-order = nodes sorted by (end of subtree ascending, start descending); references are skipped
    std::vector<uint32_t> idx;
    for (uint32_t i = 0; i < N; ++i) {
      if (next[b + i] <= i || next[b + i] > N) return fail(CARMEL_HIP_ERR_ARG, "bad forest node extent");
      if (ref[b + i] >= 0) {
        if ((uint32_t)ref[b + i] >= i) return fail(CARMEL_HIP_ERR_ARG, "forest back-reference must point backwards");
        continue;
      }
      if (label[b + i] >= n_rules && label[b + i] != 0) return fail(CARMEL_HIP_ERR_ARG, "rule id out of range");
      idx.push_back(i);
    }
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) {
      if (next[b + x] != next[b + y]) return next[b + x] < next[b + y];
      return x > y;
    });
    for (uint32_t k = 0; k < idx.size(); ++k) pi[idx[k]] = k;
    Flat& fl = flat[f];
    fl.n = (uint32_t)idx.size();
    if (fl.n > F_IDX) return fail(CARMEL_HIP_ERR_UNSUPPORTED, "forest too large");
    auto resolve = [&](uint32_t c) {
      while (ref[b + c] >= 0) c = (uint32_t)ref[b + c];
      return pi[c];
    };
    std::vector<std::vector<uint32_t> > kids(fl.n), kid_ref(fl.n);  // kid_ref: 1 = reached through a back-reference
    for (uint32_t k = 0; k < fl.n; ++k) {
      uint32_t i = idx[k];
      for (uint32_t c = i + 1; c < next[b + i]; c = next[b + c]) {
        kids[k].push_back(resolve(c));
        kid_ref[k].push_back(ref[b + c] >= 0 ? 1u : 0u);
      }
    }
    fl.hdr.resize(fl.n);
    for (uint32_t k = 0; k < fl.n; ++k) {
      uint32_t i = idx[k];
      bool is_and = label[b + i] != 0;
      fl.hdr[k] = (uint32_t)fl.ins.size();
      // header word: flags | child count in bits 20..27 (255 = "255 or more: count the records") | node order k
      uint32_t hx = F_HEADER | F_VALID | (is_and ? F_AND : 0u) | (kids[k].empty() ? F_LAST : 0u) |
                    ((uint32_t)std::min<size_t>(kids[k].size(), 255) << 20) | (k & 0xfffffu);
      fl.ins.push_back(uint2_t{hx, label[b + i]});
      for (size_t c = 0; c < kids[k].size(); ++c)
        fl.ins.push_back(uint2_t{F_VALID | (c + 1 == kids[k].size() ? F_LAST : 0u) | kids[k][c], kid_ref[k][c] << 31});
    }
    // second word of a child record: stream position of the child's header | bit 31 = reached through a back-reference
    for (uint32_t k = 0; k < fl.n; ++k)
      for (size_t c = 0; c < kids[k].size(); ++c) fl.ins[fl.hdr[k] + 1 + c].y |= fl.hdr[kids[k][c]];
    for (uint32_t k = fl.n; k-- > 0;) {
      uint32_t i = idx[k];
      bool is_and = label[b + i] != 0;
      fl.outs.push_back(uint2_t{F_HEADER | F_VALID | (is_and ? F_AND : 0u) | k, label[b + i]});
      for (uint32_t c : kids[k]) fl.outs.push_back(uint2_t{F_VALID | c, 0u});
    }
    if (!(label[b + 0] == 0 || ref[b + 0] < 0)) return fail(CARMEL_HIP_ERR_ARG, "forest root cannot be a reference");
    std::vector<uint64_t> dsz(fl.n, 0);
    for (uint32_t k = 0; k < fl.n; ++k) {
      uint64_t v = 0;
      if (label[b + idx[k]] != 0) {
        v = 1;
        for (uint32_t c : kids[k]) v += dsz[c];
      } else
        for (uint32_t c : kids[k]) v = std::max(v, dsz[c]);
      dsz[k] = std::min<uint64_t>(v, 1u << 20);
    }
    fl.max_deriv = std::max<uint64_t>(1, dsz[fl.n - 1]);
    if (fl.max_deriv >= (1u << 20)) return fail(CARMEL_HIP_ERR_ARG, "forest derivation larger than 2^20 rules");
    {
      // tables of the several-lanes-per-forest sampler: nodes by height (leaves 0; a node is above all of its children,
      // reached directly or through a back-reference), children lists, header rows
      size_t nk = 0;
      for (uint32_t k = 0; k < fl.n; ++k) nk += kids[k].size();
      // the widest frontier a breadth-first walk can reach: w[d][k] = most entries d levels below node k (an AND node hands on
      // all of its children, an OR node the widest of them); depth by depth until nothing is left
      uint64_t front = 1;
      {
        std::vector<uint64_t> w(fl.n, 1), w2(fl.n);
        for (uint32_t depth = 0; depth < 4096; ++depth) {
          bool any = false;
          for (uint32_t k = 0; k < fl.n; ++k) {  // (children have smaller ids: w of the previous depth is complete)
            uint64_t v = 0;
            if (label[b + idx[k]] != 0)
              for (uint32_t c : kids[k]) v += w[c];
            else
              for (uint32_t c : kids[k]) v = std::max(v, w[c]);
            w2[k] = std::min<uint64_t>(v, 1u << 20);
            any = any || v;
          }
          w.swap(w2);
          front = std::max(front, w[fl.n - 1]);
          if (!any) break;
        }
        front += 1;
      }
      if (fl.n < 0x7fffu && nk < 0x7fffu && front < 4096) {
        std::vector<uint32_t> height(fl.n, 0);
        uint32_t Hh = 0;
        for (uint32_t k = 0; k < fl.n; ++k) {  // post-order: children first
          uint32_t hh = 0;
          for (uint32_t c : kids[k]) hh = std::max(hh, height[c] + 1);
          height[k] = hh;
          Hh = std::max(Hh, hh + 1);
        }
        std::vector<uint16_t>& mt = fl.mt;
        mt.assign(4, 0);
        mt[0] = (uint16_t)fl.n;
        mt[1] = (uint16_t)Hh;
        mt[2] = (uint16_t)nk;
        std::vector<uint32_t> cnt(Hh + 1, 0);
        for (uint32_t k = 0; k < fl.n; ++k) cnt[height[k] + 1]++;
        for (uint32_t h = 0; h < Hh; ++h) cnt[h + 1] += cnt[h];
        for (uint32_t h = 0; h <= Hh; ++h) mt.push_back((uint16_t)cnt[h]);
        // the sampler numbers the nodes BY HEIGHT (stable: the root, alone at the top, stays last): the nodes of a height are a
        // range of ids, a node's children have smaller ids
        std::vector<uint16_t>& ordv = fl.m_ord;
        ordv.assign(fl.n, 0);
        std::vector<uint16_t> newid(fl.n);
        {
          std::vector<uint32_t> cur(cnt.begin(), cnt.end() - 1);
          for (uint32_t k = 0; k < fl.n; ++k) {
            newid[k] = (uint16_t)cur[height[k]];
            ordv[cur[height[k]]++] = (uint16_t)k;
          }
        }
        uint32_t off = 0;
        for (uint32_t q = 0; q < fl.n; ++q) {
          mt.push_back((uint16_t)off);
          off += (uint32_t)kids[ordv[q]].size();
        }
        mt.push_back((uint16_t)off);
        for (uint32_t q = 0; q < fl.n; ++q) {
          const uint32_t k = ordv[q];
          for (size_t c = 0; c < kids[k].size(); ++c) mt.push_back((uint16_t)(newid[kids[k][c]] | (kid_ref[k][c] ? 0x8000u : 0u)));
        }
        fl.mh.assign((size_t)4 * fl.n, 0u);  // (class words and norm groups follow once they are known)
        for (uint32_t q = 0; q < fl.n; ++q) fl.mh[4 * q] = fl.hdr[ordv[q]] | (label[b + idx[ordv[q]]] != 0 ? 0x80000000u : 0u);
        fl.m_front = (uint32_t)front;
      }
    }
  }
  // ---- groups of 64, sorted by stream length ----
  std::vector<uint32_t> ord(n_forests);
  std::iota(ord.begin(), ord.end(), 0u);
  std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b2) { return flat[a].ins.size() > flat[b2].ins.size(); });
  const size_t ng = (n_forests + 63) / 64;
  F->h_groups.resize(ng);
  std::vector<uint32_t> lane_forest(ng * 64, 0xffffffffu), lane_nodes(ng * 64, 0);
  F->lane_of_forest.assign(n_forests, 0);
  uint64_t base = 0, node_total = 0;
  for (size_t gidx = 0; gidx < ng; ++gidx) {
    FGroup& G = F->h_groups[gidx];
    std::memset(&G, 0, sizeof G);
    size_t l0 = gidx * 64, l1 = std::min<size_t>(n_forests, l0 + 64);
    G.stream_base = base;
    G.n_lanes = (uint32_t)(l1 - l0);
    G.lane_base = (uint32_t)l0;
    for (size_t l = l0; l < l1; ++l) {
      const Flat& fl = flat[ord[l]];
      G.maxlen = std::max<uint32_t>(G.maxlen, (uint32_t)fl.ins.size());
      G.max_nodes = std::max(G.max_nodes, fl.n);
      lane_forest[l] = ord[l];
      lane_nodes[l] = fl.n;
      F->lane_of_forest[ord[l]] = (uint32_t)l;
    }
    F->max_nodes = std::max(F->max_nodes, G.max_nodes);
    G.node_base = node_total;
    node_total += (uint64_t)G.max_nodes * 64;
    base += (uint64_t)G.maxlen * 64;
  }
  F->node_total = node_total;
  F->stream_total = base;
  std::vector<uint2_t> si(base, uint2_t{0, 0}), so(base, uint2_t{0, 0});
  std::vector<uint32_t> hp(base, 0);
  for (size_t gidx = 0; gidx < ng; ++gidx) {
    const FGroup& G = F->h_groups[gidx];
    for (uint32_t l = 0; l < G.n_lanes; ++l) {
      const Flat& fl = flat[ord[G.lane_base + l]];
      for (size_t k = 0; k < fl.ins.size(); ++k) si[G.stream_base + k * 64 + l] = fl.ins[k];
      for (size_t k = 0; k < fl.outs.size(); ++k) so[G.stream_base + k * 64 + l] = fl.outs[k];
      for (uint32_t k = 0; k < fl.n; ++k) hp[G.stream_base + (size_t)k * 64 + l] = fl.hdr[k];
    }
  }
  {  // launch classes by LDS need: a class ends where the groups have shrunk to 2/3 of its largest, 256 groups at least.
     // Finer classes (4/5, 64 groups: eleven for config 5) pad less LDS but were slower, 0.96 against 0.79 ms per sweep: only
     // four or five kernels run side by side, the rest queue behind them
    const unsigned cls_num = 2, cls_den = 3, cls_min = 256;
    size_t i = 0;
    while (i < ng) {
      uint32_t mx = F->h_groups[i].max_nodes;
      size_t j = i + 1;
      while (j < ng) {
        uint32_t m = F->h_groups[j].max_nodes;
        if (m > mx) mx = m;
        if (j - i >= cls_min && (uint64_t)m * cls_den <= (uint64_t)mx * cls_num) break;
        ++j;
      }
      carmel_hip_forests::Cls c{(uint32_t)i, (uint32_t)(j - i), mx};
      for (size_t q = i; q < j; ++q) {
        const FGroup& G = F->h_groups[q];
        c.maxlen = std::max(c.maxlen, G.maxlen);
        for (uint32_t l = 0; l < G.n_lanes; ++l) {
          const Flat& fl = flat[ord[G.lane_base + l]];
          c.max_kids = std::max<uint32_t>(c.max_kids, (uint32_t)(fl.ins.size() - fl.n));
          c.m_tab = std::max<uint32_t>(c.m_tab, (uint32_t)((fl.mt.size() + 7) / 8 * 8));  // (copied 16 bytes at a time)
          c.m_n = std::max(c.m_n, fl.n);
          c.m_front = std::max(c.m_front, fl.m_front);
        }
      }
      F->classes.push_back(c);
      i = j;
    }
    if (lib_opt("timing"))
      for (const auto& c : F->classes)
        fprintf(stderr, "timing:   forest class first=%u count=%u max_nodes=%u estep=%s\n", c.first, c.count, c.max_nodes,
                forest_estep_kind_name(forest_estep_kind(c.max_nodes)));
  }
  {  // classes too large for LDS keep their columns in global memory
    uint64_t tot = 0;
    for (auto& c : F->classes) {
      F->gcol_off.push_back(tot);
      if (forest_cols_exceed_lds(c.max_nodes) || lib_opt("forest_gcol")) tot += (uint64_t)c.count * 2 * c.max_nodes * 64;
    }
    if (tot) HIPCHK(F->gcol.alloc(tot));
  }
  // ---- posterior slots grouped by rule (AND headers of the outside stream) ----
  std::vector<uint64_t> cnt((size_t)n_rules + 1, 0);
  for (uint64_t k = 0; k < base; ++k)
    if ((so[k].x & (F_VALID | F_HEADER | F_AND)) == (F_VALID | F_HEADER | F_AND)) cnt[so[k].y + 1]++;
  for (uint32_t r = 0; r < n_rules; ++r) cnt[r + 1] += cnt[r];
  std::vector<uint64_t> arc_off = cnt, slot_pos(cnt[n_rules]), hot;
  for (uint64_t k = 0; k < base; ++k)
    if ((so[k].x & (F_VALID | F_HEADER | F_AND)) == (F_VALID | F_HEADER | F_AND)) slot_pos[cnt[so[k].y]++] = k;
  for (uint32_t r = 0; r < n_rules; ++r)
    if (arc_off[r + 1] - arc_off[r] > 64)
      for (uint64_t j = arc_off[r]; j < arc_off[r + 1]; j += 4096) {
        hot.push_back(r);
        hot.push_back(j);
        hot.push_back(std::min(arc_off[r + 1], j + 4096));
      }
  // ---- normalisation groups ----
  F->h_norm.assign(n_rules, F_NONORM);
  F->h_group_off.assign(group_off, group_off + n_groups + 1);
  F->h_group_rule.assign(group_rule, group_rule + group_off[n_groups]);
  for (uint64_t gi = 0; gi < n_groups; ++gi)
    for (uint64_t j = group_off[gi]; j < group_off[gi + 1]; ++j) {
      if (group_rule[j] >= n_rules) return fail(CARMEL_HIP_ERR_ARG, "normalization group rule id out of range");
      if (F->h_norm[group_rule[j]] != F_NONORM)
        return fail(CARMEL_HIP_ERR_ARG, "a rule occurs in more than one normalization group");
      F->h_norm[group_rule[j]] = (uint32_t)gi;
    }
  // classes of equal rules / equal norm groups within a forest, per AND header record (the parallel sweep's
  // counterfactual counts are kept per class: forest_proposal_kernel)
  std::vector<uint32_t> rc_all(base, 0);
  {
    std::vector<uint32_t>& rc = rc_all;
    F->sweep2_ok = F->max_nodes <= 0xffffu;
    std::unordered_map<uint32_t, uint32_t> rid, gid;
    for (size_t gidx = 0; gidx < ng && F->sweep2_ok; ++gidx) {
      const FGroup& G = F->h_groups[gidx];
      for (uint32_t l = 0; l < G.n_lanes; ++l) {
        const Flat& fl = flat[ord[G.lane_base + l]];
        rid.clear();
        gid.clear();
        for (uint32_t k = 0; k < fl.n; ++k) {
          const uint2_t hr = fl.ins[fl.hdr[k]];
          if (!(hr.x & F_AND)) continue;
          const uint32_t a = rid.emplace(hr.y, (uint32_t)rid.size()).first->second;
          const uint32_t nn = F->h_norm[hr.y];
          const uint32_t b2 = nn == F_NONORM ? 0u : gid.emplace(nn, (uint32_t)gid.size()).first->second;
          rc[G.stream_base + (size_t)fl.hdr[k] * 64 + l] = a | (b2 << 16);
        }
      }
    }
    if (F->sweep2_ok) {
      HIPCHK(F->rec_cls.upload(rc, s));
      std::vector<FAnd> al;  // forest after forest: the threads of a wave scan the same forest's previous sample
      for (size_t gidx = 0; gidx < ng; ++gidx) {
        const FGroup& G = F->h_groups[gidx];
        for (uint32_t l = 0; l < G.n_lanes; ++l)
          for (uint32_t k = 0; k < G.maxlen; ++k) {
            const uint64_t q = G.stream_base + (uint64_t)k * 64 + l;
            const uint2_t r = si[q];
            if ((r.x & (F_VALID | F_HEADER | F_AND)) == (F_VALID | F_HEADER | F_AND))
              al.push_back(FAnd{q, (uint32_t)gidx, rc[q], r.y, lane_forest[G.lane_base + l]});
          }
      }
      F->n_and = al.size();
      HIPCHK(F->and_list.upload(al, s));
    }
    HIPCHK(F->lane_of_forest_d.upload(F->lane_of_forest, s));
  }
  {  // the several-lanes-per-forest tables, in lane-slot order (a wavefront's forests are neighbours)
    F->multi_ok = F->sweep2_ok;
    for (uint64_t f = 0; f < n_forests; ++f)
      if (flat[f].mt.empty()) F->multi_ok = false;
    if (F->multi_ok) {
      std::vector<uint64_t> toff(ng * 64, 0), hoff(ng * 64, 0);
      std::vector<uint32_t> slots(ng * 64 * 8, 0u);
      for (size_t l = 0; l < ng * 64; ++l) slots[8 * l + 6] = 0xffffffffu;
      // (the samples' offsets: capacity = size of the largest derivation of the forest, as below)
      std::vector<uint64_t> so_all(n_forests + 1, 0);
      for (uint64_t f = 0; f < n_forests; ++f) so_all[f + 1] = so_all[f] + flat[f].max_deriv + 2;
      auto F_sample_off_of = [&](uint32_t f) { return so_all[f]; };
      std::vector<uint16_t> tab;
      std::vector<uint32_t> hdrs;
      for (size_t l = 0; l < ng * 64; ++l) {
        if (lane_forest[l] == 0xffffffffu) continue;
        const Flat& fl = flat[lane_forest[l]];
        toff[l] = tab.size();
        hoff[l] = hdrs.size();
        tab.insert(tab.end(), fl.mt.begin(), fl.mt.end());
        tab.resize((tab.size() + 7) / 8 * 8, 0);  // (copied 16 bytes at a time)
        {
          const uint64_t so = F_sample_off_of(lane_forest[l]);
          uint32_t* d = &slots[8 * l];
          d[0] = (uint32_t)toff[l];
          d[1] = (uint32_t)(toff[l] >> 32);
          d[2] = (uint32_t)hoff[l];
          d[3] = (uint32_t)(hoff[l] >> 32);
          d[4] = (uint32_t)so;
          d[5] = (uint32_t)(so >> 32);
          d[6] = lane_forest[l];
          d[7] = fl.n | ((uint32_t)fl.mt.size() << 15);
        }
        hdrs.insert(hdrs.end(), fl.mh.begin(), fl.mh.end());
        const FGroup& G = F->h_groups[l / 64];
        for (uint32_t q = 0; q < fl.n; ++q) {  // rule, class word (rec_cls) and norm group of the node's header record
          const uint32_t k = fl.m_ord[q];
          const uint2_t hr = fl.ins[fl.hdr[k]];
          if (!(hr.x & F_AND)) continue;
          uint32_t* w = &hdrs[hoff[l] + 4 * (size_t)q];
          w[1] = hr.y;
          w[2] = rc_all[G.stream_base + (size_t)fl.hdr[k] * 64 + (l % 64)];
          w[3] = F->h_norm[hr.y];
        }
      }
      HIPCHK(F->mt_tab.upload(tab, s));
      HIPCHK(F->mt_hdr.upload(hdrs, s));
      HIPCHK(F->mt_slots.upload(slots, s));
      if (hdrs.size() / 4 < 0xffffffffull) {  // rule -> the AND nodes that carry it (rules inside a normalisation group: the counted ones)
        const size_t nn_ = hdrs.size() / 4;
        std::vector<uint32_t> ioff((size_t)n_rules + 1, 0u);
        for (size_t q = 0; q < nn_; ++q)
          if ((hdrs[4 * q] & 0x80000000u) && hdrs[4 * q + 3] != F_NONORM) ioff[(size_t)hdrs[4 * q + 1] + 1]++;
        for (uint32_t r = 0; r < n_rules; ++r) ioff[r + 1] += ioff[r];
        std::vector<uint32_t> inode(ioff[n_rules]), fill(ioff.begin(), ioff.end() - 1), pieces;
        for (size_t q = 0; q < nn_; ++q)
          if ((hdrs[4 * q] & 0x80000000u) && hdrs[4 * q + 3] != F_NONORM) inode[fill[hdrs[4 * q + 1]]++] = (uint32_t)q;
        for (uint32_t r = 0; r < n_rules; ++r)
          if (ioff[r + 1] - ioff[r] > FRG_COLD)
            for (uint32_t j = ioff[r]; j < ioff[r + 1]; j += FRG_PIECE) {
              pieces.push_back(r);
              pieces.push_back(j);
              pieces.push_back(std::min(ioff[r + 1], j + FRG_PIECE));
            }
        F->n_inv_pieces = (uint32_t)(pieces.size() / 3);
        if (pieces.empty()) pieces.assign(3, 0u);
        if (inode.empty()) inode.assign(1, 0u);
        HIPCHK(F->inv_off.upload(ioff, s));
        HIPCHK(F->inv_node.upload(inode, s));
        HIPCHK(F->inv_pieces.upload(pieces, s));
        HIPCHK(F->mt_node_cnt.alloc(nn_ + 8));
        HIPCHK(hipMemsetAsync(F->mt_node_cnt.p, 0, (nn_ + 8) * sizeof(uint16_t), s));
        HIPCHK(F->rule_cnt.alloc((size_t)n_rules + 1));
        HIPCHK(hipMemsetAsync(F->rule_cnt.p, 0, ((size_t)n_rules + 1) * sizeof(uint32_t), s));
      }
      // the exact chain's records (forest_exact.hip), forest after forest in the order of the chain: per node its children,
      // rule, norm group, height; per forest where they start, how many, how high, where its sample lives, and whether it
      // fits the register path (FX_NODES nodes, FX_KIDS children a node, FX_STACK pending nodes, FX_NODES rules a derivation)
      {
        std::vector<uint32_t> xd(4 * (size_t)n_forests), xr, xm;
        std::vector<uint32_t> need;
        for (uint64_t f = 0; f < n_forests; ++f) {
          const Flat& fl = flat[f];
          const uint16_t* mt = fl.mt.data();
          const uint32_t n = mt[0], H = mt[1];
          const uint16_t* lvl = mt + 4;
          const uint16_t* koff = lvl + H + 1;
          const uint16_t* kids = koff + n + 1;
          bool slow = n > FX_NODES || fl.max_deriv > FX_NODES;
          const uint64_t first = xm.size();
          need.assign(n, 0);
          for (uint32_t h = 0; h < H; ++h)
            for (uint32_t q = lvl[h]; q < lvl[h + 1]; ++q) {
              const uint32_t nch = (uint32_t)koff[q + 1] - koff[q];
              const bool is_and = (fl.mh[4 * (size_t)q] & 0x80000000u) != 0;
              if (nch > FX_KIDS) slow = true;
              uint32_t kid[4] = {0xffu, 0xffu, 0xffu, 0xffu}, nd = 0;
              for (uint32_t c = 0; c < nch; ++c) {
                const uint32_t id = kids[koff[q] + c] & 0x7fffu;
                if (c < 4) kid[c] = id & 0xffu;  // (ids beyond a byte: a forest of the LDS path, which reads other tables)
                nd = std::max(nd, is_and ? (nch - 1 - c) + need[id] : need[id]);
              }
              need[q] = std::min(nd, 1u << 20);
              const uint2_t hrw = fl.ins[fl.hdr[fl.m_ord[q]]];
              const uint32_t rule = is_and ? hrw.y : 0u;
              xr.push_back(kid[0] | (std::min(nch, 255u) << 8) | (std::min(h, 0x7fffu) << 16) | (is_and ? 0x80000000u : 0u));
              xr.push_back(kid[1] | (kid[2] << 8) | (kid[3] << 16));
              xr.push_back(rule);
              xr.push_back(is_and ? F->h_norm[rule] : F_NONORM);
              xm.push_back(0);
            }
          if (need[n - 1] > FX_STACK) slow = true;
          if (first > 0xffffffffull || (so_all[f] >> 48)) return fail(CARMEL_HIP_ERR_UNSUPPORTED, "forests too large for the exact sampler's tables");
          uint32_t* d = &xd[4 * (size_t)f];
          d[0] = (uint32_t)first;
          d[1] = n | (H << 16);
          d[2] = (uint32_t)so_all[f];
          // (bit 17: a derivation of more than 64 rules -- shared sub-forests count once per use, so 64 NODES can yield more --:
          // the register path keeps a sample entry per lane and register, such a forest takes two registers whatever its size)
          d[3] = (uint32_t)(so_all[f] >> 32) | (slow ? 0x10000u : 0u) | (fl.max_deriv > 64 ? 0x20000u : 0u);
        }
        HIPCHK(F->x_desc.upload(xd, s));
        HIPCHK(F->x_rec.upload(xr, s));
      }
      HIPCHK(hipStreamSynchronize(s));
    }
  }
  // samples: capacity = size of the largest derivation of the forest
  F->h_sample_off.assign(n_forests + 1, 0);
  for (uint64_t f = 0; f < n_forests; ++f) {
    F->h_sample_off[f + 1] = F->h_sample_off[f] + flat[f].max_deriv + 2;
    F->max_sample = std::max<uint32_t>(F->max_sample, (uint32_t)flat[f].max_deriv);
  }
  HIPCHK(F->groups.upload(F->h_groups, s));
  HIPCHK(F->ins_stream.upload(si, s));
  HIPCHK(F->out_stream.upload(so, s));
  HIPCHK(F->hdr_pos.upload(hp, s));
  HIPCHK(F->lane_forest.upload(lane_forest, s));
  HIPCHK(F->lane_nodes.upload(lane_nodes, s));
  HIPCHK(F->rule_logw.upload(std::vector<double>(rule_logw, rule_logw + n_rules), s));
  HIPCHK(F->counts.alloc(n_rules));
  HIPCHK(F->post.alloc(base));
  HIPCHK(F->forest_logprob.alloc(n_forests));
  HIPCHK(F->scalars.alloc(4));
  HIPCHK(F->arc_off.upload(arc_off, s));
  HIPCHK(F->slot_pos.upload(slot_pos, s));
  HIPCHK(F->hot_chunks.upload(hot, s));
  HIPCHK(F->group_off.upload(F->h_group_off, s));
  HIPCHK(F->group_rule.upload(F->h_group_rule, s));
  HIPCHK(F->p_norm.upload(F->h_norm, s));
  HIPCHK(F->sample_off.upload(F->h_sample_off, s));
  HIPCHK(F->maxbits.alloc(1));
  HIPCHK(F->iter_out.alloc(2));
  HIPCHK(hipStreamSynchronize(s));
  *out = F.release();
  return CARMEL_HIP_OK;
}

int carmel_hip_forests_destroy(carmel_hip_forests* F) {
  if (F) {
    (void)hipSetDevice(F->device);
    (void)hipDeviceSynchronize();
    hipStream_t s = F->stream;
    for (int k = 0; k < carmel_hip_forests::N_SIDE; ++k) {
      if (F->side[k]) (void)hipStreamDestroy(F->side[k]);
      if (F->ev_side[k]) (void)hipEventDestroy(F->ev_side[k]);
      if (F->ev_samp[k]) (void)hipEventDestroy(F->ev_samp[k]);
    }
    if (F->ev_fork) (void)hipEventDestroy(F->ev_fork);
    delete F;
    if (s) (void)hipStreamDestroy(s);
  }
  return CARMEL_HIP_OK;
}

// FForests::estimate (forest-em.hpp:561-578): counts = prior_count * n_forests + expected rule counts;
// returns the average log probability over the forests with non-zero probability
int carmel_hip_forests_estimate(carmel_hip_forests* F, double prior_count, double* avg_logprob, uint64_t* n_zero,
                                double* per_forest_logprob) {
  if (!F) return fail(CARMEL_HIP_ERR_ARG, "null handle");
  HIPCHK(hipSetDevice(F->device));
  hipStream_t s = F->stream;
  ForestArgs A;
  fill_args(F, A);
  HIPCHK(hipMemsetAsync(F->scalars.p, 0, 4 * sizeof(double), s));
  HIPCHK(fork_side(F, s));
  // mantissa / exponent arithmetic where the columns fit LDS at 12 bytes per value (otherwise: the log domain)
  for (size_t ci = 0; ci < F->classes.size(); ++ci) {
    const auto& c = F->classes[ci];
    A.first_group = c.first;
    const FEstepKind kind = forest_estep_kind(c.max_nodes);
    if (kind == F_ESTEP_GCOL) {
      A.gcol = F->gcol.p + F->gcol_off[ci];
      A.gcol_stride = (uint64_t)2 * c.max_nodes * 64;
    }
    if (kind == F_ESTEP_EXT)
      HIPCHK(launch_forest_estimate_ext(A, c.count, c.max_nodes, class_stream(F, s, ci)));
    else
      HIPCHK(launch_forest_estimate(A, kind == F_ESTEP_GCOL, c.count, c.max_nodes, class_stream(F, s, ci)));
  }
  HIPCHK(join_side(F, s));
  ReduceArgs R;
  R.arc_off = F->arc_off.p;
  R.slot_pos = F->slot_pos.p;
  R.hot_chunks = F->hot_chunks.p;
  R.post = F->post.p;
  R.counts = F->counts.p;
  R.n_arcs = F->n_rules;
  R.n_hot_chunks = F->hot_chunks.n / 3;
  HIPCHK(launch_count_reduce(R, s));
  double sc[4];
  HIPCHK(hipMemcpyAsync(sc, F->scalars.p, sizeof sc, hipMemcpyDeviceToHost, s));
  if (per_forest_logprob)
    HIPCHK(hipMemcpyAsync(per_forest_logprob, F->forest_logprob.p, F->n_forests * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  (void)prior_count;  // folded in at maximize / get_counts (it is a constant added to every count)
  if (avg_logprob) *avg_logprob = sc[1] > 0 ? sc[0] / sc[1] : -std::numeric_limits<double>::infinity();
  if (n_zero) *n_zero = (uint64_t)(sc[2] + 0.5);
  return CARMEL_HIP_OK;
}

int carmel_hip_forests_get_counts(carmel_hip_forests* F, double prior_count, double* counts) {
  if (!F || !counts) return fail(CARMEL_HIP_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(F->device));
  HIPCHK(hipMemcpyAsync(counts, F->counts.p, F->n_rules * sizeof(double), hipMemcpyDeviceToHost, F->stream));
  HIPCHK(hipStreamSynchronize(F->stream));
  const double wp = prior_count * (double)F->n_forests;
  for (uint32_t r = 0; r < F->n_rules; ++r) counts[r] += wp;
  return CARMEL_HIP_OK;
}

// FForests::maximize (forest-em.hpp:626-655) -> NormalizeGroups (normalize.hpp:123-164)
int carmel_hip_forests_maximize(carmel_hip_forests* F, double prior_count, double add_k, int zero_zerocounts,
                                double* max_delta) {
  if (!F) return fail(CARMEL_HIP_ERR_ARG, "null handle");
  HIPCHK(hipSetDevice(F->device));
  hipStream_t s = F->stream;
  HIPCHK(hipMemsetAsync(F->maxbits.p, 0, sizeof(unsigned long long), s));
  if (F->n_groups)
    HIPCHK(launch_forest_mstep(F->rule_logw.p, F->counts.p, prior_count * (double)F->n_forests, F->group_off.p, F->group_rule.p,
                               F->n_groups, add_k, zero_zerocounts, F->maxbits.p, s));
  unsigned long long bits = 0;
  HIPCHK(hipMemcpyAsync(&bits, F->maxbits.p, sizeof bits, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  double d;
  std::memcpy(&d, &bits, sizeof d);
  if (max_delta) *max_delta = d;
  return CARMEL_HIP_OK;
}

int carmel_hip_forests_get_weights(carmel_hip_forests* F, double* rule_logw) {
  if (!F || !rule_logw) return fail(CARMEL_HIP_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(F->device));
  HIPCHK(hipMemcpyAsync(rule_logw, F->rule_logw.p, F->n_rules * sizeof(double), hipMemcpyDeviceToHost, F->stream));
  HIPCHK(hipStreamSynchronize(F->stream));
  return CARMEL_HIP_OK;
}
int carmel_hip_forests_set_weights(carmel_hip_forests* F, const double* rule_logw) {
  if (!F || !rule_logw) return fail(CARMEL_HIP_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(F->device));
  HIPCHK(hipMemcpyAsync(F->rule_logw.p, rule_logw, F->n_rules * sizeof(double), hipMemcpyHostToDevice, F->stream));
  HIPCHK(hipStreamSynchronize(F->stream));
  return CARMEL_HIP_OK;
}

uint32_t carmel_hip_forests_best_run(carmel_hip_forests* F) { return F ? F->best_run : 0; }
int carmel_hip_forests_final_counts(carmel_hip_forests* F, double* x) {
  if (!F || !x) return fail(CARMEL_HIP_ERR_ARG, "null argument");
  if (F->h_final_x.size() != F->n_rules) return fail(CARMEL_HIP_ERR_STATE, "carmel_hip_forests_final_counts: run the sampler first");
  std::memcpy(x, F->h_final_x.data(), F->h_final_x.size() * sizeof(double));
  return CARMEL_HIP_OK;
}
int carmel_hip_forests_set_prior_inference(carmel_hip_forests* F, double stddev, int global, int local, uint32_t start,
                                           uint32_t end) {
  if (!F) return fail(CARMEL_HIP_ERR_ARG, "null handle");
  F->pi_stddev = stddev;
  F->pi_global = global != 0;
  F->pi_local = local != 0;
  F->pi_start = start;
  F->pi_end = end;
  return CARMEL_HIP_OK;
}
int carmel_hip_forests_prior_trace(carmel_hip_forests* F, double* out6, uint32_t n_sweeps, double* cumulative, uint32_t n_cumulative,
                                   uint32_t* n_scales) {
  if (!F) return fail(CARMEL_HIP_ERR_ARG, "null handle");
  if (out6)
    for (size_t k = 0; k < (size_t)n_sweeps * 6; ++k) out6[k] = k < F->pi_trace.size() ? F->pi_trace[k] : 0.0;
  if (cumulative)
    for (uint32_t k = 0; k < n_cumulative; ++k) cumulative[k] = k < F->pi_cumulative.size() ? F->pi_cumulative[k] : 1.0;
  if (n_scales) *n_scales = (uint32_t)F->pi_cumulative.size();
  return CARMEL_HIP_OK;
}

int carmel_hip_forests_set_alphas(carmel_hip_forests* F, const double* alpha_per_rule, uint32_t n) {
  if (!F) return fail(CARMEL_HIP_ERR_ARG, "null handle");
  if (alpha_per_rule && n)
    F->h_alphas.assign(alpha_per_rule, alpha_per_rule + n);
  else
    F->h_alphas.clear();
  return CARMEL_HIP_OK;
}

int carmel_hip_forests_get_sample(carmel_hip_forests* F, uint64_t forest, uint32_t* rules, uint32_t* n) {
  if (!F || !n || forest >= F->n_forests) return fail(CARMEL_HIP_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(F->device));
  uint32_t len = 0;
  HIPCHK(hipMemcpyAsync(&len, F->sample_len[0].p + forest, sizeof len, hipMemcpyDeviceToHost, F->stream));
  HIPCHK(hipStreamSynchronize(F->stream));
  if (rules && len)
    HIPCHK(hipMemcpyAsync(rules, F->sample_rules[0].p + F->h_sample_off[forest], len * 4, hipMemcpyDeviceToHost, F->stream));
  HIPCHK(hipStreamSynchronize(F->stream));
  *n = len;
  return CARMEL_HIP_OK;
}
uint32_t carmel_hip_forests_max_sample(carmel_hip_forests* F) { return F ? F->max_sample : 0; }

// Replaces FForest::compute_viterbi + write_viterbi's walk (forest.hpp:507-632) for every forest, with the current weights.
int carmel_hip_forests_viterbi(carmel_hip_forests* F, double* best_logprob) {
  if (!F || !best_logprob) return fail(CARMEL_HIP_ERR_ARG, "null argument");
  HIPCHK(hipSetDevice(F->device));
  hipStream_t s = F->stream;
  const uint64_t nf = F->n_forests;
  if (!F->sample_len[0].n) HIPCHK(F->sample_len[0].alloc(nf));
  if (!F->sample_rules[0].n) HIPCHK(F->sample_rules[0].alloc(F->h_sample_off.back()));
  if (!F->sample_hdr.n) HIPCHK(F->sample_hdr.alloc(F->h_sample_off.back()));
  DevBuf<double> best;
  HIPCHK(best.alloc(nf));
  ForestArgs A;
  fill_args(F, A);
  A.sample_len = F->sample_len[0].p;
  A.sample_rules = F->sample_rules[0].p;
  A.sample_hdr = F->sample_hdr.p;
  const uint32_t stack_lds = 32u;
  HIPCHK(fork_side(F, s));
  for (size_t ci = 0; ci < F->classes.size(); ++ci) {
    const auto& c = F->classes[ci];
    A.first_group = c.first;
    const bool gcol = forest_cols_exceed_lds(c.max_nodes);
    if (gcol) {  // (the class has room for two columns per group in gcol: the E-step's)
      A.gcol = F->gcol.p + F->gcol_off[ci];
      A.gcol_stride = (uint64_t)2 * c.max_nodes * 64;
    }
    HIPCHK(launch_forest_viterbi(A, gcol, c.count, F->max_sample, c.max_nodes, stack_lds, best.p, class_stream(F, s, ci)));
  }
  HIPCHK(join_side(F, s));
  HIPCHK(hipMemcpyAsync(best_logprob, best.p, nf * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return CARMEL_HIP_OK;
}

int carmel_hip_forests_get_viterbi(carmel_hip_forests* F, uint64_t forest, uint32_t* rules, uint32_t* arity, uint32_t* n) {
  if (!F || !n || forest >= F->n_forests || !F->sample_hdr.n || !F->sample_len[0].n)
    return fail(CARMEL_HIP_ERR_ARG, "bad argument (carmel_hip_forests_viterbi first)");
  HIPCHK(hipSetDevice(F->device));
  uint32_t len = 0;
  HIPCHK(hipMemcpyAsync(&len, F->sample_len[0].p + forest, sizeof len, hipMemcpyDeviceToHost, F->stream));
  HIPCHK(hipStreamSynchronize(F->stream));
  if (rules && arity && len) {
    HIPCHK(hipMemcpyAsync(rules, F->sample_rules[0].p + F->h_sample_off[forest], len * 4, hipMemcpyDeviceToHost, F->stream));
    HIPCHK(hipMemcpyAsync(arity, F->sample_hdr.p + F->h_sample_off[forest], len * 4, hipMemcpyDeviceToHost, F->stream));
  }
  HIPCHK(hipStreamSynchronize(F->stream));
  *n = len;
  return CARMEL_HIP_OK;
}


}  // extern "C"
