// decode_prune.hip — pruning the whole machine by best-path weight (carmel -w w, -z n, -p w on the composed result:
// WFST::prunePaths, fst.cc:382-466; WFST::pruneArcs, fst.cc:20-22; carmel.cc:533, 633-636, 951-956, 979).  The best distance from
// the start to every state and from every state to the final state, over the whole, possibly cyclic, machine; then one pass over
// the states and one over the arcs.  The distances are decode_best_paths.hip's relaxation at K = 1, without its K dimension.
//
// The rule (DESIGN.md and include/carmel_hip.h state it in the same words; tests/prune_ref.py restates it).
// Inputs.  log_ratio >= 0, or +inf for no ratio test; max_states >= 1, or UINT32_MAX for no cap; min_arc_logw, or -inf for no arc
//   threshold.
// Arcs.  An arc exists if its log weight is > -inf and >= min_arc_logw.  Symbols play no part.
// Forward distance F[q].  Exactly list(q) of carmel_hip_decoder_best_paths at K = 1 on the existing arcs: an entry is (value,
//   length, last arc); the value is the arcs' logs added in path order from 0.0; ties go to the smaller length, then to the lower
//   arc id; the empty path at state 0 comes first; Jacobi rounds to the first fixed point; an unreachable state has -inf.
// Backward distance R[q].  The same computation on the reversed machine, started at the final state: every existing arc is turned
//   round.  The value is then w1 + (w2 + (... + (wn + 0))), because floating-point addition commutes: the decoders' "reported"
//   fold.  The tie order is the same.
// Through values.  T(q) = F[q] + R[q]; T(a) = (F[src a] + w(a)) + R[dst a]; either is -inf when a term is -inf.
// Limit.  limit = F[final] - log_ratio; it is -inf when log_ratio = +inf.
// Best path P*.  The path the K = 1 back-pointers give from the final state.  Its arcs and states pass the ratio test by
//   definition: rounding may put T(a) of one of P*'s own arcs an ulp below F[final], and a ratio of 1 must keep the best path.
//   (The reference has this hazard in float and asserts it away only in debug builds.)
// State cap.  The states are ordered by T(q) descending, then by state id ascending; states of rank >= max_states are removed.
//   P* is not exempt from the cap.
// State kept iff its rank is < max_states and (T(q) >= limit or q is on P*).
// Arc kept iff it exists, its source and destination are kept, and (T(a) >= limit or the arc is on P*).
// No path or lost endpoint.  F[final] = -inf, or state 0 or the final state not kept: nothing is kept; the call succeeds with
//   counts 0.
// Refused.  An existing arc of log weight > 0 on a cycle: CARMEL_HIP_ERR_UNSUPPORTED, the same arc and the same message form as
//   carmel_hip_decoder_best_paths.
// Deviations from the reference: it has no P* exemption; the order for the cap is total, where it uses an unstable std::sort;
//   arcs of weight 0 are never kept; positive-weight cycles are refused.
//
// The kernels.
//   1. The distance pass takes BestPathsTables and a start state: for F the tables of (src, dst, w'), for R those of (dst, src,
//      w'), w' being the weights with the arcs that do not exist at -inf.  An entry per state in A (committed) and B (proposed), a
//      length of kNone standing for "no entry".  Per round: select over the active states (a plain argmax under the tie order; a
//      state per lane up to the option "best_paths_wave_degree" in-arcs, a wavefront per state above it with a shuffle argmax:
//      the same bytes), commit over the changed states (B to A, the successors marked), compact (the marks become the next
//      worklists).  The two passes share nothing, so their rounds are queued on the handle's one stream side by side and the host
//      reads both passes' counters in one copy a round.  More than |Q| + 1 rounds of either: CARMEL_HIP_ERR_STATE.
//   2. The walk-back: one lane follows F's back-pointers from the final state, bounded by F's length, and marks P*.
//   3. The ranking, only when max_states < |Q|: a radix sort of (T(q) as a u64 that sorts descending, state id); it is stable and
//      the ids go in ascending, so equal keys stay in state order.
//   4. The mark passes: one over the states, one over the arcs in arc-id order, bytes of 0 / 1 and two counters.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "decode.hpp"
#include "engine.hpp"

namespace {
constexpr uint32_t kWaveDegree = 32;  // decode_best_paths.hip's default of the same option
constexpr double kNegInf = -std::numeric_limits<double>::infinity();

struct PrEntry {
  double* val;    // [|Q|]; -inf: no entry
  uint32_t* len;  // kNone: no entry
  uint32_t* arc;  // the arc id; kNone: the empty path (or no entry)
};

struct PrPass {
  uint32_t n_states, start, wave_degree;
  PrEntry A, B;
  uint8_t* mark;        // [|Q|]
  uint32_t* lane_list;  // [|Q|] each
  uint32_t* wave_list;
  uint32_t* changed;
  uint32_t* counts;     // the lengths of lane_list, wave_list and changed
};

// candidate 1 comes before candidate 2 (p: the position in the in-arc table, which stands for the arc id; kNone: no candidate)
__device__ inline bool pr_before(double v1, uint32_t l1, uint32_t p1, double v2, uint32_t l2, uint32_t p2) {
  if (p1 == kNone) return false;
  if (p2 == kNone) return true;
  if (v1 != v2) return v1 > v2;
  if (l1 != l2) return l1 < l2;
  return p1 < p2;
}

// the best candidate of in-arcs p0, p0 + step, ... below p1
__device__ inline void pr_scan(const BestPathsTables& T, const PrPass& R, uint32_t p0, uint32_t p1, uint32_t step, double& bv,
                               uint32_t& bl, uint32_t& bp) {
  bp = kNone;
  bv = 0.0;
  bl = 0;
  for (uint32_t p = p0; p < p1; p += step) {
    const uint32_t s = T.in_src[p], ls = R.A.len[s];
    if (ls == kNone) continue;
    const double v = R.A.val[s] + T.in_w[p];
    if (pr_before(v, ls + 1, p, bv, bl, bp)) {
      bv = v;
      bl = ls + 1;
      bp = p;
    }
  }
}

// state q's entry of this round, from its best candidate (one lane): proposed in B and filed as changed if it differs from A's
__device__ inline void pr_put(const BestPathsTables& T, const PrPass& R, uint32_t q, double bv, uint32_t bl, uint32_t bp) {
  uint32_t arc;
  if (q == R.start && (bp == kNone || !(bv > 0.0))) {  // the empty path comes before anything of equal value
    bv = 0.0;
    bl = 0;
    arc = kNone;
  } else if (bp == kNone)
    return;  // (no source has an entry: the state has none either, as before)
  else
    arc = T.in_id[bp];
  if (R.A.len[q] == bl && R.A.arc[q] == arc && __double_as_longlong(R.A.val[q]) == __double_as_longlong(bv)) return;
  R.B.val[q] = bv;
  R.B.len[q] = bl;
  R.B.arc[q] = arc;
  R.changed[atomicAdd(&R.counts[2], 1u)] = q;
}

__global__ void __launch_bounds__(256) prune_select_lane_kernel(BestPathsTables T, PrPass R, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const uint32_t q = R.lane_list[idx];
  double bv;
  uint32_t bl, bp;
  pr_scan(T, R, T.in_off[q], T.in_off[q + 1], 1, bv, bl, bp);
  pr_put(T, R, q, bv, bl, bp);
}

__global__ void __launch_bounds__(kLanes) prune_select_wave_kernel(BestPathsTables T, PrPass R, uint32_t n) {
  if (blockIdx.x >= n) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t q = R.wave_list[blockIdx.x];
  double v;
  uint32_t l, p;
  pr_scan(T, R, T.in_off[q] + lane, T.in_off[q + 1], kLanes, v, l, p);
  for (int off = kLanes / 2; off > 0; off >>= 1) {  // the order is total, so every lane ends with the same candidate
    const double ov = __shfl_xor(v, off, kLanes);
    const uint32_t ol = __shfl_xor(l, off, kLanes), op = __shfl_xor(p, off, kLanes);
    if (pr_before(ov, ol, op, v, l, p)) {
      v = ov;
      l = ol;
      p = op;
    }
  }
  if (lane == 0) pr_put(T, R, q, v, l, p);
}

// a wavefront per changed state: B's entry becomes A's, the destinations of its out-arcs are active in the next round
__global__ void __launch_bounds__(256) prune_commit_kernel(BestPathsTables T, PrPass R) {
  const uint32_t i = blockIdx.x * (blockDim.x / kLanes) + threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
  if (i >= R.counts[2]) return;
  const uint32_t q = R.changed[i];
  if (lane == 0) {
    R.A.val[q] = R.B.val[q];
    R.A.len[q] = R.B.len[q];
    R.A.arc[q] = R.B.arc[q];
  }
  for (uint32_t p = T.out_off[q] + lane; p < T.out_off[q + 1]; p += kLanes) R.mark[T.out_dst[p]] = 1;
}

__global__ void __launch_bounds__(256) prune_compact_kernel(BestPathsTables T, PrPass R) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= R.n_states || !R.mark[q]) return;
  R.mark[q] = 0;
  if (T.in_off[q + 1] - T.in_off[q] > R.wave_degree)
    R.wave_list[atomicAdd(&R.counts[1], 1u)] = q;
  else
    R.lane_list[atomicAdd(&R.counts[0], 1u)] = q;
}

// round 0: no state has an entry but the start state, whose proposed entry is the empty path and which is the one changed state
__global__ void __launch_bounds__(256) prune_init_kernel(PrPass R) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < R.n_states) {
    R.A.val[q] = kNegInf;
    R.A.len[q] = kNone;
    R.A.arc[q] = kNone;
    R.mark[q] = 0;
  }
  if (q == 0) {
    R.B.val[R.start] = 0.0;
    R.B.len[R.start] = 0;
    R.B.arc[R.start] = kNone;
    R.changed[0] = R.start;
    R.counts[0] = R.counts[1] = 0;
    R.counts[2] = 1;
  }
}

struct PrMark {
  uint32_t n_states, final_state, max_states;
  uint64_t n_arcs;
  double limit, min_arc_logw;
  PrEntry F, R;  // the committed entries of the two passes
  const uint32_t* a_src;
  const uint32_t* a_dst;
  const double* a_w;
  uint8_t* on_state;   // [|Q|], [n_arcs]: on P*
  uint8_t* on_arc;
  uint64_t* key;       // [|Q|] x 2 each, the ranking's input and output
  uint32_t* id;
  uint8_t* state_keep;
  uint8_t* arc_keep;
  unsigned long long* kept;  // states, arcs
  int* err;
};

// one lane: P* back from the final state, its length known
__global__ void prune_walk_kernel(PrMark M) {
  uint32_t q = M.final_state;
  uint32_t k = M.F.len[q];
  if (k == kNone) return;  // (no path)
  if (k > M.n_states) {    // (a best path of more arcs than states would repeat a state)
    atomicOr(M.err, kErrWalk);
    return;
  }
  for (; k > 0; --k) {
    const uint32_t arc = M.F.arc[q];
    if (arc >= M.n_arcs || M.F.len[q] != k) {
      atomicOr(M.err, kErrWalk);
      return;
    }
    M.on_arc[arc] = 1;
    M.on_state[q] = 1;
    q = M.a_src[arc];
  }
  M.on_state[q] = 1;
  if (q != 0 || M.F.len[0] != 0 || M.F.arc[0] != kNone) atomicOr(M.err, kErrWalk);  // (it ends at the empty path)
}

// T(q) as a key that sorts ascending where T sorts descending, and the state ids
__global__ void __launch_bounds__(256) prune_key_kernel(PrMark M) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= M.n_states) return;
  double t = M.F.val[q] + M.R.val[q];
  if (t == 0.0) t = 0.0;  // (-0.0 is 0.0)
  const uint64_t b = (uint64_t)__double_as_longlong(t);
  const uint64_t up = (b >> 63) ? ~b : (b | 0x8000000000000000ull);  // ascending with t
  M.key[q] = ~up;
  M.id[q] = q;
}

// the sorted ids' first max_states are within the cap
__global__ void __launch_bounds__(256) prune_cap_kernel(PrMark M) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < M.n_states && i < M.max_states) M.state_keep[M.id[M.n_states + i]] = 1;
}

__device__ inline void pr_count(bool keep, unsigned long long* counter) {
  const unsigned long long m = __ballot(keep);
  if (keep && (threadIdx.x % kLanes) == (uint32_t)__ffsll(m) - 1) atomicAdd(counter, (unsigned long long)__popcll(m));
}

// state_keep holds "within the cap" on entry
__global__ void __launch_bounds__(256) prune_states_kernel(PrMark M) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  bool keep = false;
  if (q < M.n_states) {
    keep = M.state_keep[q] && (M.F.val[q] + M.R.val[q] >= M.limit || M.on_state[q]);
    M.state_keep[q] = keep ? 1 : 0;
  }
  pr_count(keep, &M.kept[0]);
}

__global__ void __launch_bounds__(256) prune_arcs_kernel(PrMark M) {
  const uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool keep = false;
  if (a < M.n_arcs) {
    const double w = M.a_w[a];
    const uint32_t s = M.a_src[a], t = M.a_dst[a];
    keep = w > kNegInf && w >= M.min_arc_logw && M.state_keep[s] && M.state_keep[t] &&
           ((M.F.val[s] + w) + M.R.val[t] >= M.limit || M.on_arc[a]);
    M.arc_keep[a] = keep ? 1 : 0;
  }
  pr_count(keep, &M.kept[1]);
}

// the tables of the two passes for this threshold: built and copied by the first call, dropped by carmel_hip_decoder_set_weights
int upload_prune_tables(carmel_hip_decoder* d, double min_arc_logw) {
  if (d->pr_ready && d->pr_min_arc_logw == min_arc_logw) return CARMEL_HIP_OK;
  d->pr_ready = false;
  std::vector<double> w(d->logw);
  for (double& x : w)
    if (!(x >= min_arc_logw)) x = kNegInf;
  const BestPathsTablesHost HF = build_best_paths_tables(d->n_states, d->src, d->dst, w);  // (they live until the copies are made)
  const BestPathsTablesHost HR = build_best_paths_tables(d->n_states, d->dst, d->src, w);
  d->pr_cycle_arc = positive_cycle_arc(HF, d->src, d->dst, w);
  if (d->pr_cycle_arc < 0) {
    hipStream_t s = d->stream;
    const BestPathsTablesHost* H[2] = {&HF, &HR};
    for (int i = 0; i < 2; ++i) {
      DevBuf<uint32_t>* u = d->pr_u32 + 5 * i;
      HIPCHK(u[0].upload(H[i]->in_off, s));
      HIPCHK(u[1].upload(H[i]->in_src, s));
      HIPCHK(u[2].upload(H[i]->in_id, s));
      HIPCHK(d->pr_f64[i].upload(H[i]->in_w, s));
      HIPCHK(u[3].upload(H[i]->out_off, s));
      HIPCHK(u[4].upload(H[i]->out_dst, s));
      d->PR[i] = BestPathsTables{u[0].p, u[1].p, u[2].p, d->pr_f64[i].p, u[3].p, u[4].p};
    }
    HIPCHK(d->pr_dst.upload(d->dst, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  d->pr_min_arc_logw = min_arc_logw;
  d->pr_ready = true;
  return CARMEL_HIP_OK;
}

// one pass' buffers
struct PassBufs {
  DevBuf<double> a_val, b_val;
  DevBuf<uint32_t> a_len, a_arc, b_len, b_arc, lane_list, wave_list, changed;
  DevBuf<uint8_t> mark;
  int alloc(PrPass& R, uint32_t Q, uint32_t start, uint32_t wave_degree, uint32_t* counts) {
    HIPCHK(a_val.alloc(Q));
    HIPCHK(b_val.alloc(Q));
    HIPCHK(a_len.alloc(Q));
    HIPCHK(a_arc.alloc(Q));
    HIPCHK(b_len.alloc(Q));
    HIPCHK(b_arc.alloc(Q));
    HIPCHK(lane_list.alloc(Q));
    HIPCHK(wave_list.alloc(Q));
    HIPCHK(changed.alloc(Q));
    HIPCHK(mark.alloc(Q));
    R = PrPass{Q, start, wave_degree, {a_val.p, a_len.p, a_arc.p}, {b_val.p, b_len.p, b_arc.p}, mark.p, lane_list.p, wave_list.p,
               changed.p, counts};
    return CARMEL_HIP_OK;
  }
};
}  // namespace

extern "C" {

int carmel_hip_decoder_prune(carmel_hip_decoder* d, double log_ratio, uint32_t max_states, double min_arc_logw, uint8_t* state_keep,
                             uint8_t* arc_keep, uint64_t* n_states_kept, uint64_t* n_arcs_kept) {
  const std::string who = "carmel_hip_decoder_prune";
  if (!d || !state_keep || !arc_keep) return fail(CARMEL_HIP_ERR_ARG, who + ": bad argument");
  if (!(log_ratio >= 0.0)) return fail(CARMEL_HIP_ERR_ARG, who + ": log_ratio must be >= 0 (+inf: no ratio test)");
  if (max_states == 0) return fail(CARMEL_HIP_ERR_ARG, who + ": max_states must be >= 1 (UINT32_MAX: no cap)");
  if (std::isnan(min_arc_logw)) return fail(CARMEL_HIP_ERR_ARG, who + ": min_arc_logw is not a number");
  if (d->n_states >= (1u << 31)) return fail(CARMEL_HIP_ERR_ARG, who + ": states must be below 2^31");
  HIPCHK(hipSetDevice(d->device));
  if (const int rc = upload_prune_tables(d, min_arc_logw)) return rc;
  if (d->pr_cycle_arc >= 0) {
    const int64_t a = d->pr_cycle_arc;
    return fail(CARMEL_HIP_ERR_UNSUPPORTED, who + ": arc " + std::to_string(a) + " (" + std::to_string(d->src[a]) + " -> " +
                                                std::to_string(d->dst[a]) + ") has a weight above 1 and lies on a cycle: the best path is undefined");
  }
  hipStream_t s = d->stream;
  const uint32_t Q = d->n_states;
  const uint64_t n_arcs = d->n_arcs;
  uint32_t wave_degree = kWaveDegree;
  if (const char* v = lib_opt("best_paths_wave_degree")) wave_degree = (uint32_t)std::min<unsigned long long>(std::strtoull(v, nullptr, 10), kNone);
  PassBufs bufs[2];
  PrPass P[2];
  DevBuf<uint32_t> counts, id;
  DevBuf<uint64_t> key;
  DevBuf<uint8_t> on_state, on_arc, d_state_keep, d_arc_keep, sort_tmp;
  DevBuf<unsigned long long> kept;
  DevBuf<int> d_err;
  HIPCHK(counts.alloc(6));
  for (int i = 0; i < 2; ++i)
    if (const int rc = bufs[i].alloc(P[i], Q, i ? d->final_state : 0, wave_degree, counts.p + 3 * i)) return rc;
  HIPCHK(on_state.alloc(Q));
  HIPCHK(on_arc.alloc(std::max<uint64_t>(n_arcs, 1)));
  HIPCHK(d_state_keep.alloc(Q));
  HIPCHK(d_arc_keep.alloc(std::max<uint64_t>(n_arcs, 1)));
  HIPCHK(kept.alloc(2));
  HIPCHK(d_err.alloc(1));
  const bool capped = max_states < Q;
  size_t tmp_bytes = 0;
  if (capped) {
    HIPCHK(key.alloc(2 * (size_t)Q));
    HIPCHK(id.alloc(2 * (size_t)Q));
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, key.p, key.p + Q, id.p, id.p + Q, (int)Q, 0, 64, s));
    HIPCHK(sort_tmp.alloc(std::max<size_t>(tmp_bytes, 1)));
  }
  HIPCHK(hipMemsetAsync(on_state.p, 0, Q, s));
  HIPCHK(hipMemsetAsync(on_arc.p, 0, std::max<uint64_t>(n_arcs, 1), s));
  HIPCHK(hipMemsetAsync(d_state_keep.p, capped ? 0 : 1, Q, s));
  HIPCHK(hipMemsetAsync(kept.p, 0, 2 * sizeof(unsigned long long), s));
  HIPCHK(hipMemsetAsync(d_err.p, 0, sizeof(int), s));
  DecodeChunk c{d};
  c.ms = 0;
  const uint32_t qb = (Q + 255) / 256;
  uint32_t h_counts[6] = {0, 0, 0, 0, 0, 0};
  // round 0 of both passes, then the states that the start states' arcs enter
  if (const int rc = c.begin()) return rc;
  for (int i = 0; i < 2; ++i) {
    prune_init_kernel<<<qb, 256, 0, s>>>(P[i]);
    prune_commit_kernel<<<1, 256, 0, s>>>(d->PR[i], P[i]);
    prune_compact_kernel<<<qb, 256, 0, s>>>(d->PR[i], P[i]);
  }
  if (const int rc = c.end()) return rc;
  HIPCHK(hipMemcpyAsync(h_counts, counts.p, sizeof h_counts, hipMemcpyDeviceToHost, s));
  if (const int rc = c.wait()) return rc;
  const uint64_t cap = (uint64_t)Q + 1;
  uint32_t rounds[2] = {0, 0};
  while (h_counts[0] + h_counts[1] + h_counts[3] + h_counts[4]) {
    uint32_t n_lane[2], n_wave[2];
    for (int i = 0; i < 2; ++i) {
      n_lane[i] = h_counts[3 * i];
      n_wave[i] = h_counts[3 * i + 1];
      if (n_lane[i] > Q || n_wave[i] > Q - n_lane[i]) return fail(CARMEL_HIP_ERR_STATE, who + ": inconsistent worklist");
      if (n_lane[i] + n_wave[i] && ++rounds[i] > cap)
        return fail(CARMEL_HIP_ERR_STATE, who + ": did not converge in " + std::to_string(cap) + " rounds");
    }
    if (const int rc = c.begin()) return rc;
    HIPCHK(hipMemsetAsync(counts.p, 0, 6 * sizeof(uint32_t), s));
    for (int i = 0; i < 2; ++i) {
      if (!(n_lane[i] + n_wave[i])) continue;
      if (n_lane[i]) prune_select_lane_kernel<<<(n_lane[i] + 255) / 256, 256, 0, s>>>(d->PR[i], P[i], n_lane[i]);
      if (n_wave[i]) prune_select_wave_kernel<<<n_wave[i], kLanes, 0, s>>>(d->PR[i], P[i], n_wave[i]);
      prune_commit_kernel<<<(n_lane[i] + n_wave[i] + 3) / 4, 256, 0, s>>>(d->PR[i], P[i]);
      prune_compact_kernel<<<qb, 256, 0, s>>>(d->PR[i], P[i]);
    }
    if (const int rc = c.end()) return rc;
    HIPCHK(hipMemcpyAsync(h_counts, counts.p, sizeof h_counts, hipMemcpyDeviceToHost, s));
    if (const int rc = c.wait()) return rc;
  }
  // the limit, P*, the ranking and the marks
  double f_final = kNegInf;
  HIPCHK(hipMemcpyAsync(&f_final, P[0].A.val + d->final_state, sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  PrMark M{Q, d->final_state, max_states, n_arcs, std::isinf(log_ratio) ? kNegInf : f_final - log_ratio, min_arc_logw, P[0].A, P[1].A,
           d->a_src.p, d->pr_dst.p, d->a_w.p, on_state.p, on_arc.p, key.p, id.p, d_state_keep.p, d_arc_keep.p, kept.p, d_err.p};
  std::vector<uint8_t> h_state(Q), h_arc(n_arcs);
  std::vector<double> fwd(Q), bwd(Q);
  unsigned long long h_kept[2] = {0, 0};
  int err = 0;
  if (const int rc = c.begin()) return rc;
  prune_walk_kernel<<<1, 1, 0, s>>>(M);
  if (capped) {
    prune_key_kernel<<<qb, 256, 0, s>>>(M);
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(sort_tmp.p, tmp_bytes, key.p, key.p + Q, id.p, id.p + Q, (int)Q, 0, 64, s));
    prune_cap_kernel<<<qb, 256, 0, s>>>(M);
  }
  prune_states_kernel<<<qb, 256, 0, s>>>(M);
  if (n_arcs) prune_arcs_kernel<<<(uint32_t)((n_arcs + 255) / 256), 256, 0, s>>>(M);
  if (const int rc = c.end()) return rc;
  HIPCHK(hipMemcpyAsync(h_state.data(), d_state_keep.p, Q, hipMemcpyDeviceToHost, s));
  if (n_arcs) HIPCHK(hipMemcpyAsync(h_arc.data(), d_arc_keep.p, n_arcs, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(fwd.data(), P[0].A.val, Q * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(bwd.data(), P[1].A.val, Q * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h_kept, kept.p, sizeof h_kept, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
  if (const int rc = c.wait()) return rc;
  if (err) return fail(CARMEL_HIP_ERR_STATE, who + ": inconsistent back-pointers");
  if (!(f_final > kNegInf) || !h_state[0] || !h_state[d->final_state]) {  // no path, or an endpoint lost: nothing is kept
    std::fill(h_state.begin(), h_state.end(), 0);
    std::fill(h_arc.begin(), h_arc.end(), 0);
    h_kept[0] = h_kept[1] = 0;
  }
  std::memcpy(state_keep, h_state.data(), Q);
  if (n_arcs) std::memcpy(arc_keep, h_arc.data(), n_arcs);
  if (n_states_kept) *n_states_kept = h_kept[0];
  if (n_arcs_kept) *n_arcs_kept = h_kept[1];
  d->pr_fwd.swap(fwd);
  d->pr_bwd.swap(bwd);
  d->pr_have = true;
  d->pr_rounds[0] = rounds[0];
  d->pr_rounds[1] = rounds[1];
  d->last_ms = c.ms;
  return CARMEL_HIP_OK;
}

int carmel_hip_decoder_prune_distances(carmel_hip_decoder* d, double* fwd, double* bwd) {
  if (!d) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decoder_prune_distances: bad argument");
  if (!d->pr_have) return fail(CARMEL_HIP_ERR_STATE, "carmel_hip_decoder_prune_distances: no successful carmel_hip_decoder_prune call yet");
  if (fwd) std::memcpy(fwd, d->pr_fwd.data(), d->pr_fwd.size() * sizeof(double));
  if (bwd) std::memcpy(bwd, d->pr_bwd.data(), d->pr_bwd.size() * sizeof(double));
  return CARMEL_HIP_OK;
}

int carmel_hip_decoder_prune_stats(carmel_hip_decoder* d, uint32_t* fwd_rounds, uint32_t* bwd_rounds) {
  if (!d || !fwd_rounds || !bwd_rounds) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decoder_prune_stats: bad argument");
  *fwd_rounds = d->pr_rounds[0];
  *bwd_rounds = d->pr_rounds[1];
  return CARMEL_HIP_OK;
}

}  // extern "C"
