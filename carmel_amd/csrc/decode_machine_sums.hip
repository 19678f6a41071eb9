// decode_machine_sums.hip — the sum over all paths of the whole machine, the number of its paths and every arc's posterior under
// the machine's own path distribution (carmel --sum outside batch mode: WFST::sum_acyclic_paths, carmel.cc:555-599, fst.h:1183-1191,
// graph.h:391-419; the third line of carmel -c: WFST::numNoCyclePaths, carmel.cc:841-855, fst.h:1166-1174, graph.h:363-378).  The
// log-semiring counterpart of decode_best_paths.hip and decode_prune.hip: a topological sweep over the useful part of the machine.
//
// The rule (DESIGN.md and include/carmel_hip.h state it in the same words; tests/machine_sums_ref.py restates it).
// Arcs.  Only arcs of log weight > -inf exist.  Symbols and `side` play no part.  Log weights above 0 are legal: there are no
//   cycles to amplify them.
// Useful states U.  q is in U iff q is reachable from state 0 and the final state is reachable from q, over existing arcs.  Useful
//   arcs are the existing arcs with both ends in U.  If the final state is not reachable, U is empty.  Cycles outside U (on
//   reachable dead ends, in unreachable parts, self-loops there) are harmless.
// Levels.  U is peeled by in-degree over the useful arcs: state 0 has level 0, level(q) = 1 + max level(src a) over the useful arcs
//   a into q.  A useful state that never reaches in-degree 0 lies on or behind a cycle inside U: CARMEL_HIP_ERR_UNSUPPORTED, the
//   message names the lowest-numbered such state, and the handle's earlier results stay.  A useful self-loop is a cycle, and so is
//   a useful arc into state 0 or out of the final state (every useful state lies between the two).  The backward levels come from
//   the same peeling of the reversed useful machine, started at the final state.
// Forward sum.  alpha[0] = 0.0.  For q in U, q != 0: alpha[q] = Lse (sweep_math.hpp) over q's useful in-arcs of (alpha[src a] +
//   w(a)) in a fixed order: a state of at most `machine_sums_wave_degree` useful in-arcs (option, default 32) by one lane in arc-id
//   order; a state of more by a wavefront, lane l taking positions l, l + 64, ... of the state's list of existing in-arcs (which is
//   in arc-id order; an arc that is not useful has a term of -inf, which Lse passes over), then six shuffle steps (distance 32, 16,
//   8, 4, 2, 1) combining the lanes' (m, acc) pairs, lane k taking lane k + distance's, as consolidate.hip does.  A state with one
//   useful in-arc gets alpha[src] + w bit for bit.  alpha = -inf outside U.
// Backward sum.  The same on the reversed machine: beta[final] = 0.0, the terms are w(a) + beta[dst a], a state's out-arcs in
//   arc-id order.
// Total.  Z = alpha[final]; beta[0] is a second estimate of the same number.
// Path counts.  cf[0] = 1.0, cf[q] = the sum of cf[src a] over the useful in-arcs, plain f64 additions in the order of the sum
//   beside them (the wavefront form adds its lanes' partial counts in the same tree), so the two forms differ only above 2^53, below
//   which the counts are exact.  cb is the same backwards; N = cf[final].  Deviation: the reference counts in its log-float
//   Weight and counts arcs of weight 0 too; here only existing arcs count, in f64.
// Arc posterior.  ln gamma(a) = ((alpha[src a] + w(a)) + beta[dst a]) - Z for a useful arc, -inf otherwise.
// Empty cases.  U empty: success, Z = -inf, N = 0, every array -inf, 0 or 0xffffffff.  The final state being state 0 with nothing
//   useful looping through it: U = {0}, Z = 0.0, N = 1.
// Determinism.  No float atomics; for one value of the option two calls return the same bytes; the worklists' order and the launch
//   geometry play no part in any value (they decide where a state stands in a level's list, never what it reads).
// Deviation from the reference on cycles: it drops the back arcs its depth-first search happens to meet and warns; this refuses.
//
// The kernels.  Every pass runs once per direction -- on the tables of (src, dst, w) for the forward quantities and on those of
// (dst, src, w) for the backward ones -- queued side by side on the handle's one stream; where the host drives a loop it reads both
// directions' counters in one copy a round.  More than |Q| + 1 rounds in any loop: CARMEL_HIP_ERR_STATE.
//   1. Reachability: a frontier search, a round per frontier, a wavefront per frontier state marking its successors with an
//      integer exchange; a state joins the next frontier once.
//   2. Useful states (both marks set) and their count; the useful in-degree of every useful state, a lane per state.
//   3. Peeling: a round per level, a wavefront per state of the level taking one from the in-degree of every useful successor;
//      the successor that reaches 0 gets the next level and is filed on the lanes' or the wavefronts' list, both level-ordered.
//   4. The sweep: per level one launch over the level's slice of either list, sum and path count in the same pass.  The host
//      knows the slices from the peeling, so the levels are queued without reading anything back.
//   5. The posteriors: a lane per arc.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "decode.hpp"
#include "engine.hpp"
#include "sweep_math.hpp"

namespace {
constexpr uint32_t kWaveDegree = 32;  // option machine_sums_wave_degree
constexpr double kNegInf = -std::numeric_limits<double>::infinity();
constexpr int kWavesPerBlock = 4;

// one direction's state: `start` is state 0 (forward) or the final state (backward); T files an arc under the state the sums flow
// into (in_*) and under the state they flow out of (out_*)
struct MsDir {
  BestPathsTables T;
  uint32_t n_states, start, wave_degree;
  uint32_t* reach;      // [|Q|]: 1 once the search from `start` has met the state
  uint32_t* front;      // [2 |Q|]: the search's frontiers, in turn
  uint32_t* deg;        // [|Q|]: the useful in-degree still standing (peeling)
  uint32_t* deg0;       // [|Q|]: the useful in-degree
  uint32_t* level;      // [|Q|]; kNone outside U
  uint32_t* lane_list;  // [|Q|] each: the useful states in level order, by the form that sums them
  uint32_t* wave_list;
  double* sum;          // [|Q|]: alpha or beta
  double* cnt;          // [|Q|]: cf or cb
  uint32_t* counts;     // the lengths of lane_list and wave_list, the length of the next frontier, the lowest state left unpeeled
};

__global__ void __launch_bounds__(256) ms_init_kernel(MsDir R) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < R.n_states) {
    R.reach[q] = q == R.start ? 1u : 0u;
    R.deg[q] = R.deg0[q] = 0;
    R.level[q] = kNone;
    R.sum[q] = kNegInf;
    R.cnt[q] = 0.0;
  }
  if (q == 0) {
    R.front[0] = R.start;
    R.counts[0] = R.counts[1] = R.counts[2] = 0;
    R.counts[3] = kNone;
  }
}

// pass 1: a wavefront per state of the frontier `cur` (n states); a successor met for the first time joins `next`
__global__ void __launch_bounds__(256) ms_reach_kernel(MsDir R, const uint32_t* cur, uint32_t n, uint32_t* next) {
  const uint32_t i = blockIdx.x * kWavesPerBlock + threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
  if (i >= n) return;
  const uint32_t q = cur[i];
  for (uint32_t p = R.T.out_off[q] + lane; p < R.T.out_off[q + 1]; p += kLanes) {
    const uint32_t t = R.T.out_dst[p];
    if (atomicExch(&R.reach[t], 1u) == 0u) next[atomicAdd(&R.counts[2], 1u)] = t;  // (once a state: at most |Q| entries)
  }
}

// pass 2a: U and its size
__global__ void __launch_bounds__(256) ms_useful_kernel(uint32_t n_states, const uint32_t* reach_f, const uint32_t* reach_b, uint8_t* useful,
                                                        unsigned long long* n_useful) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  bool u = false;
  if (q < n_states) {
    u = reach_f[q] && reach_b[q];
    useful[q] = u ? 1 : 0;
  }
  const unsigned long long m = __ballot(u);
  if (u && (threadIdx.x % kLanes) == (uint32_t)__ffsll(m) - 1) atomicAdd(n_useful, (unsigned long long)__popcll(m));
}

// pass 2b: the useful in-degrees; the start state, if nothing useful enters it, is level 0 and holds the empty path
__global__ void __launch_bounds__(256) ms_degree_kernel(MsDir R, const uint8_t* useful) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= R.n_states || !useful[q]) return;
  uint32_t c = 0;
  for (uint32_t p = R.T.in_off[q]; p < R.T.in_off[q + 1]; ++p) c += useful[R.T.in_src[p]];
  R.deg[q] = R.deg0[q] = c;
  if (q == R.start && c == 0) {
    R.level[q] = 0;
    R.sum[q] = 0.0;
    R.cnt[q] = 1.0;
    R.lane_list[0] = q;
    R.counts[0] = 1;
  }
}

// pass 3: a wavefront per state of a level (n states of `list` from `begin`); the successors that lose their last useful in-arc
// are the next level's
__global__ void __launch_bounds__(256) ms_peel_kernel(MsDir R, const uint8_t* useful, const uint32_t* list, uint32_t begin, uint32_t n,
                                                      uint32_t next_level) {
  const uint32_t i = blockIdx.x * kWavesPerBlock + threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
  if (i >= n) return;
  const uint32_t q = list[begin + i];
  for (uint32_t p = R.T.out_off[q] + lane; p < R.T.out_off[q + 1]; p += kLanes) {
    const uint32_t t = R.T.out_dst[p];
    if (!useful[t] || atomicSub(&R.deg[t], 1u) != 1u) continue;
    R.level[t] = next_level;  // (once a state: its in-degree reaches 0 once, so either list holds at most |Q| entries)
    if (R.deg0[t] > R.wave_degree)
      R.wave_list[atomicAdd(&R.counts[1], 1u)] = t;
    else
      R.lane_list[atomicAdd(&R.counts[0], 1u)] = t;
  }
}

// after a peeling that left useful states behind: the lowest of them
__global__ void __launch_bounds__(256) ms_stuck_kernel(MsDir R, const uint8_t* useful) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q < R.n_states && useful[q] && R.level[q] == kNone) atomicMin(&R.counts[3], q);
}

// pass 4, lane form: a lane per state of a level's slice of lane_list
__global__ void __launch_bounds__(256) ms_sweep_lane_kernel(MsDir R, uint32_t begin, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const uint32_t q = R.lane_list[begin + idx];
  carmel_hip::Lse L;
  L.init();
  double c = 0.0;
  for (uint32_t p = R.T.in_off[q]; p < R.T.in_off[q + 1]; ++p) {
    const uint32_t s = R.T.in_src[p];
    L.add(R.sum[s] + R.T.in_w[p]);  // (-inf from a source outside U: no term)
    c += R.cnt[s];                  // (0 from there)
  }
  R.sum[q] = L.value();
  R.cnt[q] = c;
}

// pass 4, wavefront form: a wavefront per state of a level's slice of wave_list
__global__ void __launch_bounds__(256) ms_sweep_wave_kernel(MsDir R, uint32_t begin, uint32_t n) {
  const uint32_t i = blockIdx.x * kWavesPerBlock + threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
  if (i >= n) return;  // (a whole wavefront)
  const uint32_t q = R.wave_list[begin + i];
  carmel_hip::Lse L;
  L.init();
  double c = 0.0;
  for (uint32_t p = R.T.in_off[q] + lane; p < R.T.in_off[q + 1]; p += kLanes) {
    const uint32_t s = R.T.in_src[p];
    L.add(R.sum[s] + R.T.in_w[p]);
    c += R.cnt[s];
  }
  for (int d = kLanes / 2; d; d >>= 1) {
    const double om = __shfl_down(L.m, d, kLanes), oacc = __shfl_down(L.acc, d, kLanes);
    c += __shfl_down(c, d, kLanes);
    if (om == NEG_INF) {  // (a lane without terms adds nothing)
    } else if (L.m == NEG_INF) {
      L.m = om;
      L.acc = oacc;
    } else if (om <= L.m)
      L.acc = L.acc + oacc * K_EXP(om - L.m);
    else {
      L.acc = oacc + L.acc * K_EXP(L.m - om);
      L.m = om;
    }
  }
  if (lane == 0) {
    R.sum[q] = L.value();
    R.cnt[q] = c;
  }
}

// pass 5: a lane per arc
__global__ void __launch_bounds__(256) ms_posterior_kernel(uint64_t n_arcs, const uint32_t* a_src, const uint32_t* a_dst, const double* a_w,
                                                           const uint8_t* useful, const double* alpha, const double* beta,
                                                           uint32_t final_state, double* post) {
  const uint64_t a = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (a >= n_arcs) return;
  const double total = alpha[final_state];
  const double w = a_w[a];
  const uint32_t s = a_src[a], t = a_dst[a];
  post[a] = (w > kNegInf && useful[s] && useful[t]) ? ((alpha[s] + w) + beta[t]) - total : kNegInf;
}

// the tables of the machine and of its reversal (the arc ids stay): built and copied by the first call, dropped by
// carmel_hip_decoder_set_weights
int upload_machine_sums_tables(carmel_hip_decoder* d) {
  if (d->ms_ready) return CARMEL_HIP_OK;
  const BestPathsTablesHost HF = build_best_paths_tables(d->n_states, d->src, d->dst, d->logw);  // (they live until the copies are made)
  const BestPathsTablesHost HR = build_best_paths_tables(d->n_states, d->dst, d->src, d->logw);
  hipStream_t s = d->stream;
  const BestPathsTablesHost* H[2] = {&HF, &HR};
  for (int i = 0; i < 2; ++i) {
    DevBuf<uint32_t>* u = d->ms_u32 + 5 * i;
    HIPCHK(u[0].upload(H[i]->in_off, s));
    HIPCHK(u[1].upload(H[i]->in_src, s));
    HIPCHK(u[2].upload(H[i]->in_id, s));
    HIPCHK(d->ms_f64[i].upload(H[i]->in_w, s));
    HIPCHK(u[3].upload(H[i]->out_off, s));
    HIPCHK(u[4].upload(H[i]->out_dst, s));
    d->MS[i] = BestPathsTables{u[0].p, u[1].p, u[2].p, d->ms_f64[i].p, u[3].p, u[4].p};
  }
  HIPCHK(d->ms_dst.upload(d->dst, s));
  HIPCHK(hipStreamSynchronize(s));
  d->ms_ready = true;
  return CARMEL_HIP_OK;
}

// one direction's buffers
struct DirBufs {
  DevBuf<uint32_t> reach, front, deg, deg0, level, lane_list, wave_list;
  DevBuf<double> sum, cnt;
  int alloc(MsDir& R, const BestPathsTables& T, uint32_t Q, uint32_t start, uint32_t wave_degree, uint32_t* counts) {
    HIPCHK(reach.alloc(Q));
    HIPCHK(front.alloc(2 * (size_t)Q));
    HIPCHK(deg.alloc(Q));
    HIPCHK(deg0.alloc(Q));
    HIPCHK(level.alloc(Q));
    HIPCHK(lane_list.alloc(Q));
    HIPCHK(wave_list.alloc(Q));
    HIPCHK(sum.alloc(Q));
    HIPCHK(cnt.alloc(Q));
    R = MsDir{T, Q, start, wave_degree, reach.p, front.p, deg.p, deg0.p, level.p, lane_list.p, wave_list.p, sum.p, cnt.p, counts};
    return CARMEL_HIP_OK;
  }
};

inline uint32_t wave_blocks(uint32_t n) { return (n + kWavesPerBlock - 1) / kWavesPerBlock; }
}  // namespace

extern "C" {

int carmel_hip_decoder_machine_sums(carmel_hip_decoder* d, double* total_logw, double* n_paths, uint64_t* n_useful) {
  const std::string who = "carmel_hip_decoder_machine_sums";
  if (!d) return fail(CARMEL_HIP_ERR_ARG, who + ": bad argument");
  if (d->n_states >= (1u << 31)) return fail(CARMEL_HIP_ERR_ARG, who + ": states must be below 2^31");
  HIPCHK(hipSetDevice(d->device));
  if (const int rc = upload_machine_sums_tables(d)) return rc;
  hipStream_t s = d->stream;
  const uint32_t Q = d->n_states;
  const uint64_t n_arcs = d->n_arcs;
  uint32_t wave_degree = kWaveDegree;
  if (const char* v = lib_opt("machine_sums_wave_degree")) wave_degree = (uint32_t)std::min<unsigned long long>(std::strtoull(v, nullptr, 10), kNone);
  DirBufs bufs[2];
  MsDir P[2];
  DevBuf<uint32_t> counts;
  DevBuf<uint8_t> useful;
  DevBuf<unsigned long long> d_useful;
  DevBuf<double> post;
  HIPCHK(counts.alloc(8));
  for (int i = 0; i < 2; ++i)
    if (const int rc = bufs[i].alloc(P[i], d->MS[i], Q, i ? d->final_state : 0, wave_degree, counts.p + 4 * i)) return rc;
  HIPCHK(useful.alloc(Q));
  HIPCHK(d_useful.alloc(1));
  HIPCHK(post.alloc(std::max<uint64_t>(n_arcs, 1)));
  HIPCHK(hipMemsetAsync(d_useful.p, 0, sizeof(unsigned long long), s));
  DecodeChunk c{d};
  c.ms = 0;
  const uint32_t qb = (Q + 255) / 256;
  const uint64_t cap = (uint64_t)Q + 1;
  uint32_t h_counts[8];
  // 1. reachability, both directions a round at a time
  if (const int rc = c.begin()) return rc;
  for (int i = 0; i < 2; ++i) ms_init_kernel<<<qb, 256, 0, s>>>(P[i]);
  if (const int rc = c.end()) return rc;
  if (const int rc = c.wait()) return rc;
  uint32_t n_front[2] = {1, 1};
  for (uint64_t round = 0; n_front[0] + n_front[1]; ++round) {
    if (round > cap) return fail(CARMEL_HIP_ERR_STATE, who + ": the search did not end in " + std::to_string(cap) + " rounds");
    const uint32_t par = (uint32_t)(round & 1);
    if (const int rc = c.begin()) return rc;
    for (int i = 0; i < 2; ++i) {
      HIPCHK(hipMemsetAsync(P[i].counts + 2, 0, sizeof(uint32_t), s));
      if (n_front[i])
        ms_reach_kernel<<<wave_blocks(n_front[i]), 256, 0, s>>>(P[i], P[i].front + (size_t)par * Q, n_front[i], P[i].front + (size_t)(1 - par) * Q);
    }
    if (const int rc = c.end()) return rc;
    HIPCHK(hipMemcpyAsync(h_counts, counts.p, sizeof h_counts, hipMemcpyDeviceToHost, s));
    if (const int rc = c.wait()) return rc;
    for (int i = 0; i < 2; ++i) {
      n_front[i] = h_counts[4 * i + 2];
      if (n_front[i] > Q) return fail(CARMEL_HIP_ERR_STATE, who + ": inconsistent frontier");
    }
  }
  // 2. U, the useful in-degrees, level 0
  unsigned long long h_useful = 0;
  if (const int rc = c.begin()) return rc;
  ms_useful_kernel<<<qb, 256, 0, s>>>(Q, P[0].reach, P[1].reach, useful.p, d_useful.p);
  for (int i = 0; i < 2; ++i) ms_degree_kernel<<<qb, 256, 0, s>>>(P[i], useful.p);
  if (const int rc = c.end()) return rc;
  HIPCHK(hipMemcpyAsync(&h_useful, d_useful.p, sizeof h_useful, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h_counts, counts.p, sizeof h_counts, hipMemcpyDeviceToHost, s));
  if (const int rc = c.wait()) return rc;
  if (h_useful > Q) return fail(CARMEL_HIP_ERR_STATE, who + ": inconsistent count of useful states");
  // 3. peeling: lane_off / wave_off [i][l] .. [i][l + 1] are level l's slices of direction i's lists
  std::vector<uint32_t> lane_off[2], wave_off[2];
  for (int i = 0; i < 2; ++i) {
    lane_off[i].assign(1, 0);
    wave_off[i].assign(1, 0);
  }
  bool open[2] = {h_useful > 0, h_useful > 0};  // the direction may still have a level to peel
  for (uint64_t round = 0; open[0] || open[1]; ++round) {
    if (round > cap) return fail(CARMEL_HIP_ERR_STATE, who + ": the peeling did not end in " + std::to_string(cap) + " rounds");
    uint32_t lo[2][2] = {{0, 0}, {0, 0}}, n[2][2] = {{0, 0}, {0, 0}};  // [direction][lane, wave]: the level's slices
    for (int i = 0; i < 2; ++i) {
      if (!open[i]) continue;
      const uint32_t nl = h_counts[4 * i], nw = h_counts[4 * i + 1];
      lo[i][0] = lane_off[i].back();
      lo[i][1] = wave_off[i].back();
      if (nl > Q || nw > Q - nl || nl < lo[i][0] || nw < lo[i][1]) return fail(CARMEL_HIP_ERR_STATE, who + ": inconsistent worklist");
      n[i][0] = nl - lo[i][0];
      n[i][1] = nw - lo[i][1];
      if (!(n[i][0] + n[i][1])) {
        open[i] = false;
        continue;
      }
      lane_off[i].push_back(nl);
      wave_off[i].push_back(nw);
    }
    if (!open[0] && !open[1]) break;
    if (const int rc = c.begin()) return rc;
    for (int i = 0; i < 2; ++i) {
      if (!open[i]) continue;
      const uint32_t next_level = (uint32_t)lane_off[i].size() - 1;
      if (n[i][0]) ms_peel_kernel<<<wave_blocks(n[i][0]), 256, 0, s>>>(P[i], useful.p, P[i].lane_list, lo[i][0], n[i][0], next_level);
      if (n[i][1]) ms_peel_kernel<<<wave_blocks(n[i][1]), 256, 0, s>>>(P[i], useful.p, P[i].wave_list, lo[i][1], n[i][1], next_level);
    }
    if (const int rc = c.end()) return rc;
    HIPCHK(hipMemcpyAsync(h_counts, counts.p, sizeof h_counts, hipMemcpyDeviceToHost, s));
    if (const int rc = c.wait()) return rc;
  }
  const uint32_t n_levels[2] = {(uint32_t)lane_off[0].size() - 1, (uint32_t)lane_off[1].size() - 1};
  uint64_t n_peeled[2];
  for (int i = 0; i < 2; ++i) n_peeled[i] = (uint64_t)lane_off[i].back() + wave_off[i].back();
  if (n_peeled[0] != h_useful || n_peeled[1] != h_useful) {
    // a cycle inside U: useful states were left with useful in-arcs standing.  It stalls both directions (a state on it is never
    // peeled either way), so the forward peeling's leftovers are the ones the rule names
    if (n_peeled[0] == h_useful) return fail(CARMEL_HIP_ERR_STATE, who + ": the two peelings disagree");
    if (const int rc = c.begin()) return rc;
    ms_stuck_kernel<<<qb, 256, 0, s>>>(P[0], useful.p);
    if (const int rc = c.end()) return rc;
    HIPCHK(hipMemcpyAsync(h_counts, counts.p, sizeof h_counts, hipMemcpyDeviceToHost, s));
    if (const int rc = c.wait()) return rc;
    if (h_counts[3] >= Q) return fail(CARMEL_HIP_ERR_STATE, who + ": inconsistent levels");
    return fail(CARMEL_HIP_ERR_UNSUPPORTED, who + ": state " + std::to_string(h_counts[3]) +
                                                " lies on or behind a cycle of the useful part of the machine: the sum over all paths is undefined");
  }
  // 4. the sweeps, level by level (level 0 is the start state alone, set by pass 2), and 5. the posteriors
  std::vector<double> alpha(Q), beta(Q), cf(Q), cb(Q), h_post(n_arcs);
  std::vector<uint32_t> level(Q);
  if (const int rc = c.begin()) return rc;
  for (uint32_t l = 1; l < std::max(n_levels[0], n_levels[1]); ++l)
    for (int i = 0; i < 2; ++i) {
      if (l >= n_levels[i]) continue;
      const uint32_t nl = lane_off[i][l + 1] - lane_off[i][l], nw = wave_off[i][l + 1] - wave_off[i][l];
      if (nl) ms_sweep_lane_kernel<<<(nl + 255) / 256, 256, 0, s>>>(P[i], lane_off[i][l], nl);
      if (nw) ms_sweep_wave_kernel<<<wave_blocks(nw), 256, 0, s>>>(P[i], wave_off[i][l], nw);
    }
  if (n_arcs)
    ms_posterior_kernel<<<(uint32_t)((n_arcs + 255) / 256), 256, 0, s>>>(n_arcs, d->a_src.p, d->ms_dst.p, d->a_w.p, useful.p, P[0].sum, P[1].sum,
                                                                        d->final_state, post.p);
  if (const int rc = c.end()) return rc;
  HIPCHK(hipMemcpyAsync(alpha.data(), P[0].sum, Q * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(beta.data(), P[1].sum, Q * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(cf.data(), P[0].cnt, Q * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(cb.data(), P[1].cnt, Q * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(level.data(), P[0].level, Q * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if (n_arcs) HIPCHK(hipMemcpyAsync(h_post.data(), post.p, n_arcs * sizeof(double), hipMemcpyDeviceToHost, s));
  if (const int rc = c.wait()) return rc;
  d->ms_total = alpha[d->final_state];
  d->ms_paths = cf[d->final_state];
  d->ms_useful = h_useful;
  d->ms_levels[0] = n_levels[0];
  d->ms_levels[1] = n_levels[1];
  d->ms_alpha.swap(alpha);
  d->ms_beta.swap(beta);
  d->ms_cf.swap(cf);
  d->ms_cb.swap(cb);
  d->ms_level.swap(level);
  d->ms_post.swap(h_post);
  d->ms_have = true;
  if (total_logw) *total_logw = d->ms_total;
  if (n_paths) *n_paths = d->ms_paths;
  if (n_useful) *n_useful = d->ms_useful;
  d->last_ms = c.ms;
  return CARMEL_HIP_OK;
}

int carmel_hip_decoder_machine_sums_states(carmel_hip_decoder* d, double* alpha, double* beta, double* paths_to, double* paths_from,
                                           uint32_t* fwd_level) {
  if (!d) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decoder_machine_sums_states: bad argument");
  if (!d->ms_have)
    return fail(CARMEL_HIP_ERR_STATE, "carmel_hip_decoder_machine_sums_states: no successful carmel_hip_decoder_machine_sums call yet");
  const size_t Q = d->ms_alpha.size();
  if (alpha) std::memcpy(alpha, d->ms_alpha.data(), Q * sizeof(double));
  if (beta) std::memcpy(beta, d->ms_beta.data(), Q * sizeof(double));
  if (paths_to) std::memcpy(paths_to, d->ms_cf.data(), Q * sizeof(double));
  if (paths_from) std::memcpy(paths_from, d->ms_cb.data(), Q * sizeof(double));
  if (fwd_level) std::memcpy(fwd_level, d->ms_level.data(), Q * sizeof(uint32_t));
  return CARMEL_HIP_OK;
}

int carmel_hip_decoder_machine_sums_arcs(carmel_hip_decoder* d, double* log_posterior) {
  if (!d) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decoder_machine_sums_arcs: bad argument");
  if (!d->ms_have)
    return fail(CARMEL_HIP_ERR_STATE, "carmel_hip_decoder_machine_sums_arcs: no successful carmel_hip_decoder_machine_sums call yet");
  if (log_posterior && !d->ms_post.empty()) std::memcpy(log_posterior, d->ms_post.data(), d->ms_post.size() * sizeof(double));
  return CARMEL_HIP_OK;
}

int carmel_hip_decoder_machine_sums_stats(carmel_hip_decoder* d, uint32_t* fwd_levels, uint32_t* bwd_levels) {
  if (!d) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decoder_machine_sums_stats: bad argument");
  if (!d->ms_have)
    return fail(CARMEL_HIP_ERR_STATE, "carmel_hip_decoder_machine_sums_stats: no successful carmel_hip_decoder_machine_sums call yet");
  if (fwd_levels) *fwd_levels = d->ms_levels[0];
  if (bwd_levels) *bwd_levels = d->ms_levels[1];
  return CARMEL_HIP_OK;
}

}  // extern "C"
