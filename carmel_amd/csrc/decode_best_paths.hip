// decode_best_paths.hip — the K best paths of the whole machine (carmel -k n without -b / -i: print_kbest(kPaths, result) on the
// composed result, carmel.cc:1380-1381, 379-397; WFST::visit_kbest, fst.h:791, kbest.h).  No lines and no positions: the machine
// is the big object and may be cyclic, so the dense trellises do not apply.  K-lists per state, relaxed in Jacobi rounds over a
// worklist until nothing changes.
//
// The rule (DESIGN.md and include/carmel_hip.h state it in the same words; tests/best_paths_ref.py restates it).
// Arcs.  Only arcs of log weight > -inf exist.  Symbols play no part: an *e*:*e* arc is an arc like any other.
// Paths.  A path is a sequence of arcs from state 0 that ends in the final state; it may pass through the final state on the way.
//   The empty path exists if and only if the final state is state 0.  Two paths differ if their arc-id sequences differ.
// Value.  A path's value is its arcs' logs added in path order from 0.0, ((0 + w1) + w2) + ...  The weight REPORTED is, as
//   everywhere in the decoders, the arcs added from the end, w1 + (w2 + (... + (wn + 0))); the empty path reports 0.0.
// Lists.  Every state holds a list of at most K entries (value f64, length u32 = number of arcs, last arc u32, rank u16 of the
//   predecessor in the last arc's source list).  The candidates of state q are: for q = 0 the empty path (0.0, 0, no arc); for
//   every arc a into q and every rank r of list(src a) the entry (list(src a)[r].value + w(a), list(src a)[r].length + 1, a, r).
//   The list is a K-way merge: every arc's candidates are taken in rank order (a later rank of an arc never overtakes an earlier
//   one of the same arc), and among the arcs' current heads -- and the empty path, which comes before anything of equal value --
//   the next entry is the one of the greatest value, then the smallest length, then the lowest arc id.  This is NOT a global sort
//   key: after rounding, S[r] + w can collide for two ranks whose lengths are the other way round, so decode_kbest_list.hpp's
//   bisection (a key monotone in r) does not carry over; a head counter per in-arc does (a u16 per position of the in-arc table,
//   in global memory).  The length key keeps the read-out well-founded: without it a zero-weight self-loop of lower arc id than
//   the arc entering its state would put (loop, rank 0) at rank 0, pointing at itself.
// Rounds.  Round 0: list(0) = [empty path], every other list empty.  Round t + 1 computes every list from round t's lists (Jacobi,
//   never in place).  The result is the lists of the first round that equal the previous round's in all four fields.  Round t's
//   lists are the K best walks of at most t arcs, so the result does not depend on scheduling, worklists or lane counts; a state
//   none of whose sources' lists changed in round t keeps its list in round t + 1 by definition, which is what permits the worklist.
// Read-out.  Path r of list(final) is followed back through (arc, rank) to the empty path; the length field gives its size.
// Convergence.  In exact arithmetic removing a cycle from a walk yields a walk that comes before it, so the K-th best walk has
//   fewer than K |Q| arcs: more than K |Q| + 1 rounds is CARMEL_HIP_ERR_STATE.
// Weights above 1.  An existing arc of log weight > 0 whose source and destination lie on a common cycle makes the call fail with
//   CARMEL_HIP_ERR_UNSUPPORTED (decode_best_paths_tables.cpp finds it on the host); positive arcs off every cycle are legal.
//
// Two buffers of |Q| K entries, A and B, as arrays per field.  Per round:
//   1. select over the active states: reads A, merges into B, files the state as changed if B's list differs from A's.  Two forms
//      that give the same bytes: a state per lane (best_paths_select_lane_kernel) for in-degree <= the option
//      "best_paths_wave_degree" (default kWaveDegree; 0: every state takes the wave form), and a wavefront per state above it
//      (best_paths_select_wave_kernel): its 64 lanes stride over the in-arcs, each keeps the best of its heads in registers, a
//      wave-wide argmax by (value, length, position) through shuffles picks the slot's entry, and only the lane that owned it
//      advances that head and looks through its arcs again.  Within a destination the in-arcs are in arc-id order, so the
//      position in the table stands for the arc id.  Nothing is indexed per lane: no scratch.
//   2. commit over the changed states, a wavefront each: copies B to A and marks the destinations of the state's out-arcs with
//      plain byte stores of 1.
//   3. compact: the marks become the next round's two active lists (by in-degree) and are cleared.
// The host reads the three counters once a round and stops when nothing is active.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "decode.hpp"
#include "decode_kbest_list.hpp"  // kMaxK
#include "engine.hpp"

namespace {
constexpr uint32_t kWaveDegree = 32;  // states of more in-arcs than this take the wave form

struct BpLists {
  double* val;     // [|Q| K]
  uint32_t* len;
  uint32_t* arc;   // the arc id; kNone: the empty path
  uint16_t* rank;
  uint32_t* n;     // [|Q|]: the entries the state's list holds
};

struct BpRound {
  uint32_t K, n_states, wave_degree;
  BpLists A, B;
  uint16_t* head;       // [n_in]: per in-arc position, the rank of its next candidate
  uint8_t* mark;        // [|Q|]
  uint32_t* lane_list;  // [|Q|] each
  uint32_t* wave_list;
  uint32_t* changed;
  uint32_t* counts;     // the lengths of lane_list, wave_list and changed
};

// candidate 1 comes before candidate 2 (p: the position in the in-arc table, kNone: no candidate)
__device__ inline bool bp_before(double v1, uint32_t l1, uint32_t p1, double v2, uint32_t l2, uint32_t p2) {
  if (p1 == kNone) return false;
  if (p2 == kNone) return true;
  if (v1 != v2) return v1 > v2;
  if (l1 != l2) return l1 < l2;
  return p1 < p2;
}

// the best of the heads of in-arcs p0, p0 + step, ... below p1
__device__ inline void bp_scan(const BestPathsTables& T, const BpRound& R, uint32_t p0, uint32_t p1, uint32_t step, double& bv,
                               uint32_t& bl, uint32_t& bp) {
  bp = kNone;
  bv = 0.0;
  bl = 0;
  for (uint32_t p = p0; p < p1; p += step) {
    const uint32_t h = R.head[p], s = T.in_src[p];
    if (h >= R.A.n[s]) continue;
    const size_t e = (size_t)s * R.K + h;
    const double v = R.A.val[e] + T.in_w[p];
    const uint32_t l = R.A.len[e] + 1;
    if (bp_before(v, l, p, bv, bl, bp)) {
      bv = v;
      bl = l;
      bp = p;
    }
  }
}

// the first of the 64 lanes' candidates, to every lane: the order is total, so every lane ends with the same one
__device__ inline void bp_wave_best(double& v, uint32_t& l, uint32_t& p) {
  for (int off = kLanes / 2; off > 0; off >>= 1) {
    const double ov = __shfl_xor(v, off, kLanes);
    const uint32_t ol = __shfl_xor(l, off, kLanes), op = __shfl_xor(p, off, kLanes);
    if (bp_before(ov, ol, op, v, l, p)) {
      v = ov;
      l = ol;
      p = op;
    }
  }
}

// entry s of B's list of state q -> it differs from A's
__device__ inline bool bp_put(const BpRound& R, uint32_t q, uint32_t s, uint32_t n_old, double v, uint32_t l, uint32_t arc, uint32_t r) {
  const size_t e = (size_t)q * R.K + s;
  R.B.val[e] = v;
  R.B.len[e] = l;
  R.B.arc[e] = arc;
  R.B.rank[e] = (uint16_t)r;
  return s >= n_old || __double_as_longlong(R.A.val[e]) != __double_as_longlong(v) || R.A.len[e] != l || R.A.arc[e] != arc ||
         R.A.rank[e] != (uint16_t)r;
}

__global__ void __launch_bounds__(256) best_paths_select_lane_kernel(BestPathsTables T, BpRound R, uint32_t n) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  const uint32_t q = R.lane_list[idx];
  const uint32_t a0 = T.in_off[q], a1 = T.in_off[q + 1], n_old = R.A.n[q];
  for (uint32_t p = a0; p < a1; ++p) R.head[p] = 0;
  bool empty_left = q == 0, diff = false;
  uint32_t s = 0;
  for (; s < R.K; ++s) {
    double bv;
    uint32_t bl, bp;
    bp_scan(T, R, a0, a1, 1, bv, bl, bp);
    if (empty_left && (bp == kNone || !(bv > 0.0))) {
      empty_left = false;
      diff |= bp_put(R, q, s, n_old, 0.0, 0, kNone, 0);
      continue;
    }
    if (bp == kNone) break;
    const uint32_t h = R.head[bp];
    diff |= bp_put(R, q, s, n_old, bv, bl, T.in_id[bp], h);
    R.head[bp] = (uint16_t)(h + 1);
  }
  R.B.n[q] = s;
  if (diff || s != n_old) R.changed[atomicAdd(&R.counts[2], 1u)] = q;
}

__global__ void __launch_bounds__(kLanes) best_paths_select_wave_kernel(BestPathsTables T, BpRound R, uint32_t n) {
  if (blockIdx.x >= n) return;
  const uint32_t lane = threadIdx.x;
  const uint32_t q = R.wave_list[blockIdx.x];
  const uint32_t a0 = T.in_off[q], a1 = T.in_off[q + 1], n_old = R.A.n[q];
  for (uint32_t p = a0 + lane; p < a1; p += kLanes) R.head[p] = 0;  // (a lane reads only the heads it wrote)
  double bv;
  uint32_t bl, bp;
  bp_scan(T, R, a0 + lane, a1, kLanes, bv, bl, bp);
  bool empty_left = q == 0, diff = false;
  uint32_t s = 0;
  for (; s < R.K; ++s) {
    double v = bv;
    uint32_t l = bl, p = bp;
    bp_wave_best(v, l, p);
    if (empty_left && (p == kNone || !(v > 0.0))) {
      empty_left = false;
      if (lane == 0) diff |= bp_put(R, q, s, n_old, 0.0, 0, kNone, 0);
      continue;
    }
    if (p == kNone) break;
    if (p == bp) {  // the lane that held it: bp is a position of its own, no other lane's
      const uint32_t h = R.head[p];
      diff |= bp_put(R, q, s, n_old, v, l, T.in_id[p], h);
      R.head[p] = (uint16_t)(h + 1);
      bp_scan(T, R, a0 + lane, a1, kLanes, bv, bl, bp);
    }
  }
  const bool any = __any(diff);
  if (lane == 0) {
    R.B.n[q] = s;
    if (any || s != n_old) R.changed[atomicAdd(&R.counts[2], 1u)] = q;
  }
}

// a wavefront per changed state: B's list becomes A's, the destinations of its out-arcs are active in the next round
__global__ void __launch_bounds__(256) best_paths_commit_kernel(BestPathsTables T, BpRound R) {
  const uint32_t i = blockIdx.x * (blockDim.x / kLanes) + threadIdx.x / kLanes, lane = threadIdx.x % kLanes;
  if (i >= R.counts[2]) return;
  const uint32_t q = R.changed[i], n = R.B.n[q];
  for (uint32_t s = lane; s < n; s += kLanes) {
    const size_t e = (size_t)q * R.K + s;
    R.A.val[e] = R.B.val[e];
    R.A.len[e] = R.B.len[e];
    R.A.arc[e] = R.B.arc[e];
    R.A.rank[e] = R.B.rank[e];
  }
  if (lane == 0) R.A.n[q] = n;
  for (uint32_t p = T.out_off[q] + lane; p < T.out_off[q + 1]; p += kLanes) R.mark[T.out_dst[p]] = 1;
}

__global__ void __launch_bounds__(256) best_paths_compact_kernel(BestPathsTables T, BpRound R) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= R.n_states || !R.mark[q]) return;
  R.mark[q] = 0;
  if (T.in_off[q + 1] - T.in_off[q] > R.wave_degree)
    R.wave_list[atomicAdd(&R.counts[1], 1u)] = q;
  else
    R.lane_list[atomicAdd(&R.counts[0], 1u)] = q;
}

// round 0: B's list of state 0 is the empty path, and state 0 is the one changed state
__global__ void best_paths_init_kernel(BpRound R) {
  R.B.val[0] = 0.0;
  R.B.len[0] = 0;
  R.B.arc[0] = kNone;
  R.B.rank[0] = 0;
  R.B.n[0] = 1;
  R.changed[0] = 0;
  R.counts[0] = R.counts[1] = 0;
  R.counts[2] = 1;
}

struct BpReadout {
  uint32_t n, K, final_state, n_states;
  uint64_t n_arcs;
  BpLists A;
  const uint32_t* a_src;
  const double* a_w;
  const uint64_t* path_off;  // [n + 1]
  uint32_t* path;
  double* logw;
  int* err;
};

// one lane per path: written from the end with the known length, the reported weight added on the way
__global__ void __launch_bounds__(256) best_paths_readout_kernel(BpReadout P) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= P.n) return;
  uint32_t q = P.final_state, r = idx;
  uint32_t* out = P.path + P.path_off[idx];
  double w = 0.0;
  for (uint64_t k = P.path_off[idx + 1] - P.path_off[idx]; k-- > 0;) {
    const size_t e = (size_t)q * P.K + r;
    const uint32_t arc = P.A.arc[e];
    if (r >= P.A.n[q] || arc >= P.n_arcs || P.A.len[e] != k + 1 || P.A.rank[e] >= P.K) {
      atomicOr(P.err, kErrWalk);
      return;
    }
    out[k] = arc;
    w = P.a_w[arc] + w;
    r = P.A.rank[e];
    q = P.a_src[arc];
  }
  if (q != 0 || r >= P.A.n[0] || P.A.arc[(size_t)r] != kNone) atomicOr(P.err, kErrWalk);  // (it ends at the empty path)
  P.logw[idx] = w;
}

int upload_best_paths_tables(carmel_hip_decoder* d) {
  if (d->bp_ready) return CARMEL_HIP_OK;
  const BestPathsTablesHost H = build_best_paths_tables(d->n_states, d->src, d->dst, d->logw);  // (lives until the copies are made)
  d->bp_cycle_arc = positive_cycle_arc(H, d->src, d->dst, d->logw);
  if (d->bp_cycle_arc < 0) {
    hipStream_t s = d->stream;
    HIPCHK(d->bp_u32[0].upload(H.in_off, s));
    HIPCHK(d->bp_u32[1].upload(H.in_src, s));
    HIPCHK(d->bp_u32[2].upload(H.in_id, s));
    HIPCHK(d->bp_f64.upload(H.in_w, s));
    HIPCHK(d->bp_u32[3].upload(H.out_off, s));
    HIPCHK(d->bp_u32[4].upload(H.out_dst, s));
    HIPCHK(hipStreamSynchronize(s));
    d->BP = BestPathsTables{d->bp_u32[0].p, d->bp_u32[1].p, d->bp_u32[2].p, d->bp_f64.p, d->bp_u32[3].p, d->bp_u32[4].p};
    d->bp_n_in = H.in_src.size();
  }
  d->bp_ready = true;
  return CARMEL_HIP_OK;
}

int alloc_lists(BpLists& L, DevBuf<double>& val, DevBuf<uint32_t>& len, DevBuf<uint32_t>& arc, DevBuf<uint16_t>& rank,
                DevBuf<uint32_t>& n, size_t entries, size_t states) {
  HIPCHK(val.alloc(entries));
  HIPCHK(len.alloc(entries));
  HIPCHK(arc.alloc(entries));
  HIPCHK(rank.alloc(entries));
  HIPCHK(n.alloc(states));
  L = BpLists{val.p, len.p, arc.p, rank.p, n.p};
  return CARMEL_HIP_OK;
}
}  // namespace

extern "C" {

int carmel_hip_decoder_best_paths(carmel_hip_decoder* d, uint32_t k, uint64_t* n_paths) {
  const std::string who = "carmel_hip_decoder_best_paths";
  if (!d || !n_paths) return fail(CARMEL_HIP_ERR_ARG, who + ": bad argument");
  if (k < 1 || k > kMaxK) return fail(CARMEL_HIP_ERR_ARG, who + ": k must be in 1 .. " + std::to_string(kMaxK));
  if ((uint64_t)d->n_states * k >= (1ull << 31)) return fail(CARMEL_HIP_ERR_ARG, who + ": states x k must be below 2^31");
  HIPCHK(hipSetDevice(d->device));
  if (const int rc = upload_best_paths_tables(d)) return rc;
  if (d->bp_cycle_arc >= 0) {
    const int64_t a = d->bp_cycle_arc;
    return fail(CARMEL_HIP_ERR_UNSUPPORTED, who + ": arc " + std::to_string(a) + " (" + std::to_string(d->src[a]) + " -> " +
                                                std::to_string(d->dst[a]) + ") has a weight above 1 and lies on a cycle: the best path is undefined");
  }
  hipStream_t s = d->stream;
  const uint32_t Q = d->n_states;
  const size_t entries = (size_t)Q * k;
  uint32_t wave_degree = kWaveDegree;
  if (const char* v = lib_opt("best_paths_wave_degree")) wave_degree = (uint32_t)std::min<unsigned long long>(std::strtoull(v, nullptr, 10), kNone);
  DevBuf<double> a_val, b_val, d_logw;
  DevBuf<uint32_t> a_len, a_arc, a_n, b_len, b_arc, b_n, lane_list, wave_list, changed, counts, d_path;
  DevBuf<uint16_t> a_rank, b_rank, head;
  DevBuf<uint8_t> mark;
  DevBuf<uint64_t> d_poff;
  DevBuf<int> d_err;
  BpRound R{k, Q, wave_degree};
  if (const int rc = alloc_lists(R.A, a_val, a_len, a_arc, a_rank, a_n, entries, Q)) return rc;
  if (const int rc = alloc_lists(R.B, b_val, b_len, b_arc, b_rank, b_n, entries, Q)) return rc;
  HIPCHK(head.alloc(std::max<uint64_t>(d->bp_n_in, 1)));
  HIPCHK(mark.alloc(Q));
  HIPCHK(lane_list.alloc(Q));
  HIPCHK(wave_list.alloc(Q));
  HIPCHK(changed.alloc(Q));
  HIPCHK(counts.alloc(3));
  HIPCHK(d_err.alloc(1));
  R.head = head.p;
  R.mark = mark.p;
  R.lane_list = lane_list.p;
  R.wave_list = wave_list.p;
  R.changed = changed.p;
  R.counts = counts.p;
  HIPCHK(hipMemsetAsync(a_n.p, 0, Q * sizeof(uint32_t), s));
  HIPCHK(hipMemsetAsync(mark.p, 0, Q, s));
  HIPCHK(hipMemsetAsync(d_err.p, 0, sizeof(int), s));
  DecodeChunk c{d};
  c.ms = 0;
  const uint32_t qb = (Q + 255) / 256;
  uint32_t h_counts[3] = {0, 0, 0};
  // round 0, then the states that state 0's arcs enter
  if (const int rc = c.begin()) return rc;
  best_paths_init_kernel<<<1, 1, 0, s>>>(R);
  best_paths_commit_kernel<<<1, 256, 0, s>>>(d->BP, R);
  best_paths_compact_kernel<<<qb, 256, 0, s>>>(d->BP, R);
  if (const int rc = c.end()) return rc;
  HIPCHK(hipMemcpyAsync(h_counts, counts.p, sizeof h_counts, hipMemcpyDeviceToHost, s));
  if (const int rc = c.wait()) return rc;
  const uint64_t cap = (uint64_t)k * Q + 1;
  uint64_t rounds = 0, selected = 0;
  while (h_counts[0] + h_counts[1]) {
    const uint32_t n_lane = h_counts[0], n_wave = h_counts[1];
    if (n_lane > Q || n_wave > Q - n_lane) return fail(CARMEL_HIP_ERR_STATE, who + ": inconsistent worklist");
    if (++rounds > cap) return fail(CARMEL_HIP_ERR_STATE, who + ": did not converge in " + std::to_string(cap) + " rounds");
    selected += (uint64_t)n_lane + n_wave;
    if (const int rc = c.begin()) return rc;
    HIPCHK(hipMemsetAsync(counts.p, 0, 3 * sizeof(uint32_t), s));
    if (n_lane) best_paths_select_lane_kernel<<<(n_lane + 255) / 256, 256, 0, s>>>(d->BP, R, n_lane);
    if (n_wave) best_paths_select_wave_kernel<<<n_wave, kLanes, 0, s>>>(d->BP, R, n_wave);
    best_paths_commit_kernel<<<(n_lane + n_wave + 3) / 4, 256, 0, s>>>(d->BP, R);
    best_paths_compact_kernel<<<qb, 256, 0, s>>>(d->BP, R);
    if (const int rc = c.end()) return rc;
    HIPCHK(hipMemcpyAsync(h_counts, counts.p, sizeof h_counts, hipMemcpyDeviceToHost, s));
    if (const int rc = c.wait()) return rc;
  }
  // the read-out of list(final)
  uint32_t n = 0;
  HIPCHK(hipMemcpyAsync(&n, a_n.p + d->final_state, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (n > k) return fail(CARMEL_HIP_ERR_STATE, who + ": inconsistent list");
  std::vector<uint32_t> len(n);
  if (n) HIPCHK(hipMemcpyAsync(len.data(), a_len.p + (size_t)d->final_state * k, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::vector<double> r_logw(n, 0.0);
  std::vector<uint64_t> r_off(n + 1, 0);
  for (uint32_t p = 0; p < n; ++p) {
    if (len[p] > rounds) return fail(CARMEL_HIP_ERR_STATE, who + ": inconsistent list");
    r_off[p + 1] = r_off[p] + len[p];
  }
  std::vector<uint32_t> r_arcs(r_off[n]);
  if (n) {
    int err = 0;
    HIPCHK(d_poff.upload(r_off, s));
    HIPCHK(d_path.alloc(std::max<uint64_t>(r_off[n], 1)));
    HIPCHK(d_logw.alloc(n));
    const BpReadout P{n, k, d->final_state, Q, d->n_arcs, R.A, d->a_src.p, d->a_w.p, d_poff.p, d_path.p, d_logw.p, d_err.p};
    if (const int rc = c.begin()) return rc;
    best_paths_readout_kernel<<<(n + 255) / 256, 256, 0, s>>>(P);
    if (const int rc = c.end()) return rc;
    if (r_off[n]) HIPCHK(hipMemcpyAsync(r_arcs.data(), d_path.p, r_off[n] * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(r_logw.data(), d_logw.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    if (const int rc = c.wait()) return rc;
    if (err) return fail(CARMEL_HIP_ERR_STATE, who + ": inconsistent read-out");
  }
  d->kb_logw.swap(r_logw);
  d->kb_off.swap(r_off);
  d->kb_arcs.swap(r_arcs);
  d->last_ms = c.ms;
  d->bp_rounds = (uint32_t)rounds;
  d->bp_selected = selected;
  *n_paths = n;
  return CARMEL_HIP_OK;
}

int carmel_hip_decoder_best_paths_stats(carmel_hip_decoder* d, uint32_t* rounds, uint64_t* states_selected) {
  if (!d || !rounds || !states_selected) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decoder_best_paths_stats: bad argument");
  *rounds = d->bp_rounds;
  *states_selected = d->bp_selected;
  return CARMEL_HIP_OK;
}

}  // extern "C"
