// decode_kbest.hip — batch k-best decoding (carmel -b -k n: print_kbest / WFST::visit_kbest(k, ...), carmel.cc:379-397,
// fst.h:791, kbest.h) of many lines against one (composed) transducer: the trellis of decode.hip with an ordered LIST of up to K
// values per (line position i, state q) instead of one value.  Tables, handle and constants are decode.hpp's.
//
// A derivation of a line is a path of the machine from state 0 to the final state whose matched-side symbols (without *e*) spell
// the line and that uses no arc of weight zero; two derivations differ if their arc-id sequences differ (equal printed strings
// are not merged, as in the reference).  Its VALUE is its arcs' weights added in path order from the start, ((0 + w1) + w2) + ...,
// the trellis value the 1-best kernel chooses by.  A line gets its min(K, number of derivations) best derivations, greatest
// value first.
//
// A candidate at node (i, q) is (arc a into q, rank r in the list of a's source node) with value list[src][r] + w(a); the source
// node is (i - 1, src) for a matched arc and (i, src) for an epsilon arc.  Candidates are ordered by
//   value, descending; then matched arcs before epsilon arcs; then arc id, ascending; then r, ascending
// and the node's list is the first K of them.  The order is total, so the lists do not depend on lane count, scheduling, chunking
// or the memory tier, and with K = 1 it is decode.hip's tie rule: rank 0 is the path carmel_hip_decode returns.
//
// Selection (kb_select): one lane owns a node and fills its list slot by slot.  It keeps no array per rank or per arc (K is a
// run-time value; such an array would live in scratch memory): a source list is sorted and rounding is monotone, so an arc's
// candidates are in candidate order by r, and the arc's next candidate is the first r whose candidate comes AFTER the one picked
// last -- found by bisecting the source list against the last picked key (kb_next).  A slot costs (arcs into q) x log2 K reads.
//
// Rows: a row is |Q| K doubles, a state's list padded with -inf (no value is -inf: arcs of weight zero are dropped, so the
// length of a list is where its -inf begin and no count is stored).  The two rows are in LDS when 16 |Q| K bytes fit 64 KiB
// (|Q| K <= 4096), otherwise in a global buffer per line; option decode_lds=0 forces the global tier.
//
// Order within a position: first the nodes that no epsilon arc enters (one lane per destination segment of the line's symbol);
// then, level by level, the nodes that epsilon arcs enter: such a node selects among its matched arcs (sources in the previous
// row) AND its epsilon arcs (sources in the same row, of strictly lower level, final since the barrier that ended their level) in
// one pass into its own, still empty, list.  Nothing is merged in place and no lane reads a list that another is writing; the
// barriers are the 1-best kernel's, one per level.  Only acyclic epsilon subgraphs have levels: a cyclic one is refused for K > 1.
//
// Back-pointers: per (i, q, rank) the arc id (u32) and the predecessor's rank (u16), two arrays of (n + 1) |Q| K entries per
// line.  The walk (one lane per (line, rank)) follows them from (n, final, j) to (0, 0, 0), once to count a path's arcs and add
// their weights from the END, w1 + (w2 + (... + (wn + 0))) -- the weight reported, as by carmel_hip_decode -- and once to write
// the arcs in path order.  The lists are ordered by the path-order value, so a line's reported weights may fail to be monotone in
// the last bit.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>
#include <string>
#include <vector>
#include "decode.hpp"
#include "engine.hpp"

namespace {
constexpr uint32_t kMaxK = 1024;
constexpr uint64_t kEpsTag = 1ull << 32;  // a candidate's tag: (0 matched, 1 epsilon) << 32 | arc id

struct KbLines {
  const uint64_t* off;      // chunk-local CSR of the lines' symbols
  const uint32_t* sym;
  const uint32_t* order;    // launch order: chunk-local line index of block b
  const uint64_t* bp_off;   // [n + 1]: each line's (len + 1) x |Q| x K back-pointer slots
  uint32_t* bp_arc;
  uint16_t* bp_rank;
  double* rows;             // global tier: 2 |Q| K doubles per line (nullptr in the LDS tier)
  uint32_t* n_paths;        // [n]: the length of the final node's list
  const uint8_t* eps_in;    // [|Q|]: an epsilon arc enters the state
  uint32_t K;
};

// the first rank r of the source list S (sorted, padded with -inf) whose candidate (S[r] + w, tag, r) comes after the candidate
// picked last, (vl, tagl, rl); K if none does.  "After" is monotone in r: S is non-increasing and so is S[r] + w.
__device__ inline uint32_t kb_next(const double* S, double w, uint32_t K, uint64_t tag, double vl, uint64_t tagl, uint32_t rl) {
  uint32_t lo = 0, hi = K;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const double v = S[mid] + w;
    if (v < vl || (v == vl && (tag > tagl || (tag == tagl && mid > rl))))
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

// fill one node's list: the first K candidates of the matched arcs [m0, m1) (sources in row `prev`) and the epsilon arcs [e0, e1)
// (sources in row `same`), into out / oarc / orank (the node's K slots)
__device__ void kb_select(const DecodeTables& T, uint32_t K, const double* prev, uint32_t m0, uint32_t m1, const double* same,
                          uint32_t e0, uint32_t e1, double* out, uint32_t* oarc, uint16_t* orank) {
  const double ninf = -std::numeric_limits<double>::infinity();
  double vl = 0.0;  // the candidate picked last: (vl, tagl, rl), from slot 1 on
  uint64_t tagl = 0;
  uint32_t rl = 0;
  for (uint32_t j = 0; j < K; ++j) {
    double bv = ninf;
    uint64_t btag = 0;
    uint32_t br = 0;
    for (uint32_t k = m0; k < m1; ++k) {  // (arc-id order: of equal values the first seen stays)
      const double* S = prev + (size_t)T.m_src[k] * K;
      const double w = T.m_w[k];
      const uint64_t tag = T.m_id[k];
      const uint32_t r = j ? kb_next(S, w, K, tag, vl, tagl, rl) : 0;  // (slot 0: every arc's first)
      if (r < K) {
        const double v = S[r] + w;
        if (v > bv) {
          bv = v;
          btag = tag;
          br = r;
        }
      }
    }
    for (uint32_t k = e0; k < e1; ++k) {
      const double* S = same + (size_t)T.e_src[k] * K;
      const double w = T.e_w[k];
      const uint64_t tag = kEpsTag | T.e_id[k];
      const uint32_t r = j ? kb_next(S, w, K, tag, vl, tagl, rl) : 0;  // (slot 0: every arc's first)
      if (r < K) {
        const double v = S[r] + w;
        if (v > bv) {
          bv = v;
          btag = tag;
          br = r;
        }
      }
    }
    if (!(bv > ninf)) break;
    out[j] = bv;
    oarc[j] = (uint32_t)btag;
    orank[j] = (uint16_t)br;
    vl = bv;
    tagl = btag;
    rl = br;
  }
}

// the nodes of one position that epsilon arcs enter, level by level; [g0, g1) are the segments of the position's symbol (empty at
// position 0, where `skip0` keeps state 0's initial list: an epsilon path into state 0 at position 0 would close a cycle)
__device__ void kb_close(const DecodeTables& T, uint32_t K, const double* prev, uint32_t g0, uint32_t g1, double* row,
                         uint32_t* arc_r, uint16_t* rank_r, int lane, bool skip0) {
  for (uint32_t L = 0; L < T.n_levels; ++L) {
    for (uint32_t e = T.lvl_ent[L] + lane; e < T.lvl_ent[L + 1]; e += kLanes) {
      const uint32_t q = T.ent_dst[e];
      if (skip0 && q == 0) continue;
      uint32_t lo = g0, hi = g1;  // the segment of destination q, if the symbol has one (seg_dst ascends within a symbol)
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (T.seg_dst[mid] < q)
          lo = mid + 1;
        else
          hi = mid;
      }
      const bool has = lo < g1 && T.seg_dst[lo] == q;
      const uint32_t m0 = has ? T.seg_arc[lo] : 0, m1 = has ? T.seg_arc[lo + 1] : 0;
      kb_select(T, K, prev, m0, m1, row, T.ent_arc[e], T.ent_arc[e + 1], row + (size_t)q * K, arc_r + (size_t)q * K,
                rank_r + (size_t)q * K);
    }
    __syncthreads();
  }
}

template <bool kLds>
__global__ void __launch_bounds__(kLanes) kbest_trellis_kernel(DecodeTables T, KbLines D) {
  extern __shared__ double lds_rows[];
  const int lane = threadIdx.x;
  const uint32_t line = D.order[blockIdx.x];
  const uint32_t K = D.K;
  const size_t QK = (size_t)T.n_states * K;
  double* cur = kLds ? lds_rows : D.rows + (size_t)line * 2 * QK;
  double* nxt = cur + QK;
  const uint64_t s0 = D.off[line];
  const uint32_t n = (uint32_t)(D.off[line + 1] - s0);
  uint32_t* bp_arc = D.bp_arc + D.bp_off[line];
  uint16_t* bp_rank = D.bp_rank + D.bp_off[line];
  const double ninf = -std::numeric_limits<double>::infinity();
  for (size_t s = lane; s < QK; s += kLanes) cur[s] = s == 0 ? 0.0 : ninf;
  if (lane == 0) {  // (0, start, rank 0): where every walk ends
    bp_arc[0] = kNone;
    bp_rank[0] = 0;
  }
  __syncthreads();
  kb_close(T, K, cur, 0, 0, cur, bp_arc, bp_rank, lane, true);
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t* arc_n = bp_arc + (size_t)(i + 1) * QK;
    uint16_t* rank_n = bp_rank + (size_t)(i + 1) * QK;
    for (size_t s = lane; s < QK; s += kLanes) nxt[s] = ninf;
    __syncthreads();
    const uint32_t x = D.sym[s0 + i];
    const bool known = x < T.n_syms;  // (a symbol no arc matches leaves the row empty: no derivation)
    const uint32_t g0 = known ? T.sym_seg[x] : 0, g1 = known ? T.sym_seg[x + 1] : 0;
    for (uint32_t g = g0 + lane; g < g1; g += kLanes) {
      const uint32_t q = T.seg_dst[g];
      if (D.eps_in[q]) continue;  // selected with its epsilon arcs, at its level
      kb_select(T, K, cur, T.seg_arc[g], T.seg_arc[g + 1], nxt, 0, 0, nxt + (size_t)q * K, arc_n + (size_t)q * K,
                rank_n + (size_t)q * K);
    }
    __syncthreads();
    kb_close(T, K, cur, g0, g1, nxt, arc_n, rank_n, lane, false);
    double* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (lane == 0) {
    const double* F = cur + (size_t)T.final_state * K;
    uint32_t c = 0;
    while (c < K && F[c] > ninf) ++c;
    D.n_paths[line] = c;
  }
}

// one lane per (line, rank j): slot line * K + j, idle if j >= n_paths[line].  Walks the back-pointers from (n, final, j) to
// (0, start, 0): kWrite = false counts the path's arcs into len[slot] and adds their weights from the end into logw[slot];
// kWrite = true writes the arcs in path order at path[path_off[slot] ..)
template <bool kWrite>
__global__ void kbest_walk_kernel(uint32_t n_lines, uint32_t n_states, uint32_t K, uint32_t final_state, uint64_t n_arcs,
                                  const uint64_t* off, const uint64_t* bp_off, const uint32_t* bp_arc, const uint16_t* bp_rank,
                                  const uint32_t* n_paths, const uint32_t* a_src, const uint8_t* a_eps, const double* a_w,
                                  uint32_t* len, double* logw, const uint64_t* path_off, uint32_t* path, int* err) {
  const uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= (uint64_t)n_lines * K) return;
  const uint32_t line = (uint32_t)(slot / K);
  uint32_t r = (uint32_t)(slot % K);
  if (r >= n_paths[line]) return;
  uint32_t i = (uint32_t)(off[line + 1] - off[line]), q = final_state;
  const uint32_t* ba = bp_arc + bp_off[line];
  const uint16_t* br = bp_rank + bp_off[line];
  const uint64_t cap = (uint64_t)(i + 1) * n_states;  // no path of the trellis is longer
  const uint32_t n_path = kWrite ? len[slot] : 0;
  uint32_t steps = 0;
  double w = 0.0;
  while (true) {
    const size_t at = ((size_t)i * n_states + q) * K + r;
    const uint32_t a = ba[at];
    if (a == kNone) break;
    if (a >= n_arcs || steps >= cap || (kWrite && steps >= n_path) || (!a_eps[a] && i == 0) || br[at] >= K) {
      atomicOr(err, kErrWalk);
      return;
    }
    ++steps;
    if (kWrite) path[path_off[slot] + n_path - steps] = a;
    w = a_w[a] + w;
    q = a_src[a];
    r = br[at];
    if (!a_eps[a]) --i;
  }
  if (i != 0 || q != 0 || r != 0) atomicOr(err, kErrWalk);
  if (!kWrite) {
    len[slot] = steps;
    logw[slot] = w;
  }
}
}  // namespace

extern "C" {

int carmel_hip_decode_kbest(carmel_hip_decoder* d, uint32_t k, uint64_t n_lines, const uint64_t* off, const uint32_t* sym,
                            uint64_t* line_paths) {
  if (!d || !off || !line_paths || (off[n_lines] && !sym)) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decode_kbest: bad argument");
  if (k < 1 || k > kMaxK) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decode_kbest: k must be in 1 .. 1024");
  for (uint64_t l = 0; l < n_lines; ++l)
    if (off[l + 1] < off[l] || off[l + 1] - off[l] >= kNone)
      return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decode_kbest: bad line offsets");
  if (d->eps_cyclic) {
    if (k > 1)
      return fail(CARMEL_HIP_ERR_UNSUPPORTED,
                  "carmel_hip_decode_kbest: the epsilon arcs of the matched side have a cycle; k-best paths over an epsilon cycle "
                  "are not supported (k = 1 is)");
    // k = 1 over a cyclic epsilon subgraph is carmel_hip_decode, best_path_has_cycle included
    std::vector<double> best(n_lines);
    std::vector<uint64_t> poff(n_lines + 1);
    const int rc = carmel_hip_decode(d, n_lines, off, sym, best.data(), poff.data());
    if (rc) return rc;
    d->kb_logw.clear();
    d->kb_off.assign(1, 0);
    line_paths[0] = 0;
    for (uint64_t l = 0; l < n_lines; ++l) {
      const bool has = best[l] > -std::numeric_limits<double>::infinity();
      if (has) {
        d->kb_logw.push_back(best[l]);
        d->kb_off.push_back(poff[l + 1]);
      }
      line_paths[l + 1] = line_paths[l] + (has ? 1 : 0);
    }
    d->kb_arcs = d->paths;
    return CARMEL_HIP_OK;
  }
  HIPCHK(hipSetDevice(d->device));
  hipStream_t s = d->stream;
  const uint32_t Q = d->n_states, K = k;
  const uint64_t QK = (uint64_t)Q * K;
  const bool lds = QK <= kLdsStates && !lib_opt_off("decode_lds");
  // lines go in chunks, in line order, whose back-pointers (and global-tier rows) fit the budget ("decode_chunk_bytes", default
  // 1 GiB; a single line larger than it goes alone): 6 bytes per (position, state, rank)
  uint64_t budget = 1ull << 30;
  if (const char* v = lib_opt("decode_chunk_bytes")) budget = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10));
  auto line_bytes = [&](uint64_t l) { return (off[l + 1] - off[l] + 1) * QK * 6ull + (lds ? 0 : 16ull * QK); };
  std::vector<double> r_logw;
  std::vector<uint64_t> r_off(1, 0);
  std::vector<uint32_t> r_arcs;
  line_paths[0] = 0;
  float total_ms = 0;
  DevBuf<uint64_t> d_off, d_bpoff, d_poff;
  DevBuf<uint32_t> d_sym, d_order, d_bparc, d_np, d_len, d_path;
  DevBuf<uint16_t> d_bprank;
  DevBuf<double> d_rows, d_logw;
  DevBuf<int> d_err;
  HIPCHK(d_err.alloc(1));
  for (uint64_t lo = 0; lo < n_lines;) {
    uint64_t hi = lo + 1, bytes = line_bytes(lo);
    while (hi < n_lines && (hi - lo + 1) * K <= (1u << 24) && bytes + line_bytes(hi) <= budget) bytes += line_bytes(hi++);
    const uint32_t n = (uint32_t)(hi - lo);
    const uint64_t n_slots = (uint64_t)n * K;
    std::vector<uint64_t> h_off(n + 1), h_bpoff(n + 1);
    for (uint32_t l = 0; l <= n; ++l) h_off[l] = off[lo + l] - off[lo];
    h_bpoff[0] = 0;
    for (uint32_t l = 0; l < n; ++l) h_bpoff[l + 1] = h_bpoff[l] + (h_off[l + 1] - h_off[l] + 1) * QK;
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return h_off[a + 1] - h_off[a] > h_off[b + 1] - h_off[b]; });
    HIPCHK(d_off.upload(h_off, s));
    HIPCHK(d_bpoff.upload(h_bpoff, s));
    const std::vector<uint32_t> h_sym(sym + off[lo], sym + off[hi]);  // (named: the copy is asynchronous)
    HIPCHK(d_sym.upload(h_sym, s));
    HIPCHK(d_order.upload(order, s));
    HIPCHK(d_bparc.alloc(h_bpoff[n]));
    HIPCHK(d_bprank.alloc(h_bpoff[n]));
    if (!lds) HIPCHK(d_rows.alloc((size_t)n * 2 * QK));
    HIPCHK(d_np.alloc(n));
    HIPCHK(d_len.alloc(n_slots));
    HIPCHK(d_logw.alloc(n_slots));
    HIPCHK(hipMemsetAsync(d_err.p, 0, sizeof(int), s));
    KbLines D{d_off.p, d_sym.p, d_order.p, d_bpoff.p, d_bparc.p, d_bprank.p, lds ? nullptr : d_rows.p, d_np.p, d->eps_in.p, K};
    HIPCHK(hipEventRecord(d->ev0, s));
    if (lds)
      kbest_trellis_kernel<true><<<n, kLanes, 16 * (size_t)QK, s>>>(d->T, D);
    else
      kbest_trellis_kernel<false><<<n, kLanes, 0, s>>>(d->T, D);
    HIPCHK(hipGetLastError());
    const uint32_t wb = (uint32_t)((n_slots + 255) / 256);
    kbest_walk_kernel<false><<<wb, 256, 0, s>>>(n, Q, K, d->final_state, d->n_arcs, d_off.p, d_bpoff.p, d_bparc.p, d_bprank.p,
                                                d_np.p, d->a_src.p, d->a_eps.p, d->a_w.p, d_len.p, d_logw.p, nullptr, nullptr,
                                                d_err.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(d->ev1, s));
    std::vector<uint32_t> np(n), len(n_slots);
    std::vector<double> lw(n_slots);
    int err = 0;
    HIPCHK(hipMemcpyAsync(np.data(), d_np.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(len.data(), d_len.p, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(lw.data(), d_logw.p, n_slots * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, d->ev0, d->ev1));
    total_ms += ms;
    if (err) return fail(CARMEL_HIP_ERR_STATE, "carmel_hip_decode_kbest: inconsistent back-pointers");
    // the slots of ranks a line does not have are empty paths: the arcs come back compact and in (line, rank) order
    std::vector<uint64_t> h_poff(n_slots + 1, 0);
    for (uint32_t l = 0; l < n; ++l) {
      if (np[l] > K) return fail(CARMEL_HIP_ERR_STATE, "carmel_hip_decode_kbest: inconsistent back-pointers");
      for (uint32_t j = 0; j < K; ++j) {
        const uint64_t at = (uint64_t)l * K + j;
        h_poff[at + 1] = h_poff[at] + (j < np[l] ? len[at] : 0);
      }
    }
    const uint64_t base = r_arcs.size();
    for (uint32_t l = 0; l < n; ++l) {
      for (uint32_t j = 0; j < np[l]; ++j) {
        const uint64_t at = (uint64_t)l * K + j;
        r_logw.push_back(lw[at]);
        r_off.push_back(base + h_poff[at + 1]);
      }
      line_paths[lo + l + 1] = line_paths[lo + l] + np[l];
    }
    if (h_poff[n_slots]) {
      HIPCHK(d_poff.upload(h_poff, s));
      HIPCHK(d_path.alloc(h_poff[n_slots]));
      HIPCHK(hipEventRecord(d->ev0, s));
      kbest_walk_kernel<true><<<wb, 256, 0, s>>>(n, Q, K, d->final_state, d->n_arcs, d_off.p, d_bpoff.p, d_bparc.p, d_bprank.p,
                                                 d_np.p, d->a_src.p, d->a_eps.p, d->a_w.p, d_len.p, d_logw.p, d_poff.p, d_path.p,
                                                 d_err.p);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(d->ev1, s));
      r_arcs.resize(base + h_poff[n_slots]);
      HIPCHK(hipMemcpyAsync(r_arcs.data() + base, d_path.p, h_poff[n_slots] * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      HIPCHK(hipEventElapsedTime(&ms, d->ev0, d->ev1));
      total_ms += ms;
      if (err) return fail(CARMEL_HIP_ERR_STATE, "carmel_hip_decode_kbest: inconsistent back-pointers");
    }
    lo = hi;
  }
  d->kb_logw.swap(r_logw);
  d->kb_off.swap(r_off);
  d->kb_arcs.swap(r_arcs);
  d->last_ms = total_ms;
  return CARMEL_HIP_OK;
}

int carmel_hip_decoder_kbest_size(carmel_hip_decoder* d, uint64_t* n_paths, uint64_t* n_arcs) {
  if (!d || !n_paths || !n_arcs) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decoder_kbest_size: bad argument");
  *n_paths = d->kb_logw.size();
  *n_arcs = d->kb_arcs.size();
  return CARMEL_HIP_OK;
}

int carmel_hip_decoder_get_kbest(carmel_hip_decoder* d, double* path_logw, uint64_t* path_off, uint32_t* arcs) {
  if (!d || !path_off || (!path_logw && !d->kb_logw.empty()) || (!arcs && !d->kb_arcs.empty()))
    return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decoder_get_kbest: bad argument");
  if (!d->kb_logw.empty()) std::memcpy(path_logw, d->kb_logw.data(), d->kb_logw.size() * sizeof(double));
  if (!d->kb_arcs.empty()) std::memcpy(arcs, d->kb_arcs.data(), d->kb_arcs.size() * sizeof(uint32_t));
  path_off[0] = 0;
  for (size_t p = 1; p < d->kb_off.size(); ++p) path_off[p] = d->kb_off[p];
  return CARMEL_HIP_OK;
}

}  // extern "C"
