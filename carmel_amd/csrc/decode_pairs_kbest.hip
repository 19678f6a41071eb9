// decode_pairs_kbest.hip — batch pair k-best alignments (carmel --post-b=FILE with -k n: the pair's composition of
// carmel.cc:569-597 handed to print_kbest): for many pairs (x, y) against one (composed) transducer, the K best derivations of
// every pair.  It is to carmel_hip_decode_pairs what decode_kbest.hip is to the one-sided 1-best: the anti-diagonal trellis of
// decode_pairs.hip with an ordered LIST of up to K values per (matched position i, other position j, state q) instead of one
// value.  Pair, derivation, matched side, the four kinds of arc (MM, M0, 0M, 00), the 00 levels, dropped zero-weight arcs, unknown
// symbols: decode_pairs.hip's.
//
// Two derivations differ if their arc-id sequences differ.  A derivation's VALUE is its arcs' weights added in path order from
// the start, ((0 + w1) + w2) + ..., in f64.  A pair gets its min(K, number of derivations) best derivations, greatest value first,
// 1 <= K <= 1024.
//
// A candidate at node (i, j, q) is (arc a into q, rank r in the list of a's source node) with value list[source][r] + w(a); the
// source node is (i - 1, j - 1, src) for an MM arc, (i - 1, j, src) for M0, (i, j - 1, src) for 0M and (i, j, src) for 00.
// Candidates are ordered by
//   value, descending; then arcs whose matched symbol is not epsilon (MM, M0) before arcs whose matched symbol is epsilon (0M,
//   00); then arc id, ascending; then r, ascending
// and the node's list is the first K of them.  The order is total, so the lists do not depend on lane count, launch order,
// chunking or the memory tier, and with K = 1 it is BestAcc's rule (decode_pairs.hip): rank 0 is the very path and weight
// carmel_hip_decode_pairs returns.  Node (0, 0, start) keeps its initial list [0.0, -inf, ...], as KbNode does: anything that
// enters it would close a 00 cycle, which is refused before any launch.  A 0M or M0 self-loop is an ordinary arc for every K (an
// insertion loop *e*:y is an epsilon cycle of the matched side, which carmel_hip_decode_kbest refuses for K > 1; here it advances
// j and its source is on the diagonal before).
//
// Trellis (pair_kbest_trellis_kernel): one 64-lane workgroup per pair walks d = 0 .. n + m with pair_trellis_kernel's phases and
// barriers (decode_pairs_trellis.hpp, whose Diag it shares; the node enumeration is restated here so that the objects of the
// other pair entry points keep their kernels byte for byte): clear; barrier; the nodes no matched-side-epsilon arc enters;
// barrier; then 00 level by 00 level, a barrier after each.  One lane owns a node and fills its list ONCE, in one pass over its
// matched arcs and then its epsilon arcs, into its own still empty list (kb_pair_select); nothing is merged in place and no lane
// reads a node another is writing.  A diagonal holds (min(n, m) + 1) |Q| K doubles, each list padded with -inf (no value is
// -inf, so no count is stored).  The three diagonals are in LDS when 3 (min(n, m) + 1) |Q| K <= 8192 doubles (64 KiB) for the
// largest pair of the call, otherwise in a global buffer per pair; option decode_lds=0 forces the global tier.
//
// Selection: decode_kbest.hip's, with the arc's source list chosen by the arc's class and an arc whose other symbol fails its
// test skipped.  No array per rank or per arc is kept (K is a run-time value; such an array would live in scratch memory): an
// arc's next candidate is found by bisecting its source list against the candidate picked last (kb_next,
// decode_kbest_list.hpp).  A slot costs (arcs into q) x log2 K reads.
//
// Back-pointers: per (i, j, q, r) the arc id (u32, preset to kNone) and the source's rank (u16), at slot
// ((i (m + 1) + j) |Q| + q) K + r of two global arrays: 6 (n + 1)(m + 1)|Q| K bytes a pair, beside its symbols and, in the global
// tier, 24 (min(n, m) + 1)|Q| K bytes of diagonals.  Chunks hold at most 2^24 / K pairs, so at most 2^24 (pair, rank) slots.
//
// The walk (pair_kbest_walk_kernel): one lane per (pair, rank) follows the back-pointers from (n, m, final, rank) to (0, 0, start,
// 0) as decode_pairs.hip's walk does with the rank carried along; once to count the arcs and add the reported weight, once to
// write the path.  It checks the arc range, i == 0 / j == 0 against the arc's flags, a step cap of (n + m + 1)(levels + 1), source
// rank < K and the arrival.  The weight REPORTED for a path is its arcs added from the END, w1 + (w2 + (... + (wn + 0))), as
// everywhere else; the lists are ordered by the path-order value, so a pair's reported weights may fail to be monotone in the
// last bit.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <limits>
#include <string>
#include <vector>
#include "decode_kbest_list.hpp"
#include "decode_pairs_trellis.hpp"

namespace {
struct PairKbOut {
  const uint64_t* bp_off;  // [n + 1]: each pair's (n + 1)(m + 1)|Q| K slots, slot ((i (m + 1) + j) |Q| + q) K + r
  uint32_t* bp_arc;        // preset to kNone
  uint16_t* bp_rank;
  uint32_t* n_paths;  // [n]: how many of its K slots the pair's final node fills
  uint32_t K;
};

// fill node (i, j, q)'s list: the first K candidates of its matched arcs [m0, m1) (none if i = 0) and its epsilon arcs [e0, e1).
// G's diagonals hold K doubles a state; the list goes to the node's own K slots of G.cur, the back-pointers to O
__device__ void kb_pair_select(const DecodeTables& T, const DecodePairTables& P, const Diag& G, const PairKbOut& O, uint32_t pair,
                               uint32_t i, uint32_t j, uint32_t q, uint32_t m0, uint32_t m1, uint32_t e0, uint32_t e1) {
  const double ninf = -std::numeric_limits<double>::infinity();
  const uint32_t K = O.K;
  const size_t QK = (size_t)G.Q * K;
  const uint32_t p = G.by_i ? i : j;
  const bool has_y = j > 0;
  const uint32_t yj = has_y ? G.y[j - 1] : 0;
  double* cell = G.cur + (size_t)p * QK;
  // (i - 1, j - 1) is cell p - 1 of d - 2; (i - 1, j) cell p - 1 or p of d - 1; (i, j - 1) cell p or p - 1 of d - 1
  const double* mm = G.d2 + (size_t)(p ? p - 1 : 0) * QK;
  const double* m0p = G.d1 + (size_t)(G.by_i ? (p ? p - 1 : 0) : p) * QK;
  const double* zm = G.d1 + (size_t)(G.by_i ? p : (p ? p - 1 : 0)) * QK;
  const size_t slot = (((size_t)i * (G.m + 1) + j) * G.Q + q) * K;
  double* out = cell + (size_t)q * K;
  uint32_t* oarc = O.bp_arc + O.bp_off[pair] + slot;
  uint16_t* orank = O.bp_rank + O.bp_off[pair] + slot;
  double vl = 0.0;  // the candidate picked last: (vl, tagl, rl), from slot 1 on
  uint64_t tagl = 0;
  uint32_t rl = 0;
  for (uint32_t s = 0; s < K; ++s) {
    double bv = ninf;
    uint64_t btag = 0;
    uint32_t br = 0;
    for (uint32_t k = m0; k < m1; ++k) {  // (arc-id order: of equal values the first seen stays)
      const uint32_t o = P.m_osym[k];
      if (o != 0 && !(has_y && o == yj)) continue;
      const double* S = (o == 0 ? m0p : mm) + (size_t)T.m_src[k] * K;
      const double w = T.m_w[k];
      const uint64_t tag = T.m_id[k];
      const uint32_t r = s ? kb_next(S, w, K, tag, vl, tagl, rl) : 0;  // (slot 0: every arc's first)
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
      const uint32_t o = P.e_osym[k];
      if (o != 0 && !(has_y && o == yj)) continue;
      const double* S = (o == 0 ? (const double*)cell : zm) + (size_t)P.e_src[k] * K;
      const double w = P.e_w[k];
      const uint64_t tag = kEpsTag | P.e_id[k];
      const uint32_t r = s ? kb_next(S, w, K, tag, vl, tagl, rl) : 0;
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
    out[s] = bv;
    oarc[s] = (uint32_t)btag;
    orank[s] = (uint16_t)br;
    vl = bv;
    tagl = btag;
    rl = br;
  }
}

// pair_trellis_kernel (decode_pairs_trellis.hpp) with K doubles a state: the same diagonals, phases, barriers and node
// enumeration.  eps_in [|Q|]: a matched-side-epsilon arc (of weight > 0) enters the state
template <bool kLds>
__global__ void __launch_bounds__(kLanes) pair_kbest_trellis_kernel(DecodeTables T, DecodePairTables P, PairLines D,
                                                                    const uint8_t* eps_in, PairKbOut O) {
  extern __shared__ double lds_diag[];
  const int lane = threadIdx.x;
  const uint32_t pair = D.order[blockIdx.x];
  const uint32_t Q = T.n_states, K = O.K;
  const uint32_t* x = D.sym + D.off[pair];
  const uint32_t n = (uint32_t)(D.off[pair + 1] - D.off[pair]);
  const uint32_t* y = D.sym2 + D.off2[pair];
  const uint32_t m = (uint32_t)(D.off2[pair + 1] - D.off2[pair]);
  const bool by_i = n <= m;
  const size_t QK = (size_t)Q * K;
  const size_t DQ = (size_t)((by_i ? n : m) + 1) * QK;
  double* base = kLds ? lds_diag : D.rows + D.rows_off[pair];
  const double ninf = -std::numeric_limits<double>::infinity();
  Diag G;
  G.Q = Q;
  G.m = m;
  G.by_i = by_i;
  G.y = y;
  for (uint32_t d = 0; d <= n + m; ++d) {  // (n + m < 2^32 - 1: the entry point checks)
    G.cur = base + (size_t)(d % 3) * DQ;
    G.d1 = base + (size_t)((d + 2) % 3) * DQ;
    G.d2 = base + (size_t)((d + 1) % 3) * DQ;
    const uint32_t ilo = d > m ? d - m : 0, ihi = d < n ? d : n;
    const uint64_t n_cell = (uint64_t)(ihi - ilo) + 1;
    // (0, 0, start) holds its list [0.0, -inf, ...] from the beginning and is never filled again
    for (size_t s = lane; s < DQ; s += kLanes) G.cur[s] = (d == 0 && s == 0) ? 0.0 : ninf;
    __syncthreads();
    // the nodes no epsilon arc enters: one lane per (cell, destination segment of the cell's symbol)
    for (uint64_t t = lane; t < n_cell * P.max_seg; t += kLanes) {
      const uint32_t i = ilo + (uint32_t)(t / P.max_seg), sg = (uint32_t)(t % P.max_seg);
      if (i == 0) continue;
      const uint32_t xi = x[i - 1];
      if (xi >= T.n_syms) continue;  // (a symbol no arc matches: nothing enters the row)
      const uint32_t g = T.sym_seg[xi] + sg;
      if (g >= T.sym_seg[xi + 1]) continue;
      const uint32_t q = T.seg_dst[g];
      if (eps_in[q]) continue;  // filled with its epsilon arcs, at its level
      kb_pair_select(T, P, G, O, pair, i, d - i, q, T.seg_arc[g], T.seg_arc[g + 1], 0, 0);
    }
    __syncthreads();
    // the nodes epsilon arcs enter, 00 level by 00 level: one lane per (cell, entry)
    for (uint32_t L = 0; L < P.n_levels; ++L) {
      const uint32_t e_lo = P.lvl_ent[L], n_ent = P.lvl_ent[L + 1] - e_lo;
      for (uint64_t t = lane; t < n_cell * n_ent; t += kLanes) {
        const uint32_t i = ilo + (uint32_t)(t / n_ent), e = e_lo + (uint32_t)(t % n_ent);
        const uint32_t q = P.ent_dst[e];
        if (d == 0 && q == 0) continue;  // (0, 0, start)
        uint32_t m0 = 0, m1 = 0;
        const uint32_t xi = i ? x[i - 1] : T.n_syms;
        if (xi < T.n_syms) {  // the segment of destination q, if the symbol has one (seg_dst ascends within a symbol)
          const uint32_t g1 = T.sym_seg[xi + 1];
          uint32_t lo = T.sym_seg[xi], hi = g1;
          while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (T.seg_dst[mid] < q)
              lo = mid + 1;
            else
              hi = mid;
          }
          if (lo < g1 && T.seg_dst[lo] == q) {
            m0 = T.seg_arc[lo];
            m1 = T.seg_arc[lo + 1];
          }
        }
        kb_pair_select(T, P, G, O, pair, i, d - i, q, m0, m1, P.ent_arc[e], P.ent_arc[e + 1]);
      }
      __syncthreads();
    }
  }
  if (lane == 0) {  // cell (n, m) is the last of its diagonal
    const double* F = base + (size_t)((n + m) % 3) * DQ + DQ - QK + (size_t)T.final_state * K;
    uint32_t c = 0;
    while (c < K && F[c] > ninf) ++c;
    O.n_paths[pair] = c;
  }
}

// one lane per (pair, rank): slot pair * K + rank, idle if the pair has no such rank.  kWrite = false counts the path's arcs into
// len[slot] and adds their weights from the end into logw[slot]; kWrite = true writes the arcs in path order at
// path[path_off[slot] ..)
template <bool kWrite>
__global__ void pair_kbest_walk_kernel(uint32_t n_pairs, uint32_t n_states, uint32_t final_state, uint64_t n_arcs, uint32_t levels,
                                       const uint64_t* off, const uint64_t* off2, PairKbOut O, const uint32_t* a_src,
                                       const uint8_t* a_flags, const double* a_w, uint32_t* len, double* logw,
                                       const uint64_t* path_off, uint32_t* path, int* err) {
  const uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (a chunk has at most 2^24 slots: the driver's cap)
  const uint32_t K = O.K;
  if (slot >= (uint64_t)n_pairs * K) return;
  const uint32_t pair = (uint32_t)(slot / K);
  uint32_t r = (uint32_t)(slot % K);
  if (r >= O.n_paths[pair]) return;
  uint32_t i = (uint32_t)(off[pair + 1] - off[pair]), j = (uint32_t)(off2[pair + 1] - off2[pair]), q = final_state;
  const uint32_t m = j;
  const uint32_t* ba = O.bp_arc + O.bp_off[pair];
  const uint16_t* br = O.bp_rank + O.bp_off[pair];
  const uint64_t cap = ((uint64_t)i + j + 1) * ((uint64_t)levels + 1);  // no path of the trellis is longer
  const uint32_t n_path = kWrite ? len[slot] : 0;
  uint32_t steps = 0;
  double w = 0.0;
  while (true) {
    const size_t at = (((size_t)i * (m + 1) + j) * n_states + q) * K + r;
    const uint32_t a = ba[at];
    if (a == kNone) break;
    const uint32_t rs = br[at];
    if (a >= n_arcs || steps >= cap || (kWrite && steps >= n_path) || rs >= K) {
      atomicOr(err, kErrWalk);
      return;
    }
    const uint32_t f = a_flags[a];
    if (((f & 1) && i == 0) || ((f & 2) && j == 0)) {
      atomicOr(err, kErrWalk);
      return;
    }
    ++steps;
    if (kWrite) path[path_off[slot] + n_path - steps] = a;
    w = a_w[a] + w;
    q = a_src[a];
    r = rs;
    if (f & 1) --i;
    if (f & 2) --j;
  }
  if (i != 0 || j != 0 || q != 0 || r != 0 || (kWrite && steps != n_path)) atomicOr(err, kErrWalk);
  if (!kWrite) {
    len[slot] = steps;
    logw[slot] = w;
  }
}
}  // namespace

extern "C" {

int carmel_hip_decode_pairs_kbest(carmel_hip_decoder* d, uint32_t k, uint64_t n_pairs, const uint64_t* off, const uint32_t* sym,
                                  const uint64_t* off2, const uint32_t* sym2, uint64_t* line_paths) {
  const char* who = "carmel_hip_decode_pairs_kbest";
  if (k < 1 || k > kMaxK) return fail(CARMEL_HIP_ERR_ARG, std::string(who) + ": k must be in 1 .. 1024");
  PairCall call{d, n_pairs, off, off2};
  if (const int rc = call.check(who, sym, sym2, line_paths)) return rc;
  const uint32_t K = k, Q = d->n_states;
  // the tier, by K doubles a state: from the pair with the largest diagonal
  uint64_t longest = 0;
  for (uint64_t l = 0; l < n_pairs; ++l) longest = std::max(longest, call.diag_doubles(l));
  const bool lds = 3 * longest * K <= kLdsDoubles && !lib_opt_off("decode_lds");
  const size_t lds_bytes = lds ? 24 * longest * K : 0;
  const std::string bad = std::string(who) + ": inconsistent back-pointers";
  HIPCHK(hipSetDevice(d->device));  // (d_err below is allocated before the chunk driver sets it)
  std::vector<double> r_logw;
  std::vector<uint64_t> r_off(1, 0);
  std::vector<uint32_t> r_arcs;
  line_paths[0] = 0;
  DevBuf<uint64_t> d_bpoff, d_poff, d_rows_off;
  DevBuf<uint32_t> d_bparc, d_np, d_len, d_path;
  DevBuf<uint16_t> d_bprank;
  DevBuf<double> d_logw, d_rows;
  DevBuf<int> d_err;
  HIPCHK(d_err.alloc(1));
  // a pair costs its back-pointers (arc and rank), its symbols and, in the global tier, its three diagonals
  auto cost = [&](uint64_t l) {
    return 6 * call.nodes(l) * K + 4 * (call.len1(l) + call.len2(l)) + (lds ? 0 : 24 * call.diag_doubles(l) * K);
  };
  const int rc = decode_chunks_by_cost(d, n_pairs, off, sym, off2, sym2, lds, cost, (1u << 24) / K, [&](DecodeChunk& c) {
    hipStream_t s = d->stream;
    const uint32_t n = c.n;
    const uint64_t n_slots = (uint64_t)n * K;
    std::vector<uint64_t> h_bpoff(n + 1, 0), h_rows(n + 1, 0);
    for (uint32_t l = 0; l < n; ++l) {
      h_bpoff[l + 1] = h_bpoff[l] + call.nodes(c.lo + l) * K;
      h_rows[l + 1] = h_rows[l] + 3 * call.diag_doubles(c.lo + l) * K;
    }
    HIPCHK(d_bpoff.upload(h_bpoff, s));
    HIPCHK(d_bparc.alloc(h_bpoff[n]));
    HIPCHK(d_bprank.alloc(h_bpoff[n]));
    HIPCHK(d_np.alloc(n));
    HIPCHK(d_len.alloc(n_slots));
    HIPCHK(d_logw.alloc(n_slots));
    PairLines L{c.L.off, c.L.sym, c.off2, c.sym2, c.L.order, nullptr, nullptr};
    if (!lds) {
      HIPCHK(d_rows_off.upload(h_rows, s));
      HIPCHK(d_rows.alloc(h_rows[n]));
      L.rows = d_rows.p;
      L.rows_off = d_rows_off.p;
    }
    HIPCHK(hipMemsetAsync(d_err.p, 0, sizeof(int), s));
    const PairKbOut O{d_bpoff.p, d_bparc.p, d_bprank.p, d_np.p, K};
    const uint32_t wb = (uint32_t)((n_slots + 255) / 256);
    auto walk = [&](bool write) {
      (write ? pair_kbest_walk_kernel<true> : pair_kbest_walk_kernel<false>)<<<wb, 256, 0, s>>>(
          n, Q, d->final_state, d->n_arcs, d->pair_levels, L.off, L.off2, O, d->a_src.p, d->a_flags.p, d->a_w.p, d_len.p, d_logw.p,
          d_poff.p, d_path.p, d_err.p);
    };
    if (const int r = c.begin()) return r;
    HIPCHK(hipMemsetAsync(d_bparc.p, 0xff, h_bpoff[n] * sizeof(uint32_t), s));  // every slot kNone
    if (lds)
      pair_kbest_trellis_kernel<true><<<n, kLanes, lds_bytes, s>>>(d->T, d->TP, L, d->eps_in.p, O);
    else
      pair_kbest_trellis_kernel<false><<<n, kLanes, 0, s>>>(d->T, d->TP, L, d->eps_in.p, O);
    walk(false);
    if (const int r = c.end()) return r;
    std::vector<uint32_t> np(n), len(n_slots);
    std::vector<double> lw(n_slots);
    int err = 0;
    HIPCHK(hipMemcpyAsync(np.data(), d_np.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(len.data(), d_len.p, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(lw.data(), d_logw.p, n_slots * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    if (const int r = c.wait()) return r;
    if (err) return fail(CARMEL_HIP_ERR_STATE, bad);
    for (uint32_t l = 0; l < n; ++l)
      if (np[l] > K) return fail(CARMEL_HIP_ERR_STATE, bad);
    const uint64_t base = r_arcs.size();
    const std::vector<uint64_t> h_poff = decode_collect_paths(c, K, np, len, lw, base, line_paths, r_logw, r_off);
    if (!h_poff[n_slots]) return CARMEL_HIP_OK;
    HIPCHK(d_poff.upload(h_poff, s));
    HIPCHK(d_path.alloc(h_poff[n_slots]));
    if (const int r = c.begin()) return r;
    walk(true);
    if (const int r = c.end()) return r;
    r_arcs.resize(base + h_poff[n_slots]);
    HIPCHK(hipMemcpyAsync(r_arcs.data() + base, d_path.p, h_poff[n_slots] * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    if (const int r = c.wait()) return r;
    return err ? fail(CARMEL_HIP_ERR_STATE, bad) : CARMEL_HIP_OK;
  });
  if (rc) return rc;
  d->kb_logw.swap(r_logw);
  d->kb_off.swap(r_off);
  d->kb_arcs.swap(r_arcs);
  return CARMEL_HIP_OK;
}

}  // extern "C"
