// decode_pairs_posterior.hip — batch pair arc posteriors: how often every arc of one (composed) transducer is used, in
// expectation, over all the derivations of a batch of pairs (x, y) -- the E-step of carmel -t (train.cc's forward/backward,
// train.cc:254-266, 698-860) stated on the pair trellis of decode_pairs.hip, against a machine that is composed once: no
// derivation lattice is built per pair.  It is to carmel_hip_decode_pairs_sum what decode_posterior.hip is to the one-sided sum.
// Pair, derivation, matched side, the four kinds of arc (MM, M0, 0M, 00), the 00 levels, dropped zero-weight arcs, unknown
// symbols: decode_pairs.hip's.
//
// Forward.  decode_pairs_trellis.hpp's pair_trellis_kernel with KeepAcc: SumAcc's arithmetic in SumAcc's order, and every closed
// diagonal copied out, cooperatively and after its last barrier, to the pair's alpha plane of (n + 1)(m + 1)|Q| doubles in
// global memory, slot (i (m + 1) + j)|Q| + q (the back-pointers' layout).  Every slot is written, -inf where nothing reaches.
// Z = alpha[n][m][final] is bit for bit carmel_hip_decode_pairs_sum's value.
//
// Backward (pair_posterior_kernel).  One wavefront = one workgroup of 64 lanes per pair, in the chunk's launch order, over the
// anti-diagonals d = n + m down to 0, three beta diagonals kept, indexed as the forward's are (a cell by its position on the
// shorter line).  beta[i][j][q] has ONE streaming accumulator (sweep_math.hpp's Lse), owned by one lane, fed in this order and
// read out once:
//   0.0 first, at (n, m, final) only;
//   if i < n the arcs OUT of q whose matched symbol is x_{i+1}, in arc-id order, MM and M0 as their ids fall: MM (other symbol
//   y_{j+1}) reads (i + 1, j + 1, dst) on diagonal d + 2, M0 reads (i + 1, j, dst) on d + 1; an arc that fails its test is skipped;
//   the matched-side-epsilon arcs OUT of q in arc-id order, 0M and 00 as their ids fall: 0M (other symbol y_{j+1}) reads
//   (i, j + 1, dst) on d + 1, 00 reads (i, j, dst) in its own cell, which is final since the barrier that ended dst's level.
// Order within a diagonal, the forward's mirrored: the diagonal is cleared (0.0 at (n, m, final)); barrier; every node (cell, q)
// whose state no matched-side-epsilon arc leaves is filled by one lane per (cell, source segment of x_{i+1}); barrier; then,
// from the highest 00 level of a SOURCE down, every node whose state such arcs leave, one lane per (cell, entry), filled once
// from both kinds of arc (its matched segment found by the forward's binary search); barrier after every level.  No lane reads a
// node another is writing.  A node with alpha = -inf is skipped: its beta stays -inf, nothing reads it for a count.
//
// Counts.  The lane that feeds an edge's candidate forms p = exp(((alpha[source node] + w) + beta[destination node]) - Z), the
// bracketed sum first, and, if p > 0, adds c_l p to count[a] with the hardware f64 atomic; c_l is the pair's weight (1 without
// weights).  A pair without a derivation, or of weight 0, adds nothing: its workgroup leaves before the first diagonal.
//
// What is fixed: sum_logw to the bit; every term c_l p to the bit, whatever the tier, the chunking or the launch order; the order
// in which the terms of one arc are added is not.
//
// Tiers: the three beta diagonals are in LDS when 3 (min(n, m) + 1)|Q| <= 8192 doubles for the longest pair of the call (the
// forward's bound), otherwise in the pair's global rows, which the forward has finished with; decode_lds=0 applies.  A pair
// costs 8 (n + 1)(m + 1)|Q| bytes for its plane, 4 (n + m) for its symbols and, in the global tier, 24 (min(n, m) + 1)|Q|.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "decode_pairs_trellis.hpp"

namespace {
// what the backward kernel takes beside the tables and the pairs
struct PairBack {
  const uint64_t* a_off;
  const double* alpha;
  const double* weight;  // [n] pair weights; nullptr: every pair weighs 1
  double* sum;           // [n]: Z
  double* count;         // [n_arcs]
};

// what a lane knows of the pair and of the diagonal it works on
struct BackDiag {
  const double* A;   // the pair's alpha plane
  double Z, c;
  double* count;
  double* cur;       // diagonal d
  const double* d1;  // d + 1
  const double* d2;  // d + 2
  uint32_t Q, n, m, final_state;
  bool by_i;
  const uint32_t* y;
};

__device__ __forceinline__ void pair_edge(const BackDiag& G, Lse& b, double a, double w, double bd, uint32_t id) {
  b.add(bd + w);
  if (bd > NEG_INF) {
    const double p = K_EXP(((a + w) + bd) - G.Z);
    if (p > 0.0) unsafeAtomicAdd(G.count + id, G.c * p);  // hardware global_atomic_add_f64 (no CAS loop)
  }
}

// node (i, j, q): beta from its matched arcs [m0, m1) (none if i = n), then its epsilon arcs [e0, e1), and every such edge's share
// of the counts
__device__ __forceinline__ void pair_back_node(const DecodePairOutTables& O, const BackDiag& G, uint32_t i, uint32_t j, uint32_t q,
                                               uint32_t m0, uint32_t m1, uint32_t e0, uint32_t e1) {
  const uint32_t Q = G.Q;
  const double a = G.A[((size_t)i * (G.m + 1) + j) * Q + q];
  if (!(a > NEG_INF)) return;  // (no derivation passes here: the node keeps its -inf)
  const uint32_t p = G.by_i ? i : j;
  const bool has_y = j < G.m;
  const uint32_t yj = has_y ? G.y[j] : 0;  // y_{j+1}
  double* cell = G.cur + (size_t)p * Q;
  // (i + 1, j + 1) is cell p + 1 of d + 2; (i + 1, j) cell p + 1 or p of d + 1; (i, j + 1) cell p or p + 1 of d + 1.  A cell
  // beyond the pair is never read: MM needs i < n and j < m, M0 i < n, 0M j < m
  const double* mm = G.d2 + (size_t)(i < G.n && has_y ? p + 1 : p) * Q;
  const double* m0p = G.d1 + (size_t)(G.by_i && i < G.n ? p + 1 : p) * Q;
  const double* zm = G.d1 + (size_t)(!G.by_i && has_y ? p + 1 : p) * Q;
  Lse b;
  b.init();
  if (i == G.n && j == G.m && q == G.final_state) b.add(0.0);
  for (uint32_t k = m0; k < m1; ++k) {
    const uint32_t o = O.m_osym[k];
    if (o == 0)
      pair_edge(G, b, a, O.m_w[k], m0p[O.m_dst[k]], O.m_id[k]);
    else if (has_y && o == yj)
      pair_edge(G, b, a, O.m_w[k], mm[O.m_dst[k]], O.m_id[k]);
  }
  for (uint32_t k = e0; k < e1; ++k) {
    const uint32_t o = O.e_osym[k];
    if (o == 0)
      pair_edge(G, b, a, O.e_w[k], cell[O.e_dst[k]], O.e_id[k]);
    else if (has_y && o == yj)
      pair_edge(G, b, a, O.e_w[k], zm[O.e_dst[k]], O.e_id[k]);
  }
  cell[q] = b.value();
}

template <bool kLds>
__global__ void __launch_bounds__(kLanes) pair_posterior_kernel(DecodeTables T, DecodePairOutTables O, PairLines D, PairBack B) {
  extern __shared__ double lds_diag[];
  const int lane = threadIdx.x;
  const uint32_t pair = D.order[blockIdx.x];
  const uint32_t Q = T.n_states;
  const uint32_t* x = D.sym + D.off[pair];
  const uint32_t n = (uint32_t)(D.off[pair + 1] - D.off[pair]);
  const uint32_t* y = D.sym2 + D.off2[pair];
  const uint32_t m = (uint32_t)(D.off2[pair + 1] - D.off2[pair]);
  const bool by_i = n <= m;
  const size_t DQ = (size_t)((by_i ? n : m) + 1) * Q;
  const double* A = B.alpha + B.a_off[pair];
  const double Z = A[((size_t)n * (m + 1) + m) * Q + T.final_state];
  const double c = B.weight ? B.weight[pair] : 1.0;
  if (lane == 0) B.sum[pair] = Z;
  if (!(Z > NEG_INF) || !(c > 0.0)) return;  // (the whole workgroup: nothing to add)
  double* base = kLds ? lds_diag : D.rows + D.rows_off[pair];
  BackDiag G;
  G.A = A;
  G.Z = Z;
  G.c = c;
  G.count = B.count;
  G.Q = Q;
  G.n = n;
  G.m = m;
  G.final_state = T.final_state;
  G.by_i = by_i;
  G.y = y;
  for (uint32_t d = n + m + 1; d-- > 0;) {
    G.cur = base + (size_t)(d % 3) * DQ;
    G.d1 = base + (size_t)((d + 1) % 3) * DQ;
    G.d2 = base + (size_t)((d + 2) % 3) * DQ;
    const uint32_t ilo = d > m ? d - m : 0, ihi = d < n ? d : n;
    const uint64_t n_cell = (uint64_t)(ihi - ilo) + 1;
    // (n, m, final), the last cell of its diagonal, holds its 0.0 from the beginning; if epsilon arcs leave the final state its
    // level fills it again, 0.0 first
    for (size_t s = lane; s < DQ; s += kLanes) G.cur[s] = (d == n + m && s == DQ - Q + T.final_state) ? 0.0 : NEG_INF;
    __syncthreads();
    // the nodes no epsilon arc leaves: one lane per (cell, source segment of x_{i+1})
    for (uint64_t t = lane; t < n_cell * O.max_seg; t += kLanes) {
      const uint32_t i = ilo + (uint32_t)(t / O.max_seg), sg = (uint32_t)(t % O.max_seg);
      if (i == n) continue;  // (no matched symbol)
      const uint32_t xi = x[i];
      if (xi >= T.n_syms) continue;
      const uint32_t g = O.sym_seg[xi] + sg;
      if (g >= O.sym_seg[xi + 1]) continue;
      const uint32_t q = O.seg_src[g];
      if (O.eps_out[q]) continue;  // filled with its epsilon arcs, at its level
      pair_back_node(O, G, i, d - i, q, O.seg_arc[g], O.seg_arc[g + 1], 0, 0);
    }
    __syncthreads();
    // the nodes epsilon arcs leave, from the highest 00 level of a source down: one lane per (cell, entry)
    for (uint32_t L = O.n_levels; L-- > 0;) {
      const uint32_t e_lo = O.lvl_ent[L], n_ent = O.lvl_ent[L + 1] - e_lo;
      for (uint64_t t = lane; t < n_cell * n_ent; t += kLanes) {
        const uint32_t i = ilo + (uint32_t)(t / n_ent), e = e_lo + (uint32_t)(t % n_ent);
        const uint32_t q = O.ent_src[e];
        uint32_t m0 = 0, m1 = 0;
        const uint32_t xi = i < n ? x[i] : T.n_syms;
        if (xi < T.n_syms) {  // the segment of source q, if the symbol has one (seg_src ascends within a symbol)
          const uint32_t g1 = O.sym_seg[xi + 1];
          uint32_t lo = O.sym_seg[xi], hi = g1;
          while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (O.seg_src[mid] < q)
              lo = mid + 1;
            else
              hi = mid;
          }
          if (lo < g1 && O.seg_src[lo] == q) {
            m0 = O.seg_arc[lo];
            m1 = O.seg_arc[lo + 1];
          }
        }
        pair_back_node(O, G, i, d - i, q, m0, m1, O.ent_arc[e], O.ent_arc[e + 1]);
      }
      __syncthreads();
    }
  }
}
}  // namespace

extern "C" {

int carmel_hip_decode_pairs_posterior(carmel_hip_decoder* d, uint64_t n_pairs, const uint64_t* off, const uint32_t* sym,
                                      const uint64_t* off2, const uint32_t* sym2, const double* pair_weight, double* sum_logw,
                                      double* arc_count) {
  const char* who = "carmel_hip_decode_pairs_posterior";
  if (d && off && off2 && arc_count && n_pairs < kNone && pair_weight)
    for (uint64_t l = 0; l < n_pairs; ++l)
      if (!(pair_weight[l] >= 0.0) || !std::isfinite(pair_weight[l]))
        return fail(CARMEL_HIP_ERR_ARG, std::string(who) + ": a pair weight is negative or not finite");
  PairCall call{d, n_pairs, off, off2};
  if (const int rc = call.check(who, sym, sym2, arc_count)) return rc;
  HIPCHK(hipSetDevice(d->device));  // (the counts below are zeroed before the chunk driver sets it)
  hipStream_t s = d->stream;
  if (d->count.n != d->n_arcs) HIPCHK(d->count.alloc(d->n_arcs));
  if (d->n_arcs) HIPCHK(hipMemsetAsync(d->count.p, 0, d->n_arcs * sizeof(double), s));  // once per call: every chunk adds to it
  std::vector<double> r_sum(n_pairs);
  DevBuf<uint64_t> d_aoff, d_rows_off;
  DevBuf<double> d_alpha, d_sum, d_weight, d_rows;
  // a pair costs its alpha plane, its symbols and, in the global tier, its three diagonals
  auto cost = [&](uint64_t l) {
    return 8 * call.nodes(l) + 4 * (call.len1(l) + call.len2(l)) + (call.lds ? 0 : 24 * call.diag_doubles(l));
  };
  const int rc = decode_chunks_by_cost(d, n_pairs, off, sym, off2, sym2, call.lds, cost, 1u << 24, [&](DecodeChunk& c) {
    const uint32_t n = c.n;
    std::vector<uint64_t> h_aoff(n + 1, 0);
    for (uint32_t l = 0; l < n; ++l) h_aoff[l + 1] = h_aoff[l] + call.nodes(c.lo + l);
    std::vector<double> h_weight;  // (named: the copy is asynchronous)
    if (pair_weight) h_weight.assign(pair_weight + c.lo, pair_weight + c.hi);
    HIPCHK(d_aoff.upload(h_aoff, s));
    HIPCHK(d_alpha.alloc(h_aoff[n]));
    HIPCHK(d_sum.alloc(n));
    if (pair_weight) HIPCHK(d_weight.upload(h_weight, s));
    PairLines L;
    if (const int r = call.rows(c, d_rows, d_rows_off, L)) return r;
    const PairBack B{d_aoff.p, d_alpha.p, pair_weight ? d_weight.p : nullptr, d_sum.p, d->count.p};
    if (const int r = c.begin()) return r;
    launch_pairs<KeepAcc>(d, call.lds, call.lds_bytes, n, L, KeepOut{d_aoff.p, d_alpha.p}, s);
    if (call.lds)
      pair_posterior_kernel<true><<<n, kLanes, call.lds_bytes, s>>>(d->T, d->TPO, L, B);
    else
      pair_posterior_kernel<false><<<n, kLanes, 0, s>>>(d->T, d->TPO, L, B);
    if (const int r = c.end()) return r;
    HIPCHK(hipMemcpyAsync(r_sum.data() + c.lo, d_sum.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    return c.wait();
  });
  if (rc) return rc;
  if (d->n_arcs) {
    HIPCHK(hipMemcpyAsync(arc_count, d->count.p, d->n_arcs * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  if (sum_logw && n_pairs) std::memcpy(sum_logw, r_sum.data(), n_pairs * sizeof(double));
  return CARMEL_HIP_OK;
}

}  // extern "C"
