// decode_pairs_trellis.hpp — what the pair entry points (decode_pairs.hip: the Viterbi alignment and the sum;
// decode_pairs_posterior.hip: the arc posteriors; decode_pairs_sample.hip: the alignment samples) share, and of which
// decode_pairs_kbest.hip (the k best alignments: a k-list trellis kernel of its own) takes Diag and the host side: the anti-diagonal
// trellis over (matched position i, other position j, state q) with its fixed candidate order, the sum's accumulator, the
// accumulator that keeps every node (the forward pass of the posteriors and of the sampler), and the host side of a call -- the
// argument checks, the tier and the global tier's diagonals.  The trellis, its order and its barriers are described in
// decode_pairs.hip's header.
//
// An accumulator Acc gives init / add / store / read_out (decode_pairs.hip) and kKeep: if set, every closed diagonal is copied
// out, cooperatively and after its last barrier, by Acc::keep -- the forward planes of the arc posteriors and of the sampler.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <limits>
#include <string>
#include <vector>
#include "decode.hpp"
#include "engine.hpp"
#include "sweep_math.hpp"

namespace carmel_hip {
constexpr uint64_t kLdsDoubles = 2 * (uint64_t)kLdsStates;  // 64 KiB

struct PairLines {
  const uint64_t* off;   // chunk-local CSR of the matched side's lines
  const uint32_t* sym;
  const uint64_t* off2;  // ... of the other side's
  const uint32_t* sym2;
  const uint32_t* order;     // launch order: chunk-local pair index of block b
  double* rows;              // global tier: every pair's three diagonals, at rows_off[pair] (nullptr in the LDS tier)
  const uint64_t* rows_off;
};

struct SumOut {
  double* sum;  // [n]
};

struct SumAcc {
  typedef SumOut Out;
  static constexpr bool kKeep = false;
  Lse a;
  __device__ __forceinline__ void init(bool start) {
    a.init();
    if (start) a.add(0.0);
  }
  __device__ __forceinline__ void add(double x, uint32_t) { a.add(x); }
  __device__ __forceinline__ double store(const Out&, uint32_t, size_t) const { return a.value(); }
  static __device__ __forceinline__ void read_out(const Out& O, uint32_t pair, double f) { O.sum[pair] = f; }
};

struct KeepOut {
  const uint64_t* a_off;  // [n + 1]: each pair's (n + 1)(m + 1)|Q| doubles
  double* alpha;
};

// SumAcc, and the closed diagonals kept
struct KeepAcc {
  typedef KeepOut Out;
  static constexpr bool kKeep = true;
  Lse a;
  __device__ __forceinline__ void init(bool start) {
    a.init();
    if (start) a.add(0.0);
  }
  __device__ __forceinline__ void add(double x, uint32_t) { a.add(x); }
  __device__ __forceinline__ double store(const Out&, uint32_t, size_t) const { return a.value(); }
  static __device__ __forceinline__ void read_out(const Out&, uint32_t, double) {}  // (Z is the plane's last cell)
  // cells (i, d - i), i = ilo .. ihi, of the closed diagonal `cur` -> the plane
  static __device__ __forceinline__ void keep(const Out& O, uint32_t pair, const double* cur, uint32_t d, uint32_t ilo, uint32_t ihi,
                                              bool by_i, uint32_t m, uint32_t Q, int lane) {
    double* A = O.alpha + O.a_off[pair];
    const uint64_t n_slot = ((uint64_t)(ihi - ilo) + 1) * Q;
    for (uint64_t t = lane; t < n_slot; t += kLanes) {
      const uint32_t i = ilo + (uint32_t)(t / Q), q = (uint32_t)(t % Q), j = d - i;
      A[((size_t)i * (m + 1) + j) * Q + q] = cur[(size_t)(by_i ? i : j) * Q + q];
    }
  }
};

// what a lane knows of the diagonal it works on
struct Diag {
  double* cur;       // diagonal d
  const double* d1;  // d - 1
  const double* d2;  // d - 2
  uint32_t Q, m;
  bool by_i;  // a cell's position on its diagonal is i (n <= m), else j
  const uint32_t* y;
};

// node (i, j, q): its matched arcs [m0, m1) (none if i = 0), then its epsilon arcs [e0, e1)
template <class Acc>
__device__ __forceinline__ void pair_node(const DecodeTables& T, const DecodePairTables& P, const Diag& G,
                                          const typename Acc::Out& O, uint32_t pair, uint32_t i, uint32_t j, uint32_t q, uint32_t m0,
                                          uint32_t m1, uint32_t e0, uint32_t e1) {
  const uint32_t Q = G.Q;
  const uint32_t p = G.by_i ? i : j;
  const bool has_y = j > 0;
  const uint32_t yj = has_y ? G.y[j - 1] : 0;
  double* cell = G.cur + (size_t)p * Q;
  // (i - 1, j - 1) is cell p - 1 of d - 2; (i - 1, j) cell p - 1 or p of d - 1; (i, j - 1) cell p or p - 1 of d - 1
  const double* mm = G.d2 + (size_t)(p ? p - 1 : 0) * Q;
  const double* m0p = G.d1 + (size_t)(G.by_i ? (p ? p - 1 : 0) : p) * Q;
  const double* zm = G.d1 + (size_t)(G.by_i ? p : (p ? p - 1 : 0)) * Q;
  Acc A;
  A.init(i == 0 && j == 0 && q == 0);
  for (uint32_t k = m0; k < m1; ++k) {
    const uint32_t o = P.m_osym[k];
    if (o == 0)
      A.add(m0p[T.m_src[k]] + T.m_w[k], T.m_id[k]);
    else if (has_y && o == yj)
      A.add(mm[T.m_src[k]] + T.m_w[k], T.m_id[k]);
  }
  for (uint32_t k = e0; k < e1; ++k) {
    const uint32_t o = P.e_osym[k];
    if (o == 0)
      A.add(cell[P.e_src[k]] + P.e_w[k], P.e_id[k]);
    else if (has_y && o == yj)
      A.add(zm[P.e_src[k]] + P.e_w[k], P.e_id[k]);
  }
  cell[q] = A.store(O, pair, ((size_t)i * (G.m + 1) + j) * Q + q);
}

// eps_in [|Q|]: a matched-side-epsilon arc (of weight > 0) enters the state
template <class Acc, bool kLds>
__global__ void __launch_bounds__(kLanes) pair_trellis_kernel(DecodeTables T, DecodePairTables P, PairLines D, const uint8_t* eps_in,
                                                              typename Acc::Out O) {
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
  double* base = kLds ? lds_diag : D.rows + D.rows_off[pair];
  const double ninf = -std::numeric_limits<double>::infinity();
  Diag G;
  G.Q = Q;
  G.m = m;
  G.by_i = by_i;
  G.y = y;
  for (uint32_t d = 0; d <= n + m; ++d) {  // (n + m < 2^32 - 1: the entry points check)
    G.cur = base + (size_t)(d % 3) * DQ;
    G.d1 = base + (size_t)((d + 2) % 3) * DQ;
    G.d2 = base + (size_t)((d + 1) % 3) * DQ;
    const uint32_t ilo = d > m ? d - m : 0, ihi = d < n ? d : n;
    const uint64_t n_cell = (uint64_t)(ihi - ilo) + 1;
    // (0, 0, start) holds its 0.0 from the beginning; if epsilon arcs enter the start state its level fills it again, 0.0 first
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
      pair_node<Acc>(T, P, G, O, pair, i, d - i, q, T.seg_arc[g], T.seg_arc[g + 1], 0, 0);
    }
    __syncthreads();
    // the nodes epsilon arcs enter, 00 level by 00 level: one lane per (cell, entry)
    for (uint32_t L = 0; L < P.n_levels; ++L) {
      const uint32_t e_lo = P.lvl_ent[L], n_ent = P.lvl_ent[L + 1] - e_lo;
      for (uint64_t t = lane; t < n_cell * n_ent; t += kLanes) {
        const uint32_t i = ilo + (uint32_t)(t / n_ent), e = e_lo + (uint32_t)(t % n_ent);
        const uint32_t q = P.ent_dst[e];
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
        pair_node<Acc>(T, P, G, O, pair, i, d - i, q, m0, m1, P.ent_arc[e], P.ent_arc[e + 1]);
      }
      __syncthreads();
    }
    // the diagonal is closed (the barrier above, or the one after the matched phase): its cells go out, every slot of them
    if constexpr (Acc::kKeep) Acc::keep(O, pair, G.cur, d, ilo, ihi, by_i, m, Q, lane);
  }
  if (lane == 0) Acc::read_out(O, pair, base[(size_t)((n + m) % 3) * DQ + DQ - Q + T.final_state]);  // cell (n, m): the last of its diagonal
}

template <class Acc>
void launch_pairs(const carmel_hip_decoder* d, bool lds, size_t lds_bytes, uint32_t n, const PairLines& L, const typename Acc::Out& O,
                  hipStream_t s) {
  if (lds)
    pair_trellis_kernel<Acc, true><<<n, kLanes, lds_bytes, s>>>(d->T, d->TP, L, d->eps_in.p, O);
  else
    pair_trellis_kernel<Acc, false><<<n, kLanes, 0, s>>>(d->T, d->TP, L, d->eps_in.p, O);
}

// the pairs of one call: argument checks, the tier (chosen once, from the pair with the largest diagonal) and the costs
struct PairCall {
  carmel_hip_decoder* d;
  uint64_t n_pairs;
  const uint64_t *off, *off2;
  bool lds = false;
  size_t lds_bytes = 0;
  uint64_t len1(uint64_t l) const { return off[l + 1] - off[l]; }
  uint64_t len2(uint64_t l) const { return off2[l + 1] - off2[l]; }
  uint64_t diag_doubles(uint64_t l) const { return (std::min(len1(l), len2(l)) + 1) * d->n_states; }
  uint64_t nodes(uint64_t l) const { return (len1(l) + 1) * (len2(l) + 1) * d->n_states; }
  int check(const char* who, const uint32_t* sym, const uint32_t* sym2, const void* out) {
    const std::string me(who);
    if (!d || !off || !off2 || !out || n_pairs >= kNone || (off[n_pairs] && !sym) || (off2[n_pairs] && !sym2))
      return fail(CARMEL_HIP_ERR_ARG, me + ": bad argument");
    if (const int rc = decode_check_lines(who, n_pairs, off)) return rc;
    if (const int rc = decode_check_lines(who, n_pairs, off2)) return rc;
    uint64_t longest = 0;
    for (uint64_t l = 0; l < n_pairs; ++l) {
      if (len1(l) + len2(l) >= kNone - 1) return fail(CARMEL_HIP_ERR_ARG, me + ": bad line offsets");
      longest = std::max(longest, diag_doubles(l));
    }
    if (!d->pair_cycle.empty())
      return fail(CARMEL_HIP_ERR_UNSUPPORTED, me + ": the arcs with epsilon on both sides have a cycle (" + d->pair_cycle +
                                                  "); pair decoding over such a cycle is not supported");
    lds = 3 * longest <= kLdsDoubles && !lib_opt_off("decode_lds");
    lds_bytes = lds ? 24 * longest : 0;
    return CARMEL_HIP_OK;
  }
  // a chunk's global-tier diagonals
  int rows(const DecodeChunk& c, DevBuf<double>& d_rows, DevBuf<uint64_t>& d_rows_off, PairLines& L) const {
    L = PairLines{c.L.off, c.L.sym, c.off2, c.sym2, c.L.order, nullptr, nullptr};
    if (lds) return CARMEL_HIP_OK;
    std::vector<uint64_t> h(c.n + 1, 0);
    for (uint32_t l = 0; l < c.n; ++l) h[l + 1] = h[l] + 3 * diag_doubles(c.lo + l);
    HIPCHK(d_rows_off.upload(h, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));  // (h goes out of scope)
    HIPCHK(d_rows.alloc(h[c.n]));
    L.rows = d_rows.p;
    L.rows_off = d_rows_off.p;
    return CARMEL_HIP_OK;
  }
};
}  // namespace carmel_hip
