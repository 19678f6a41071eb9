// decode_trellis.hpp — the trellis kernel that the k-best decoder (decode_kbest.hip: KbNode) and the all-paths sum
// (decode_sum.hip: SumNode) share: decode.hip's trellis over (line position i, state q), one wavefront = one workgroup of 64 lanes
// per line, where a node (i, q) is computed ONCE, by one lane, from all the arcs that enter it.  A Node supplies
//   width()                      the doubles a state has in a row: K (a list, padded with -inf) or 1;
//   begin(line, lane)            before the first barrier: its per-line pointers, what it records for node (0, start);
//   fill(T, pos, q, prev, m0, m1, same, e0, e1, start)
//                                node (pos, q) from the matched arcs [m0, m1) (sources in row `prev`) and the epsilon arcs
//                                [e0, e1) (sources in row `same`), into state q of row `same`; start: the node is (0, start);
//   read_out(line, F)            F: the final state of the last row.
//
// Order within a position: first the nodes that no epsilon arc enters (one lane per destination segment of the line's symbol);
// then, level by level, the nodes that epsilon arcs enter (one lane per entry): such a node is filled from its matched arcs
// (sources in the previous row) AND its epsilon arcs (sources in the same row, of strictly lower level, final since the barrier
// that ended their level) in one pass -- never finished in the matched phase and patched afterwards, as the 1-best kernel does:
// that would merge a list in place, or read an accumulator out twice.  No lane reads a node that another is writing.  Barriers
// are the 1-best kernel's: after the row is cleared, after the matched phase, after every level.  Only acyclic epsilon subgraphs
// have levels: the hosts refuse a cyclic one before any launch.
//
// What fixes every bit of a result, whatever the memory tier, the chunking, the launch order or the lane count: a node is owned
// by one lane; the candidates reach fill() as matched arcs in arc-id order, then epsilon arcs in arc-id order (the tables are
// sorted so), and node (0, start) has its 0.0 before either; every source is final when it is read (the barriers above).
//
// Rows: two rows of |Q| width() doubles, in LDS when that is <= kLdsStates, otherwise in a global buffer per line; option
// decode_lds=0 forces the global tier.
#pragma once
#include <limits>
#include "decode.hpp"

namespace carmel_hip {
// the nodes of one position that epsilon arcs enter, level by level; [g0, g1) are the segments of the position's symbol (empty at
// position 0, the `first`)
template <class Node>
__device__ void trellis_close(const DecodeTables& T, Node& N, uint32_t pos, const double* prev, uint32_t g0, uint32_t g1,
                              double* row, int lane, bool first) {
  for (uint32_t L = 0; L < T.n_levels; ++L) {
    for (uint32_t e = T.lvl_ent[L] + lane; e < T.lvl_ent[L + 1]; e += kLanes) {
      const uint32_t q = T.ent_dst[e];
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
      N.fill(T, pos, q, prev, m0, m1, row, T.ent_arc[e], T.ent_arc[e + 1], first && q == 0);
    }
    __syncthreads();
  }
}

// eps_in [|Q|]: an epsilon arc enters the state
template <class Node, bool kLds>
__global__ void __launch_bounds__(kLanes) trellis_kernel(DecodeTables T, DecodeLines D, const uint8_t* eps_in, Node N) {
  extern __shared__ double lds_rows[];
  const int lane = threadIdx.x;
  const uint32_t line = D.order[blockIdx.x];
  const uint32_t W = N.width();
  const size_t QW = (size_t)T.n_states * W;
  double* cur = kLds ? lds_rows : D.rows + (size_t)line * 2 * QW;
  double* nxt = cur + QW;
  const uint64_t s0 = D.off[line];
  const uint32_t n = (uint32_t)(D.off[line + 1] - s0);
  const double ninf = -std::numeric_limits<double>::infinity();
  N.begin(line, lane);
  for (size_t s = lane; s < QW; s += kLanes) cur[s] = s == 0 ? 0.0 : ninf;  // (0, start): one value, 0.0
  __syncthreads();
  trellis_close(T, N, 0, cur, 0, 0, cur, lane, true);
  for (uint32_t i = 0; i < n; ++i) {
    for (size_t s = lane; s < QW; s += kLanes) nxt[s] = ninf;
    __syncthreads();
    const uint32_t x = D.sym[s0 + i];
    const bool known = x < T.n_syms;  // (a symbol no arc matches leaves the row empty: no derivation)
    const uint32_t g0 = known ? T.sym_seg[x] : 0, g1 = known ? T.sym_seg[x + 1] : 0;
    for (uint32_t g = g0 + lane; g < g1; g += kLanes) {
      const uint32_t q = T.seg_dst[g];
      if (eps_in[q]) continue;  // filled with its epsilon arcs, at its level
      N.fill(T, i + 1, q, cur, T.seg_arc[g], T.seg_arc[g + 1], nxt, 0, 0, false);
    }
    __syncthreads();
    trellis_close(T, N, i + 1, cur, g0, g1, nxt, lane, false);
    double* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (lane == 0) N.read_out(line, cur + (size_t)T.final_state * W);
}

template <class Node>
void launch_trellis(const carmel_hip_decoder* d, bool lds, uint32_t n, const DecodeLines& L, const Node& N, hipStream_t s) {
  if (lds)
    trellis_kernel<Node, true><<<n, kLanes, 16 * (size_t)d->n_states * N.width(), s>>>(d->T, L, d->eps_in.p, N);
  else
    trellis_kernel<Node, false><<<n, kLanes, 0, s>>>(d->T, L, d->eps_in.p, N);
}
}  // namespace carmel_hip
