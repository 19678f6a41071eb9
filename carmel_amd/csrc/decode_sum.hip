// decode_sum.hip — batch all-paths sums (carmel -b --sum: post_compose's WFST::sum_acyclic_paths per line, carmel.cc:555-599,
// fst.h:1183-1191, propagate_paths graehl/shared/graph.h:391-419) of many lines against one (composed) transducer: the trellis
// of decode.hip over (line position i, state q) in the log semiring (logsumexp, +) instead of the tropical one (max, +), f64.
// The reference composes each line with the machine and propagates path weights through the result in topological order; here
// nothing is composed per line and nothing is recorded per position: there are no back-pointers, a line costs its two rows.
// Tables, handle and constants are decode.hpp's.
//
// S(x) = ln of the sum, over the derivations of line x, of the product of their arcs' weights (derivation: decode_kbest.hip's
// header); -inf if x has none.  Node (i, q) has ONE streaming accumulator (sweep_math.hpp's Lse), owned by one lane, fed in a
// fixed order and read out once:
//   0.0 first, at node (0, start) only;
//   then the matched candidates row[i - 1][src] + w of the arcs into q labelled x_i, in arc-id order;
//   then the epsilon candidates row[i][src] + w of the epsilon arcs into q, in arc-id order (their sources are of strictly lower
//   epsilon level: final since the barrier that ended that level).
// A candidate of -inf adds nothing.  That order fixes every bit of S(x): it does not depend on the memory tier, the chunking, the
// launch order or the lane count.  A single derivation costs no exp and no log (acc stays 1): its sum is its arcs' weights added
// in path order.
//
// Order within a position, as in the k-best kernel: first the nodes no epsilon arc enters (one lane per destination segment of
// the line's symbol); then, level by level, the nodes epsilon arcs enter, each from its matched arcs AND its epsilon arcs in one
// pass (one lane per entry) -- never finished in the matched phase and patched afterwards, which would read an accumulator out
// twice.  Barriers are the 1-best kernel's: after the row is cleared, after the matched phase, after every level.
//
// Rows: two rows of |Q| doubles, in LDS when |Q| <= kLdsStates, otherwise in a global buffer per line; option decode_lds=0
// forces the global tier.  Only acyclic epsilon subgraphs have levels (the reference's sum is "acyclic-correct only",
// carmel.cc:1787): a cyclic one is refused by the host before any launch.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <numeric>
#include <vector>
#include "decode.hpp"
#include "engine.hpp"
#include "sweep_math.hpp"

namespace {
struct SumLines {
  const uint64_t* off;    // chunk-local CSR of the lines' symbols
  const uint32_t* sym;
  const uint32_t* order;  // launch order: chunk-local line index of block b
  double* rows;           // global tier: 2 |Q| doubles per line (nullptr in the LDS tier)
  const uint8_t* eps_in;  // [|Q|]: an epsilon arc enters the state
  double* sum;            // [n]
};

// the nodes of one position that epsilon arcs enter, level by level; [g0, g1) are the segments of the position's symbol (empty at
// position 0, where `first` feeds the start state's accumulator its 0.0)
__device__ void sum_close(const DecodeTables& T, const double* prev, uint32_t g0, uint32_t g1, double* row, int lane, bool first) {
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
      Lse a;
      a.init();
      if (first && q == 0) a.add(0.0);
      for (uint32_t k = m0; k < m1; ++k) a.add(prev[T.m_src[k]] + T.m_w[k]);
      for (uint32_t k = T.ent_arc[e]; k < T.ent_arc[e + 1]; ++k) a.add(row[T.e_src[k]] + T.e_w[k]);
      row[q] = a.value();
    }
    __syncthreads();
  }
}

template <bool kLds>
__global__ void __launch_bounds__(kLanes) sum_trellis_kernel(DecodeTables T, SumLines D) {
  extern __shared__ double lds_rows[];
  const int lane = threadIdx.x;
  const uint32_t line = D.order[blockIdx.x];
  const uint32_t Q = T.n_states;
  double* cur = kLds ? lds_rows : D.rows + (size_t)line * 2 * Q;
  double* nxt = cur + Q;
  const uint64_t s0 = D.off[line];
  const uint32_t n = (uint32_t)(D.off[line + 1] - s0);
  for (uint32_t q = lane; q < Q; q += kLanes) cur[q] = q == 0 ? 0.0 : NEG_INF;  // (Lse of the single term 0.0 is 0.0)
  __syncthreads();
  sum_close(T, cur, 0, 0, cur, lane, true);
  for (uint32_t i = 0; i < n; ++i) {
    for (uint32_t q = lane; q < Q; q += kLanes) nxt[q] = NEG_INF;
    __syncthreads();
    const uint32_t x = D.sym[s0 + i];
    const bool known = x < T.n_syms;  // (a symbol no arc matches leaves the row at -inf: no derivation)
    const uint32_t g0 = known ? T.sym_seg[x] : 0, g1 = known ? T.sym_seg[x + 1] : 0;
    for (uint32_t g = g0 + lane; g < g1; g += kLanes) {
      const uint32_t q = T.seg_dst[g];
      if (D.eps_in[q]) continue;  // summed with its epsilon arcs, at its level
      Lse a;
      a.init();
      for (uint32_t k = T.seg_arc[g]; k < T.seg_arc[g + 1]; ++k) a.add(cur[T.m_src[k]] + T.m_w[k]);
      nxt[q] = a.value();
    }
    __syncthreads();
    sum_close(T, cur, g0, g1, nxt, lane, false);
    double* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (lane == 0) D.sum[line] = cur[T.final_state];
}
}  // namespace

extern "C" {

int carmel_hip_decode_sum(carmel_hip_decoder* d, uint64_t n_lines, const uint64_t* off, const uint32_t* sym, double* sum_logw) {
  if (!d || !off || !sum_logw || (off[n_lines] && !sym)) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decode_sum: bad argument");
  for (uint64_t l = 0; l < n_lines; ++l)
    if (off[l + 1] < off[l] || off[l + 1] - off[l] >= kNone) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decode_sum: bad line offsets");
  if (d->eps_cyclic)  // (the reference's sum is "acyclic-correct only", carmel.cc:1787: refused, not approximated)
    return fail(CARMEL_HIP_ERR_UNSUPPORTED,
                "carmel_hip_decode_sum: the epsilon arcs of the matched side have a cycle; the sum of all paths over an epsilon "
                "cycle is not supported");
  HIPCHK(hipSetDevice(d->device));
  hipStream_t s = d->stream;
  const uint32_t Q = d->n_states;
  const bool lds = Q <= kLdsStates && !lib_opt_off("decode_lds");
  // lines go in chunks, in line order, whose symbols (and global-tier rows) fit the budget ("decode_chunk_bytes", default 1 GiB;
  // a single line larger than it goes alone): there are no back-pointers to hold
  uint64_t budget = 1ull << 30;
  if (const char* v = lib_opt("decode_chunk_bytes")) budget = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10));
  auto line_bytes = [&](uint64_t l) { return (off[l + 1] - off[l]) * 4ull + (lds ? 0 : 16ull * Q); };
  float total_ms = 0;
  DevBuf<uint64_t> d_off;
  DevBuf<uint32_t> d_sym, d_order;
  DevBuf<double> d_rows, d_sum;
  for (uint64_t lo = 0; lo < n_lines;) {
    uint64_t hi = lo + 1, bytes = line_bytes(lo);
    while (hi < n_lines && hi - lo < (1u << 24) && bytes + line_bytes(hi) <= budget) bytes += line_bytes(hi++);
    const uint32_t n = (uint32_t)(hi - lo);
    std::vector<uint64_t> h_off(n + 1);
    for (uint32_t l = 0; l <= n; ++l) h_off[l] = off[lo + l] - off[lo];
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return h_off[a + 1] - h_off[a] > h_off[b + 1] - h_off[b]; });
    HIPCHK(d_off.upload(h_off, s));
    const std::vector<uint32_t> h_sym(sym + off[lo], sym + off[hi]);  // (named: the copy is asynchronous)
    HIPCHK(d_sym.upload(h_sym, s));
    HIPCHK(d_order.upload(order, s));
    if (!lds) HIPCHK(d_rows.alloc((size_t)n * 2 * Q));
    HIPCHK(d_sum.alloc(n));
    SumLines D{d_off.p, d_sym.p, d_order.p, lds ? nullptr : d_rows.p, d->eps_in.p, d_sum.p};
    HIPCHK(hipEventRecord(d->ev0, s));
    if (lds)
      sum_trellis_kernel<true><<<n, kLanes, 16 * (size_t)Q, s>>>(d->T, D);
    else
      sum_trellis_kernel<false><<<n, kLanes, 0, s>>>(d->T, D);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(d->ev1, s));
    HIPCHK(hipMemcpyAsync(sum_logw + lo, d_sum.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, d->ev0, d->ev1));
    total_ms += ms;
    lo = hi;
  }
  d->last_ms = total_ms;
  return CARMEL_HIP_OK;
}

}  // extern "C"
