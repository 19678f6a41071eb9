// decode_posterior.hip — batch arc posteriors: how often every arc of one (composed) transducer is used, in expectation, over all
// the derivations of a batch of lines -- the E-step of carmel -t (train.cc's forward/backward, train.cc:254-266, 698-860) stated for
// one-sided lines against a machine that is composed once.  It stands beside the best derivation (decode.hip), the K best
// (decode_kbest.hip), the sum of all (decode_sum.hip) and N drawn from the posterior (decode_sample.hip).  Derivation, matched
// side, dropped zero-weight arcs, the empty line, unknown symbols: decode_kbest.hip's and decode_sum.hip's.
//
// Forward.  alpha[i][q], i = 0 .. n = len(x), is the sampler's forward pass (decode_sample_node.hpp's SampleNode in
// decode_trellis.hpp's kernel): every row kept in global memory, Z = alpha[n][final] bit for bit carmel_hip_decode_sum's value.
//
// Backward (decode_posterior_kernel).  beta[i][q] has ONE streaming accumulator (sweep_math.hpp's Lse), owned by one lane, fed in
// this order and read out once:
//   0.0 first, at node (n, final) only;
//   if i < n the matched arcs OUT of q labelled x_{i+1}, in arc-id order: beta[i + 1][dst] + w;
//   the epsilon arcs OUT of q, in arc-id order: beta[i][dst] + w (their destinations are of strictly higher epsilon level: final
//   since the barrier that ended that level -- a row is closed from the highest source level down, trellis_close mirrored).
// A node with alpha = -inf is skipped (its beta stays -inf: nothing reads it for a count).
//
// Counts.  A trellis edge is a matched arc a at position i = 1 .. n or an epsilon arc a in row i = 0 .. n; its posterior is
// p = exp((alpha[.][src] + w) + beta[i][dst] - Z), the bracketed sum formed first, alpha's row i - 1 for a matched arc and i for
// an epsilon arc; a -inf anywhere gives 0.  The lane that feeds the edge's candidate into its node's accumulator forms p and, if
// p > 0, adds c_l p to count[a] in global memory with the hardware f64 atomic: arc_count[a] is the sum over the lines l with
// Z_l > -inf and over their edges that are arc a, c_l the line's weight (1 without weights).  A line without a derivation, or of
// weight 0, adds nothing: its backward pass is not run.
//
// What is fixed: sum_logw to the bit (the forward pass is the sum's); arc_count up to the order of the atomic adds -- every term
// c_l p is fixed to the bit, whatever the tier, the chunking or the launch order; the order in which the terms of one arc are added
// is not.
//
// Rows: two beta rows of |Q| doubles, in LDS when |Q| <= kLdsStates, otherwise the line's two rows of the global tier (the forward
// pass has finished with them); decode_lds=0 applies.  Only acyclic epsilon subgraphs have levels: a cyclic one is refused before
// any launch, as for the sum.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include "decode_sample_node.hpp"
#include "decode_trellis.hpp"
#include "engine.hpp"

namespace {
// what the backward kernel takes beside the tables and the lines
struct PosteriorBack {
  const uint64_t* a_off;  // [n + 1]: each line's (len + 1) x |Q| doubles
  const double* alpha;
  const double* weight;  // [n] line weights; nullptr: every line weighs 1
  double* sum;           // [n]: Z
  double* count;         // [n_arcs]
};

// a line's constants in the backward pass
struct PosteriorLine {
  const double* A;  // its alpha rows
  double Z, c;
  double* count;
};

// node (i, q): beta from the matched arcs [m0, m1) (destinations in row `next`, i + 1) and the epsilon arcs [e0, e1) (destinations
// in row `row`, i), into state q of `row`, and every such edge's share of the counts; last: the node is (n, final)
__device__ __forceinline__ void posterior_fill(const DecodeTables& T, const DecodeOutTables& O, const PosteriorLine& P, uint32_t i,
                                               uint32_t q, const double* next, uint32_t m0, uint32_t m1, double* row, uint32_t e0,
                                               uint32_t e1, bool last) {
  const double a = P.A[(size_t)i * T.n_states + q];
  if (!(a > NEG_INF)) return;  // (no derivation passes here: the row keeps its -inf)
  Lse b;
  b.init();
  if (last) b.add(0.0);
  for (uint32_t k = m0; k < m1; ++k) {
    const double w = O.m_w[k], bd = next[O.m_dst[k]];
    b.add(bd + w);
    if (bd > NEG_INF) {
      const double p = K_EXP(((a + w) + bd) - P.Z);
      if (p > 0.0) unsafeAtomicAdd(P.count + O.m_id[k], P.c * p);  // hardware global_atomic_add_f64 (no CAS loop)
    }
  }
  for (uint32_t k = e0; k < e1; ++k) {
    const double w = O.e_w[k], bd = row[O.e_dst[k]];
    b.add(bd + w);
    if (bd > NEG_INF) {
      const double p = K_EXP(((a + w) + bd) - P.Z);
      if (p > 0.0) unsafeAtomicAdd(P.count + O.e_id[k], P.c * p);
    }
  }
  row[q] = b.value();
}

// the nodes of row i that epsilon arcs leave, from the highest source level down; [g0, g1) are the source segments of symbol
// x_{i+1} (empty in row n, the `last`)
__device__ void posterior_close(const DecodeTables& T, const DecodeOutTables& O, const PosteriorLine& P, uint32_t i,
                                const double* next, uint32_t g0, uint32_t g1, double* row, int lane, bool last) {
  for (uint32_t L = T.n_levels; L-- > 0;) {
    for (uint32_t e = O.lvl_ent[L] + lane; e < O.lvl_ent[L + 1]; e += kLanes) {
      const uint32_t q = O.ent_src[e];
      uint32_t lo = g0, hi = g1;  // the segment of source q, if the symbol has one (seg_src ascends within a symbol)
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (O.seg_src[mid] < q)
          lo = mid + 1;
        else
          hi = mid;
      }
      const bool has = lo < g1 && O.seg_src[lo] == q;
      const uint32_t m0 = has ? O.seg_arc[lo] : 0, m1 = has ? O.seg_arc[lo + 1] : 0;
      posterior_fill(T, O, P, i, q, next, m0, m1, row, O.ent_arc[e], O.ent_arc[e + 1], last && q == T.final_state);
    }
    __syncthreads();
  }
}

// one wavefront = one workgroup of 64 lanes per line, in the chunk's launch order.  Order within a row: first the nodes that no
// epsilon arc leaves (one lane per source segment of the symbol); then, level by level downwards, the nodes that epsilon arcs
// leave (one lane per entry), each filled from both kinds of arc in one pass.  Barriers are the forward kernel's: after the row is
// cleared, after the matched phase, after every level.  No lane reads a node that another is writing.
template <bool kLds>
__global__ void __launch_bounds__(kLanes) decode_posterior_kernel(DecodeTables T, DecodeOutTables O, DecodeLines D, PosteriorBack B) {
  extern __shared__ double lds_rows[];
  const int lane = threadIdx.x;
  const uint32_t line = D.order[blockIdx.x];
  const uint32_t Q = T.n_states;
  const uint64_t s0 = D.off[line];
  const uint32_t n = (uint32_t)(D.off[line + 1] - s0);
  const double* A = B.alpha + B.a_off[line];
  const double Z = A[(size_t)n * Q + T.final_state];
  const double c = B.weight ? B.weight[line] : 1.0;
  if (lane == 0) B.sum[line] = Z;
  if (!(Z > NEG_INF) || !(c > 0.0)) return;  // (the whole workgroup: nothing to add)
  const PosteriorLine P{A, Z, c, B.count};
  double* row = kLds ? lds_rows : D.rows + (size_t)line * 2 * Q;  // row i
  double* next = row + Q;                                          // row i + 1
  for (uint32_t q = lane; q < Q; q += kLanes) row[q] = q == T.final_state ? 0.0 : NEG_INF;  // (n, final): one value, 0.0
  __syncthreads();
  posterior_close(T, O, P, n, next, 0, 0, row, lane, true);
  for (uint32_t i = n; i-- > 0;) {
    double* t = row;
    row = next;
    next = t;
    for (uint32_t q = lane; q < Q; q += kLanes) row[q] = NEG_INF;
    __syncthreads();
    const uint32_t x = D.sym[s0 + i];  // x_{i+1}, known: the line has a derivation
    const uint32_t g0 = x < T.n_syms ? O.sym_seg[x] : 0, g1 = x < T.n_syms ? O.sym_seg[x + 1] : 0;
    for (uint32_t g = g0 + lane; g < g1; g += kLanes) {
      const uint32_t q = O.seg_src[g];
      if (O.eps_out[q]) continue;  // filled with its epsilon arcs, at its level
      posterior_fill(T, O, P, i, q, next, O.seg_arc[g], O.seg_arc[g + 1], row, 0, 0, false);
    }
    __syncthreads();
    posterior_close(T, O, P, i, next, g0, g1, row, lane, false);
  }
}
}  // namespace

extern "C" {

int carmel_hip_decode_posterior(carmel_hip_decoder* d, uint64_t n_lines, const uint64_t* off, const uint32_t* sym,
                                const double* line_weight, double* sum_logw, double* arc_count) {
  const char* who = "carmel_hip_decode_posterior";
  if (!d || !off || !arc_count || (off[n_lines] && !sym)) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decode_posterior: bad argument");
  if (const int rc = decode_check_lines(who, n_lines, off)) return rc;
  if (line_weight)
    for (uint64_t l = 0; l < n_lines; ++l)
      if (!(line_weight[l] >= 0.0) || !std::isfinite(line_weight[l]))
        return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decode_posterior: a line weight is negative or not finite");
  if (d->eps_cyclic)  // (the forward pass is the sum's: no levels, no sum)
    return fail(CARMEL_HIP_ERR_UNSUPPORTED,
                "carmel_hip_decode_posterior: the epsilon arcs of the matched side have a cycle; arc posteriors over an epsilon "
                "cycle are not supported");
  const uint32_t Q = d->n_states;
  HIPCHK(hipSetDevice(d->device));  // (the counts below are zeroed before the chunk driver sets it)
  hipStream_t s = d->stream;
  if (d->count.n != d->n_arcs) HIPCHK(d->count.alloc(d->n_arcs));
  if (d->n_arcs) HIPCHK(hipMemsetAsync(d->count.p, 0, d->n_arcs * sizeof(double), s));  // once per call: every chunk adds to it
  std::vector<double> r_sum(n_lines);
  DevBuf<uint64_t> d_aoff;
  DevBuf<uint32_t> d_has;
  DevBuf<double> d_alpha, d_sum, d_weight;
  // a line costs its symbols and its (len + 1) rows of |Q| doubles: the sampler's cost less the per-sample terms
  const int rc = decode_chunks(d, n_lines, off, sym, 8ull * Q + 4, 8ull * Q, 1u << 24, Q, [&](DecodeChunk& c) {
    const uint32_t n = c.n;
    std::vector<uint64_t> h_aoff(n + 1, 0);
    for (uint32_t l = 0; l < n; ++l) h_aoff[l + 1] = h_aoff[l] + (c.h_off[l + 1] - c.h_off[l] + 1) * Q;
    std::vector<double> h_weight;  // (named: the copy is asynchronous)
    if (line_weight) h_weight.assign(line_weight + c.lo, line_weight + c.hi);
    HIPCHK(d_aoff.upload(h_aoff, s));
    HIPCHK(d_alpha.alloc(h_aoff[n]));
    HIPCHK(d_has.alloc(n));
    HIPCHK(d_sum.alloc(n));
    if (line_weight) HIPCHK(d_weight.upload(h_weight, s));
    const PosteriorBack B{d_aoff.p, d_alpha.p, line_weight ? d_weight.p : nullptr, d_sum.p, d->count.p};
    if (const int rc = c.begin()) return rc;
    launch_trellis(d, c.lds, n, c.L, SampleNode{d_aoff.p, d_alpha.p, d_has.p}, s);
    if (c.lds)
      decode_posterior_kernel<true><<<n, kLanes, 16 * (size_t)Q, s>>>(d->T, d->TO, c.L, B);
    else
      decode_posterior_kernel<false><<<n, kLanes, 0, s>>>(d->T, d->TO, c.L, B);
    if (const int rc = c.end()) return rc;
    HIPCHK(hipMemcpyAsync(r_sum.data() + c.lo, d_sum.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    return c.wait();
  });
  if (rc) return rc;
  if (d->n_arcs) {
    HIPCHK(hipMemcpyAsync(arc_count, d->count.p, d->n_arcs * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  if (sum_logw && n_lines) std::memcpy(sum_logw, r_sum.data(), n_lines * sizeof(double));
  return CARMEL_HIP_OK;
}

}  // extern "C"
