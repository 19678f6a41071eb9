// decode_sample.hip — batch posterior path sampling: for every line x of a batch, N derivations of x against one (composed)
// transducer, each drawn with probability P(d | x) = w(d) / (the sum over all derivations of x), independently.  It stands
// beside the best derivation (decode.hip), the K best (decode_kbest.hip) and the sum of all (decode_sum.hip); it is NOT the
// reference's -G n, which walks the whole machine forward by locally normalised arc weights and retries on dead ends
// (fst.h:708-757, carmel.cc:1446-1458): that is decode_generate.hip.  Forward pass and backward sampling: the forward pass is decode_sum.hip's
// (the same node arithmetic, decode_sum_node.hpp, in decode_trellis.hpp's kernel) but keeps every row; the walk samples an arc
// into the node it stands on with probability proportional to (the source node's forward value) x (the arc's weight).
// Derivation, matched side, dropped zero-weight arcs, the empty line, unknown symbols: decode_kbest.hip's and decode_sum.hip's.
//
// Forward.  alpha[i][q], i = 0 .. len(x), is the value of node (i, q) exactly as the sum computes it; a node nothing reaches is
// -inf.  alpha[n][final] is bit for bit what carmel_hip_decode_sum returns for the line.  A line's (len + 1) |Q| doubles are in a
// global array (SampleNode): begin() fills them with -inf (the walk reads nodes the trellis never fills) and fill() stores each
// node's value beside the row the trellis keeps.
//
// Backward walk of sample s of the call's line l (decode_sample_walk_kernel).  From (i, q) = (n, final), step = 0; at node (i, q)
// the candidates are, in this order,
//   "stop", value 0.0, if (i, q) = (0, 0);
//   if i > 0 the matched arcs into q labelled x_i, in arc-id order, value alpha[i - 1][src] + w;
//   the epsilon arcs into q, in arc-id order, value alpha[i][src] + w.
// With Z = alpha[i][q]: p_c = exp(value_c - Z) (0 for a value of -inf), S = the p_c added in candidate order in f64,
// u = gibbs_uniform(seed, s, l, step) (rng.hpp; l is the line's index in the CALL), t = u S.  The choice is the first candidate
// with p_c > 0 whose running sum (same order) exceeds t, or the last candidate with p_c > 0 if none does.  "Stop" ends the walk;
// otherwise the arc is prepended to the path, step is incremented, q becomes the arc's source, and i is decremented for a matched
// arc only.  So sample s of line l depends on (machine, weights, side, x, seed, l, s) and on nothing else: not on the memory
// tier, the chunking, the launch order or the other lines.
//
// A line with alpha[n][final] = -inf gets no paths, every other line exactly N, in sample order, duplicates kept.  The weight
// reported for a path is its arcs added from the end, w1 + (w2 + (... + (wn + 0))), as for 1-best and k-best: the walk meets the
// arcs in that order.  Only acyclic epsilon subgraphs have levels: a cyclic one is refused before any launch, as for the sum.
#include <hip/hip_runtime.h>
#include <cstring>
#include <limits>
#include <vector>
#include "decode_sample_node.hpp"
#include "decode_trellis.hpp"
#include "engine.hpp"
#include "rng.hpp"

namespace {
constexpr uint32_t kMaxSamples = 65536;

// (the skeleton's node, SampleNode -- the sum's, and every node's value kept for the walk -- is decode_sample_node.hpp's, shared
// with decode_posterior.hip)
// what the walk kernel takes beside the tables and the lines
struct SampleWalk {
  uint32_t n_lines, n_samples;
  uint64_t seed, line0, n_arcs;  // line0: the call's index of the chunk's first line
  const uint64_t* a_off;
  const double* alpha;
  const uint32_t* has;
  uint32_t* len;             // [n_lines x n_samples]
  double* logw;
  const uint64_t* path_off;  // the writing pass: [n_lines x n_samples + 1]
  uint32_t* path;
  int* err;
};

// one lane per (line, sample s): slot line * N + s, so adjacent lanes share a line's alpha rows; idle if the line has no
// derivation.  kWrite = false counts the path's arcs into len[slot] and adds their weights from the end into logw[slot];
// kWrite = true writes the arcs in path order at path[path_off[slot] ..).  Both passes derive the same choices from the same
// counters.  A node's candidates are visited twice (S, then the running sum): no array per candidate is kept.
template <bool kWrite>
__global__ void __launch_bounds__(256) decode_sample_walk_kernel(DecodeTables T, DecodeLines D, SampleWalk W) {
  const uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (a chunk has at most 2^24 slots: the driver's cap)
  if (slot >= (uint64_t)W.n_lines * W.n_samples) return;
  const uint32_t line = (uint32_t)(slot / W.n_samples), s = (uint32_t)(slot % W.n_samples);
  if (!W.has[line]) return;
  const double ninf = -std::numeric_limits<double>::infinity();
  const uint32_t Q = T.n_states;
  const uint64_t s0 = D.off[line];
  const uint32_t n = (uint32_t)(D.off[line + 1] - s0);
  const double* A = W.alpha + W.a_off[line];
  const uint32_t block = (uint32_t)(W.line0 + line);
  const uint64_t cap = (uint64_t)(n + 1) * (T.n_levels + 1);  // a position has one matched arc and n_levels epsilon arcs at most
  const uint32_t n_path = kWrite ? W.len[slot] : 0;
  uint32_t i = n, q = T.final_state, steps = 0;
  double w = 0.0;
  while (true) {
    const double Z = A[(size_t)i * Q + q];
    const bool stop = i == 0 && q == 0;
    uint32_t m0 = 0, m1 = 0, e0 = 0, e1 = 0;
    if (i > 0) {
      const uint32_t x = D.sym[s0 + i - 1];
      if (x < T.n_syms) {  // the segment of destination q, if the symbol has one (seg_dst ascends within a symbol)
        const uint32_t g1 = T.sym_seg[x + 1];
        uint32_t lo = T.sym_seg[x], hi = g1;
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
    }
    const uint32_t ent = T.st_ent[q];
    if (ent != kNone) {
      e0 = T.ent_arc[ent];
      e1 = T.ent_arc[ent + 1];
    }
    const double* prev = A + (size_t)(i ? i - 1 : 0) * Q;  // (read only if i > 0: m0 == m1 otherwise)
    const double* same = A + (size_t)i * Q;
    auto prob = [&](double v) { return v > ninf ? exp(v - Z) : 0.0; };
    double S = 0.0;
    if (stop) S += prob(0.0);
    for (uint32_t k = m0; k < m1; ++k) S += prob(prev[T.m_src[k]] + T.m_w[k]);
    for (uint32_t k = e0; k < e1; ++k) S += prob(same[T.e_src[k]] + T.e_w[k]);
    const double t = gibbs_uniform(W.seed, s, block, steps) * S;
    // the choice: kind 0 none yet, 1 stop, 2 matched arc `at`, 3 epsilon arc `at`
    int kind = 0;
    uint32_t at = 0;
    double run = 0.0;
    bool found = false;
    if (stop) {
      const double p = prob(0.0);
      if (p > 0.0) {
        kind = 1;
        run += p;
        found = run > t;
      }
    }
    for (uint32_t k = m0; k < m1 && !found; ++k) {
      const double p = prob(prev[T.m_src[k]] + T.m_w[k]);
      if (p > 0.0) {
        kind = 2;
        at = k;
        run += p;
        found = run > t;
      }
    }
    for (uint32_t k = e0; k < e1 && !found; ++k) {
      const double p = prob(same[T.e_src[k]] + T.e_w[k]);
      if (p > 0.0) {
        kind = 3;
        at = k;
        run += p;
        found = run > t;
      }
    }
    if (kind == 1) break;
    const uint32_t a = kind == 2 ? T.m_id[at] : kind == 3 ? T.e_id[at] : kNone;
    if (kind == 0 || a >= W.n_arcs || steps >= cap || (kWrite && steps >= n_path)) {  // (kind 0: a node with no way back)
      atomicOr(W.err, kErrWalk);
      return;
    }
    ++steps;
    if (kWrite) W.path[W.path_off[slot] + n_path - steps] = a;
    if (kind == 2) {
      w = T.m_w[at] + w;
      q = T.m_src[at];
      --i;
    } else {
      w = T.e_w[at] + w;
      q = T.e_src[at];
    }
  }
  // ("stop" is a candidate at (0, 0) only: the walk has arrived)
  if (kWrite) {
    if (steps != n_path) atomicOr(W.err, kErrWalk);
  } else {
    W.len[slot] = steps;
    W.logw[slot] = w;
  }
}
}  // namespace

extern "C" {

int carmel_hip_decode_sample(carmel_hip_decoder* d, uint32_t n_samples, uint64_t seed, uint64_t n_lines, const uint64_t* off,
                             const uint32_t* sym, uint64_t* line_paths) {
  const char* who = "carmel_hip_decode_sample";
  if (!d || !off || !line_paths || (off[n_lines] && !sym)) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decode_sample: bad argument");
  if (n_samples < 1 || n_samples > kMaxSamples)
    return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decode_sample: n_samples must be in 1 .. 65536");
  if (n_lines >= (1ull << 32)) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decode_sample: more than 2^32 - 1 lines");
  if (const int rc = decode_check_lines(who, n_lines, off)) return rc;
  if (d->eps_cyclic)  // (the forward pass is the sum's: no levels, no sum)
    return fail(CARMEL_HIP_ERR_UNSUPPORTED,
                "carmel_hip_decode_sample: the epsilon arcs of the matched side have a cycle; sampling paths over an epsilon "
                "cycle is not supported");
  const uint32_t N = n_samples, Q = d->n_states;
  const std::string bad = std::string(who) + ": inconsistent sample walk";
  HIPCHK(hipSetDevice(d->device));  // (d_err below is allocated before the chunk driver sets it)
  std::vector<double> r_logw;
  std::vector<uint64_t> r_off(1, 0);
  std::vector<uint32_t> r_arcs;
  line_paths[0] = 0;
  DevBuf<uint64_t> d_aoff, d_poff;
  DevBuf<uint32_t> d_has, d_len, d_path;
  DevBuf<double> d_alpha, d_logw;
  DevBuf<int> d_err;
  HIPCHK(d_err.alloc(1));
  // a line costs its symbols and its (len + 1) rows of |Q| doubles, and per sample a length and a weight
  const int rc = decode_chunks(d, n_lines, off, sym, 8ull * Q + 4, 8ull * Q + 8ull * N, (1u << 24) / N, Q, [&](DecodeChunk& c) {
    hipStream_t s = d->stream;
    const uint32_t n = c.n;
    const uint64_t n_slots = (uint64_t)n * N;
    std::vector<uint64_t> h_aoff(n + 1, 0);
    for (uint32_t l = 0; l < n; ++l) h_aoff[l + 1] = h_aoff[l] + (c.h_off[l + 1] - c.h_off[l] + 1) * Q;
    HIPCHK(d_aoff.upload(h_aoff, s));
    HIPCHK(d_alpha.alloc(h_aoff[n]));
    HIPCHK(d_has.alloc(n));
    HIPCHK(d_len.alloc(n_slots));
    HIPCHK(d_logw.alloc(n_slots));
    HIPCHK(hipMemsetAsync(d_err.p, 0, sizeof(int), s));
    const uint32_t wb = (uint32_t)((n_slots + 255) / 256);
    auto walk = [&](bool write) {
      const SampleWalk W{n, N, seed, c.lo, d->n_arcs, d_aoff.p, d_alpha.p, d_has.p, d_len.p, d_logw.p, d_poff.p, d_path.p, d_err.p};
      (write ? decode_sample_walk_kernel<true> : decode_sample_walk_kernel<false>)<<<wb, 256, 0, s>>>(d->T, c.L, W);
    };
    if (const int rc = c.begin()) return rc;
    launch_trellis(d, c.lds, n, c.L, SampleNode{d_aoff.p, d_alpha.p, d_has.p}, s);
    walk(false);
    if (const int rc = c.end()) return rc;
    std::vector<uint32_t> np(n), len(n_slots);
    std::vector<double> lw(n_slots);
    int err = 0;
    HIPCHK(hipMemcpyAsync(np.data(), d_has.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(len.data(), d_len.p, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(lw.data(), d_logw.p, n_slots * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    if (const int rc = c.wait()) return rc;
    if (err) return fail(CARMEL_HIP_ERR_STATE, bad);
    for (uint32_t l = 0; l < n; ++l) {
      if (np[l] > 1) return fail(CARMEL_HIP_ERR_STATE, bad);
      np[l] *= N;  // all of its samples or none
    }
    const uint64_t base = r_arcs.size();
    const std::vector<uint64_t> h_poff = decode_collect_paths(c, N, np, len, lw, base, line_paths, r_logw, r_off);
    if (!h_poff[n_slots]) return CARMEL_HIP_OK;
    HIPCHK(d_poff.upload(h_poff, s));
    HIPCHK(d_path.alloc(h_poff[n_slots]));
    if (const int rc = c.begin()) return rc;
    walk(true);
    if (const int rc = c.end()) return rc;
    r_arcs.resize(base + h_poff[n_slots]);
    HIPCHK(hipMemcpyAsync(r_arcs.data() + base, d_path.p, h_poff[n_slots] * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    if (const int rc = c.wait()) return rc;
    return err ? fail(CARMEL_HIP_ERR_STATE, bad) : CARMEL_HIP_OK;
  });
  if (rc) return rc;
  d->kb_logw.swap(r_logw);
  d->kb_off.swap(r_off);
  d->kb_arcs.swap(r_arcs);
  return CARMEL_HIP_OK;
}

}  // extern "C"
