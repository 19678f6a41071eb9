// decode_pairs_sample.hip — batch pair alignment sampling: for every pair (x, y) of a batch, N derivations of the pair against
// one (composed) transducer, each drawn with probability P(d | x, y) = w(d) / (the sum over all derivations of the pair),
// independently.  It is to carmel_hip_decode_pairs_sum what decode_sample.hip is to the one-sided sum, and stands beside the
// pairs' Viterbi alignment and sum (decode_pairs.hip) and their arc posteriors (decode_pairs_posterior.hip).  Pair, derivation,
// matched side, the four kinds of arc (MM, M0, 0M, 00), the 00 levels, dropped zero-weight arcs, unknown symbols:
// decode_pairs.hip's.
//
// Forward.  decode_pairs_trellis.hpp's pair_trellis_kernel with KeepAcc, exactly as the arc posteriors run it: every pair's
// alpha plane of (n + 1)(m + 1)|Q| doubles in global memory, slot (i (m + 1) + j)|Q| + q, -inf where nothing reaches;
// alpha[n][m][final] is bit for bit carmel_hip_decode_pairs_sum's value.  A pair has a derivation iff it is > -inf.
//
// Backward walk of sample s of the call's pair l (pair_sample_walk_kernel).  From (i, j, q) = (n, m, final), step = 0; at node
// (i, j, q) the candidates are, in this order,
//   "stop", value 0.0, at (0, 0, 0) only;
//   if i > 0 the arcs into q whose matched symbol is x_i, in arc-id order, MM and M0 as their ids fall: an M0 arc (other symbol
//   epsilon) has value alpha[i - 1][j][src] + w; an MM arc is a candidate only if j > 0 and its other symbol is y_j, value
//   alpha[i - 1][j - 1][src] + w;
//   the matched-side-epsilon arcs into q, in arc-id order, 0M and 00 as their ids fall: a 00 arc has value alpha[i][j][src] + w;
//   a 0M arc is a candidate only if j > 0 and its other symbol is y_j, value alpha[i][j - 1][src] + w.
// With Z = alpha[i][j][q]: p_c = exp(value_c - Z) (0 for a value of -inf), S = the p_c added in candidate order in f64,
// u = gibbs_uniform(seed, s, l, step) (rng.hpp; l is the pair's index in the CALL), t = u S.  The choice is the first candidate
// with p_c > 0 whose running sum (same order) exceeds t, or the last candidate with p_c > 0 if none does.  "Stop" ends the walk;
// otherwise the arc is prepended to the path, step is incremented, q becomes the arc's source, i is decremented if the arc's
// matched symbol is not epsilon and j if its other symbol is not.  So sample s of pair l depends on (machine, weights, side, x,
// y, seed, l, s) and on nothing else: not on the memory tier, the chunking, the launch order or the other pairs.
//
// A pair without a derivation gets no paths, every other pair exactly N, in sample order, duplicates kept.  The weight reported
// for a path is its arcs added from the end, w1 + (w2 + (... + (wn + 0))), as everywhere else.  The walk checks what
// decode_pairs.hip's walk checks: the arc range, a step cap of (n + m + 1)(levels + 1), and the arrival at (0, 0, 0) -- "stop" is
// a candidate there only, and a node without a candidate of p > 0 is an error.
//
// A state's matched-side-epsilon arcs are found through DecodePairTables::st_ent (the entry whose destination the state is: by
// the 00 levels, which a 0M self-loop leaves standing; DecodeTables::st_ent is by the matched side's levels and would not do),
// the matched segment of (x_i, q) by the binary search of decode_sample.hip's walk.  A pair costs 8 (n + 1)(m + 1)|Q| bytes for
// its plane, 4 (n + m) for its symbols, 24 (min(n, m) + 1)|Q| in the global tier and 12 N for its samples' lengths and weights.
#include <hip/hip_runtime.h>
#include <cstring>
#include <limits>
#include <string>
#include <vector>
#include "decode_pairs_trellis.hpp"
#include "rng.hpp"

namespace {
constexpr uint32_t kMaxSamples = 65536;

// what the walk kernel takes beside the tables and the pairs
struct PairSampleWalk {
  uint32_t n_pairs, n_samples;
  uint64_t seed, pair0, n_arcs;  // pair0: the call's index of the chunk's first pair
  uint32_t levels;               // the highest 00 level
  const uint64_t* a_off;
  const double* alpha;
  uint32_t* has;             // [n_pairs]: 1 if the pair has a derivation (written by the counting pass)
  uint32_t* len;             // [n_pairs x n_samples]
  double* logw;
  const uint64_t* path_off;  // the writing pass: [n_pairs x n_samples + 1]
  uint32_t* path;
  int* err;
};

// one lane per (pair, sample s): slot pair * N + s, so adjacent lanes share a pair's alpha plane; idle if the pair has no
// derivation.  kWrite = false counts the path's arcs into len[slot] and adds their weights from the end into logw[slot];
// kWrite = true writes the arcs in path order at path[path_off[slot] ..).  Both passes derive the same choices from the same
// counters.  A node's candidates are visited twice (S, then the running sum): no array per candidate is kept.
template <bool kWrite>
__global__ void __launch_bounds__(256) pair_sample_walk_kernel(DecodeTables T, DecodePairTables P, PairLines D, PairSampleWalk W) {
  const uint64_t slot = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (a chunk has at most 2^24 slots: the driver's cap)
  if (slot >= (uint64_t)W.n_pairs * W.n_samples) return;
  const uint32_t pair = (uint32_t)(slot / W.n_samples), s = (uint32_t)(slot % W.n_samples);
  const double ninf = -std::numeric_limits<double>::infinity();
  const uint32_t Q = T.n_states;
  const uint32_t* x = D.sym + D.off[pair];
  const uint32_t n = (uint32_t)(D.off[pair + 1] - D.off[pair]);
  const uint32_t* y = D.sym2 + D.off2[pair];
  const uint32_t m = (uint32_t)(D.off2[pair + 1] - D.off2[pair]);
  const double* A = W.alpha + W.a_off[pair];
  const bool has = A[((size_t)n * (m + 1) + m) * Q + T.final_state] > ninf;
  if (!kWrite && s == 0) W.has[pair] = has;
  if (!has) return;
  const uint32_t block = (uint32_t)(W.pair0 + pair);
  const uint64_t cap = ((uint64_t)n + m + 1) * ((uint64_t)W.levels + 1);  // no path of the trellis is longer
  const uint32_t n_path = kWrite ? W.len[slot] : 0;
  uint32_t i = n, j = m, q = T.final_state, steps = 0;
  double w = 0.0;
  while (true) {
    const double* cell = A + ((size_t)i * (m + 1) + j) * Q;
    const double Z = cell[q];
    const bool stop = i == 0 && j == 0 && q == 0;
    uint32_t m0 = 0, m1 = 0, e0 = 0, e1 = 0;
    if (i > 0) {
      const uint32_t xi = x[i - 1];
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
    }
    const uint32_t ent = P.st_ent[q];
    if (ent != kNone) {
      e0 = P.ent_arc[ent];
      e1 = P.ent_arc[ent + 1];
    }
    const bool has_y = j > 0;
    const uint32_t yj = has_y ? y[j - 1] : 0;
    // (a cell beyond the pair is never read: M0 and MM need i > 0 -- m0 == m1 otherwise --, MM and 0M j > 0)
    const double* up = A + ((size_t)(i ? i - 1 : 0) * (m + 1) + j) * Q;                      // (i - 1, j)
    const double* diag = A + ((size_t)(i ? i - 1 : 0) * (m + 1) + (has_y ? j - 1 : 0)) * Q;  // (i - 1, j - 1)
    const double* left = A + ((size_t)i * (m + 1) + (has_y ? j - 1 : 0)) * Q;                // (i, j - 1)
    auto prob = [&](double v) { return v > ninf ? exp(v - Z) : 0.0; };
    // an arc that fails its test is no candidate: it counts as p = 0
    auto p_matched = [&](uint32_t k) {
      const uint32_t o = P.m_osym[k];
      if (o == 0) return prob(up[T.m_src[k]] + T.m_w[k]);
      if (has_y && o == yj) return prob(diag[T.m_src[k]] + T.m_w[k]);
      return 0.0;
    };
    auto p_eps = [&](uint32_t k) {
      const uint32_t o = P.e_osym[k];
      if (o == 0) return prob(cell[P.e_src[k]] + P.e_w[k]);
      if (has_y && o == yj) return prob(left[P.e_src[k]] + P.e_w[k]);
      return 0.0;
    };
    double S = 0.0;
    if (stop) S += prob(0.0);
    for (uint32_t k = m0; k < m1; ++k) S += p_matched(k);
    for (uint32_t k = e0; k < e1; ++k) S += p_eps(k);
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
      const double p = p_matched(k);
      if (p > 0.0) {
        kind = 2;
        at = k;
        run += p;
        found = run > t;
      }
    }
    for (uint32_t k = e0; k < e1 && !found; ++k) {
      const double p = p_eps(k);
      if (p > 0.0) {
        kind = 3;
        at = k;
        run += p;
        found = run > t;
      }
    }
    if (kind == 1) break;
    const uint32_t a = kind == 2 ? T.m_id[at] : kind == 3 ? P.e_id[at] : kNone;
    if (kind == 0 || a >= W.n_arcs || steps >= cap || (kWrite && steps >= n_path)) {  // (kind 0: a node with no way back)
      atomicOr(W.err, kErrWalk);
      return;
    }
    ++steps;
    if (kWrite) W.path[W.path_off[slot] + n_path - steps] = a;
    if (kind == 2) {
      w = T.m_w[at] + w;
      q = T.m_src[at];
      --i;  // (a matched arc is a candidate only if i > 0)
      if (P.m_osym[at] != 0) --j;  // (MM: only if j > 0)
    } else {
      w = P.e_w[at] + w;
      q = P.e_src[at];
      if (P.e_osym[at] != 0) --j;  // (0M: only if j > 0)
    }
  }
  // ("stop" is a candidate at (0, 0, 0) only: the walk has arrived)
  if (kWrite) {
    if (steps != n_path) atomicOr(W.err, kErrWalk);
  } else {
    W.len[slot] = steps;
    W.logw[slot] = w;
  }
}
}  // namespace

extern "C" {

int carmel_hip_decode_pairs_sample(carmel_hip_decoder* d, uint32_t n_samples, uint64_t seed, uint64_t n_pairs, const uint64_t* off,
                                   const uint32_t* sym, const uint64_t* off2, const uint32_t* sym2, uint64_t* line_paths) {
  const char* who = "carmel_hip_decode_pairs_sample";
  if (n_samples < 1 || n_samples > kMaxSamples)
    return fail(CARMEL_HIP_ERR_ARG, std::string(who) + ": n_samples must be in 1 .. 65536");
  PairCall call{d, n_pairs, off, off2};
  if (const int rc = call.check(who, sym, sym2, line_paths)) return rc;
  const uint32_t N = n_samples;
  const std::string bad = std::string(who) + ": inconsistent sample walk";
  HIPCHK(hipSetDevice(d->device));  // (d_err below is allocated before the chunk driver sets it)
  std::vector<double> r_logw;
  std::vector<uint64_t> r_off(1, 0);
  std::vector<uint32_t> r_arcs;
  line_paths[0] = 0;
  DevBuf<uint64_t> d_aoff, d_poff, d_rows_off;
  DevBuf<uint32_t> d_has, d_len, d_path;
  DevBuf<double> d_alpha, d_logw, d_rows;
  DevBuf<int> d_err;
  HIPCHK(d_err.alloc(1));
  // a pair costs its alpha plane, its symbols, in the global tier its three diagonals, and per sample a length and a weight
  auto cost = [&](uint64_t l) {
    return 8 * call.nodes(l) + 4 * (call.len1(l) + call.len2(l)) + (call.lds ? 0 : 24 * call.diag_doubles(l)) + 12ull * N;
  };
  const int rc = decode_chunks_by_cost(d, n_pairs, off, sym, off2, sym2, call.lds, cost, (1u << 24) / N, [&](DecodeChunk& c) {
    hipStream_t s = d->stream;
    const uint32_t n = c.n;
    const uint64_t n_slots = (uint64_t)n * N;
    std::vector<uint64_t> h_aoff(n + 1, 0);
    for (uint32_t l = 0; l < n; ++l) h_aoff[l + 1] = h_aoff[l] + call.nodes(c.lo + l);
    HIPCHK(d_aoff.upload(h_aoff, s));
    HIPCHK(d_alpha.alloc(h_aoff[n]));
    HIPCHK(d_has.alloc(n));
    HIPCHK(d_len.alloc(n_slots));
    HIPCHK(d_logw.alloc(n_slots));
    PairLines L;
    if (const int r = call.rows(c, d_rows, d_rows_off, L)) return r;
    HIPCHK(hipMemsetAsync(d_err.p, 0, sizeof(int), s));
    const uint32_t wb = (uint32_t)((n_slots + 255) / 256);
    auto walk = [&](bool write) {
      const PairSampleWalk W{n,       N,       seed,     c.lo,     d->n_arcs, d->pair_levels, d_aoff.p, d_alpha.p,
                             d_has.p, d_len.p, d_logw.p, d_poff.p, d_path.p,  d_err.p};
      (write ? pair_sample_walk_kernel<true> : pair_sample_walk_kernel<false>)<<<wb, 256, 0, s>>>(d->T, d->TP, L, W);
    };
    if (const int r = c.begin()) return r;
    launch_pairs<KeepAcc>(d, call.lds, call.lds_bytes, n, L, KeepOut{d_aoff.p, d_alpha.p}, s);
    walk(false);
    if (const int r = c.end()) return r;
    std::vector<uint32_t> np(n), len(n_slots);
    std::vector<double> lw(n_slots);
    int err = 0;
    HIPCHK(hipMemcpyAsync(np.data(), d_has.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(len.data(), d_len.p, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(lw.data(), d_logw.p, n_slots * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    if (const int r = c.wait()) return r;
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
