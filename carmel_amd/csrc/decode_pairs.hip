// decode_pairs.hip — batch pair decoding (carmel --post-b=FILE: a line and a second, parallel line for the other side,
// carmel.cc:569-597, 1781-1784): for many pairs (x, y) against one (composed) transducer, the pair's best derivation -- the
// Viterbi alignment -- and the sum of all its derivations.  The reference composes x, the machine and y per pair and searches or
// sums the result; here nothing is composed per pair: a trellis over (matched position i, other position j, state q), f64 log
// weights, one wavefront = one workgroup of 64 lanes per pair, pairs launched costliest first.
//
// A derivation of the pair (x, y): a path from state 0 to the final state that uses no arc of weight zero, whose matched-side
// symbols (epsilon dropped) spell x and whose other-side symbols (epsilon dropped) spell y; x is on the decoder's matched side.
// Two derivations differ if their arc-id sequences differ.  A symbol no arc carries, on either side, means no derivation.
//
// By (matched symbol a, other symbol b) an arc feeds node (i, j, dst) from
//   MM  a, b != 0, a = x_i and b = y_j   (i - 1, j - 1, src)
//   M0  a != 0, b = 0, a = x_i           (i - 1, j, src)
//   0M  a = 0, b != 0, b = y_j           (i, j - 1, src)
//   00  a = b = 0                        (i, j, src)
// so the nodes of anti-diagonal d = i + j depend on diagonals d - 1 and d - 2 and, through 00 arcs, on nodes of their own cell of
// strictly lower 00 level (DecodePairTables: the levels of the 00 subgraph alone; a 00 cycle is refused before any launch, 0M and
// M0 self-loops are ordinary arcs).  The kernel walks d = 0 .. n + m and keeps THREE diagonals, not planes: a diagonal holds
// (min(n, m) + 1) |Q| doubles, a cell indexed by its position on the shorter line.  They are in LDS when 3 (min(n, m) + 1) |Q| <=
// 8192 doubles (the 64 KiB the other decoders use) for the longest pair of the call, otherwise in a global buffer per pair; option
// decode_lds=0 forces the global tier.
//
// Order within a diagonal: the diagonal is cleared; barrier; every node (cell, q) whose state no matched-side-epsilon arc enters
// is filled by one lane from its MM / M0 arcs; barrier; then, 00 level by 00 level, every node whose state such arcs enter is
// filled ONCE, in one pass, by one lane, from its MM / M0 arcs, its 0M arcs and its 00 arcs (decode_trellis.hpp's trellis_close:
// never finished and patched afterwards); barrier after every level.  A node is owned by one lane; no lane reads a node another
// is writing.  The candidates of a node, in the order that fixes every bit:
//   0.0 first, at (0, 0, start) only;
//   the arcs into q labelled x_i in arc-id order, MM and M0 as their ids fall, an arc whose other symbol fails its test skipped;
//   the matched-side-epsilon arcs into q in arc-id order, 0M and 00 as their ids fall, a failing arc skipped.
// A candidate of -inf adds nothing.  Two accumulators run over that skeleton:
//   BestAcc (max, +): only a STRICTLY greater candidate replaces the value held, so a matched arc beats an equal epsilon arc and
//     the lowest arc id wins; one u32 back-pointer (arc id) per (i, j, q) in a global array of (n + 1)(m + 1)|Q| slots a pair;
//   SumAcc: sweep_math.hpp's Lse fed in that order and read out once, as decode_sum_node.hpp does; no back-pointers.
// The value the best trellis chooses by is the path-order sum ((0 + w1) + w2) + ...; the weight reported is the path's arcs added
// from the END, w1 + (w2 + (... + (wn + 0))), by the walk, as for 1-best (decode.hip's header).
//
// The trellis kernel, SumAcc and the host side of a call are in decode_pairs_trellis.hpp, which decode_pairs_posterior.hip (the
// pairs' arc posteriors) shares; BestAcc and the walk are here.
//
// The walk: one lane per pair follows the back-pointers from (n, m, final) to (0, 0, start): i drops if the arc's matched symbol
// is not epsilon, j if its other symbol is not, q becomes the arc's source; once to count the arcs and add the reported weight,
// once to write the path.  The arc range, a step cap of (n + m + 1)(levels + 1) and the arrival are checked.
#include <hip/hip_runtime.h>
#include <limits>
#include <string>
#include <vector>
#include "decode_pairs_trellis.hpp"

namespace {
struct BestOut {
  const uint64_t* bp_off;  // [n + 1]: each pair's (n + 1)(m + 1)|Q| slots, slot (i (m + 1) + j) |Q| + q; preset to kNone
  uint32_t* bp;
  uint32_t* n_paths;  // [n]: 1 if the pair has a derivation
};

struct BestAcc {
  typedef BestOut Out;
  static constexpr bool kKeep = false;
  double v;
  uint32_t arc;
  __device__ __forceinline__ void init(bool start) {
    v = start ? 0.0 : -std::numeric_limits<double>::infinity();
    arc = kNone;
  }
  __device__ __forceinline__ void add(double x, uint32_t id) {
    if (x > v) {
      v = x;
      arc = id;
    }
  }
  __device__ __forceinline__ double store(const Out& O, uint32_t pair, size_t slot) const {
    if (arc != kNone) O.bp[O.bp_off[pair] + slot] = arc;
    return v;
  }
  static __device__ __forceinline__ void read_out(const Out& O, uint32_t pair, double f) {
    O.n_paths[pair] = f > -std::numeric_limits<double>::infinity();
  }
};

// one lane per pair.  kWrite = false counts the path's arcs into len[pair] and adds their weights from the end into logw[pair];
// kWrite = true writes the arcs in path order at path[path_off[pair] ..)
template <bool kWrite>
__global__ void pair_walk_kernel(uint32_t n_pairs, uint32_t n_states, uint32_t final_state, uint64_t n_arcs, uint32_t levels,
                                 const uint64_t* off, const uint64_t* off2, BestOut O, const uint32_t* a_src, const uint8_t* a_flags,
                                 const double* a_w, uint32_t* len, double* logw, const uint64_t* path_off, uint32_t* path, int* err) {
  const uint32_t pair = blockIdx.x * blockDim.x + threadIdx.x;
  if (pair >= n_pairs || !O.n_paths[pair]) return;
  uint32_t i = (uint32_t)(off[pair + 1] - off[pair]), j = (uint32_t)(off2[pair + 1] - off2[pair]), q = final_state;
  const uint32_t m = j;
  const uint32_t* bp = O.bp + O.bp_off[pair];
  const uint64_t cap = ((uint64_t)i + j + 1) * ((uint64_t)levels + 1);  // no path of the trellis is longer
  const uint32_t n_path = kWrite ? len[pair] : 0;
  uint32_t steps = 0;
  double w = 0.0;
  while (true) {
    const uint32_t a = bp[((size_t)i * (m + 1) + j) * n_states + q];
    if (a == kNone) break;
    if (a >= n_arcs || steps >= cap || (kWrite && steps >= n_path)) {
      atomicOr(err, kErrWalk);
      return;
    }
    const uint32_t f = a_flags[a];
    if (((f & 1) && i == 0) || ((f & 2) && j == 0)) {
      atomicOr(err, kErrWalk);
      return;
    }
    ++steps;
    if (kWrite) path[path_off[pair] + n_path - steps] = a;
    w = a_w[a] + w;
    q = a_src[a];
    if (f & 1) --i;
    if (f & 2) --j;
  }
  if (i != 0 || j != 0 || q != 0 || (kWrite && steps != n_path)) atomicOr(err, kErrWalk);
  if (!kWrite) {
    len[pair] = steps;
    logw[pair] = w;
  }
}

}  // namespace

extern "C" {

int carmel_hip_decode_pairs(carmel_hip_decoder* d, uint64_t n_pairs, const uint64_t* off, const uint32_t* sym, const uint64_t* off2,
                            const uint32_t* sym2, double* best_logw, uint64_t* path_off) {
  const char* who = "carmel_hip_decode_pairs";
  PairCall call{d, n_pairs, off, off2};
  if (const int rc = call.check(who, sym, sym2, (best_logw && path_off) ? best_logw : nullptr)) return rc;
  const std::string bad = std::string(who) + ": inconsistent back-pointers";
  const uint32_t Q = d->n_states;
  HIPCHK(hipSetDevice(d->device));
  d->paths.clear();
  std::vector<uint64_t> line_paths(n_pairs + 1, 0), p_off(1, 0);
  std::vector<double> p_logw;
  DevBuf<uint64_t> d_bpoff, d_poff, d_rows_off;
  DevBuf<uint32_t> d_bp, d_np, d_len, d_path;
  DevBuf<double> d_logw, d_rows;
  DevBuf<int> d_err;
  HIPCHK(d_err.alloc(1));
  // a pair costs its back-pointers, its symbols and, in the global tier, its three diagonals
  auto cost = [&](uint64_t l) {
    return 4 * call.nodes(l) + 4 * (call.len1(l) + call.len2(l)) + (call.lds ? 0 : 24 * call.diag_doubles(l));
  };
  const int rc = decode_chunks_by_cost(d, n_pairs, off, sym, off2, sym2, call.lds, cost, 1u << 24, [&](DecodeChunk& c) {
    hipStream_t s = d->stream;
    const uint32_t n = c.n;
    std::vector<uint64_t> h_bpoff(n + 1, 0);
    for (uint32_t l = 0; l < n; ++l) h_bpoff[l + 1] = h_bpoff[l] + call.nodes(c.lo + l);
    HIPCHK(d_bpoff.upload(h_bpoff, s));
    HIPCHK(d_bp.alloc(h_bpoff[n]));
    HIPCHK(d_np.alloc(n));
    HIPCHK(d_len.alloc(n));
    HIPCHK(d_logw.alloc(n));
    PairLines L;
    if (const int r = call.rows(c, d_rows, d_rows_off, L)) return r;
    HIPCHK(hipMemsetAsync(d_err.p, 0, sizeof(int), s));
    const BestOut O{d_bpoff.p, d_bp.p, d_np.p};
    const uint32_t wb = (n + 255) / 256;
    auto walk = [&](bool write) {
      (write ? pair_walk_kernel<true> : pair_walk_kernel<false>)<<<wb, 256, 0, s>>>(
          n, Q, d->final_state, d->n_arcs, d->pair_levels, L.off, L.off2, O, d->a_src.p, d->a_flags.p, d->a_w.p, d_len.p, d_logw.p,
          d_poff.p, d_path.p, d_err.p);
    };
    if (const int r = c.begin()) return r;
    HIPCHK(hipMemsetAsync(d_bp.p, 0xff, h_bpoff[n] * sizeof(uint32_t), s));  // every slot kNone
    launch_pairs<BestAcc>(d, call.lds, call.lds_bytes, n, L, O, s);
    walk(false);
    if (const int r = c.end()) return r;
    std::vector<uint32_t> np(n), len(n);
    std::vector<double> lw(n);
    int err = 0;
    HIPCHK(hipMemcpyAsync(np.data(), d_np.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(len.data(), d_len.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(lw.data(), d_logw.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    if (const int r = c.wait()) return r;
    if (err) return fail(CARMEL_HIP_ERR_STATE, bad);
    for (uint32_t l = 0; l < n; ++l)
      if (np[l] > 1) return fail(CARMEL_HIP_ERR_STATE, bad);
    const uint64_t base = d->paths.size();
    const std::vector<uint64_t> h_poff = decode_collect_paths(c, 1, np, len, lw, base, line_paths.data(), p_logw, p_off);
    if (!h_poff[n]) return CARMEL_HIP_OK;
    HIPCHK(d_poff.upload(h_poff, s));
    HIPCHK(d_path.alloc(h_poff[n]));
    if (const int r = c.begin()) return r;
    walk(true);
    if (const int r = c.end()) return r;
    d->paths.resize(base + h_poff[n]);
    HIPCHK(hipMemcpyAsync(d->paths.data() + base, d_path.p, h_poff[n] * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    if (const int r = c.wait()) return r;
    return err ? fail(CARMEL_HIP_ERR_STATE, bad) : CARMEL_HIP_OK;
  });
  if (rc) return rc;
  path_off[0] = 0;
  for (uint64_t l = 0; l < n_pairs; ++l) {  // a pair has one path or none
    const uint64_t p = line_paths[l];
    best_logw[l] = line_paths[l + 1] > p ? p_logw[p] : -std::numeric_limits<double>::infinity();
    path_off[l + 1] = p_off[line_paths[l + 1]];
  }
  return CARMEL_HIP_OK;
}

int carmel_hip_decode_pairs_sum(carmel_hip_decoder* d, uint64_t n_pairs, const uint64_t* off, const uint32_t* sym,
                                const uint64_t* off2, const uint32_t* sym2, double* sum_logw) {
  PairCall call{d, n_pairs, off, off2};
  if (const int rc = call.check("carmel_hip_decode_pairs_sum", sym, sym2, sum_logw)) return rc;
  DevBuf<double> d_sum, d_rows;
  DevBuf<uint64_t> d_rows_off;
  // there are no back-pointers to hold: a pair costs its symbols (and its global-tier diagonals)
  auto cost = [&](uint64_t l) { return 4 * (call.len1(l) + call.len2(l)) + (call.lds ? 0 : 24 * call.diag_doubles(l)); };
  return decode_chunks_by_cost(d, n_pairs, off, sym, off2, sym2, call.lds, cost, 1u << 24, [&](DecodeChunk& c) {
    HIPCHK(d_sum.alloc(c.n));
    PairLines L;
    if (const int r = call.rows(c, d_rows, d_rows_off, L)) return r;
    if (const int r = c.begin()) return r;
    launch_pairs<SumAcc>(d, call.lds, call.lds_bytes, c.n, L, SumOut{d_sum.p}, d->stream);
    if (const int r = c.end()) return r;
    HIPCHK(hipMemcpyAsync(sum_logw + c.lo, d_sum.p, c.n * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    return c.wait();
  });
}

}  // extern "C"
