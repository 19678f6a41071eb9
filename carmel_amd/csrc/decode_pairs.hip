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
// The walk: one lane per pair follows the back-pointers from (n, m, final) to (0, 0, start): i drops if the arc's matched symbol
// is not epsilon, j if its other symbol is not, q becomes the arc's source; once to count the arcs and add the reported weight,
// once to write the path.  The arc range, a step cap of (n + m + 1)(levels + 1) and the arrival are checked.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <limits>
#include <string>
#include <vector>
#include "decode.hpp"
#include "engine.hpp"
#include "sweep_math.hpp"

namespace {
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

struct BestOut {
  const uint64_t* bp_off;  // [n + 1]: each pair's (n + 1)(m + 1)|Q| slots, slot (i (m + 1) + j) |Q| + q; preset to kNone
  uint32_t* bp;
  uint32_t* n_paths;  // [n]: 1 if the pair has a derivation
};

struct SumOut {
  double* sum;  // [n]
};

struct BestAcc {
  typedef BestOut Out;
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

struct SumAcc {
  typedef SumOut Out;
  Lse a;
  __device__ __forceinline__ void init(bool start) {
    a.init();
    if (start) a.add(0.0);
  }
  __device__ __forceinline__ void add(double x, uint32_t) { a.add(x); }
  __device__ __forceinline__ double store(const Out&, uint32_t, size_t) const { return a.value(); }
  static __device__ __forceinline__ void read_out(const Out& O, uint32_t pair, double f) { O.sum[pair] = f; }
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
  }
  if (lane == 0) Acc::read_out(O, pair, base[(size_t)((n + m) % 3) * DQ + DQ - Q + T.final_state]);  // cell (n, m): the last of its diagonal
}

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
