// decode_paths.hip — what the batch decoders' entry points run on (declared in decode.hpp): the chunk driver of all of them
// (carmel_hip_decode, carmel_hip_decode_kbest, carmel_hip_decode_sum, carmel_hip_decode_sample, carmel_hip_decode_posterior by a
// line's length; carmel_hip_decode_pairs, carmel_hip_decode_pairs_sum, carmel_hip_decode_pairs_posterior and
// carmel_hip_decode_pairs_sample and carmel_hip_decode_pairs_kbest by a pair's cost), for
// the two that return the
// paths of a path-recording trellis the walk kernel and the path driver around it, and the assembly of a chunk's paths that the
// samplers (decode_sample.hip and decode_pairs_sample.hip, walks of their own) and the pairs' k-best (decode_pairs_kbest.hip, a
// ranked pair walk of its own) share with that driver.
//
// The walk: a path-recording trellis leaves, per (position i, state q, rank r), the arc that enters the slot's path last and the
// rank of that arc's source (DecodePaths).  One lane per (line, rank j) follows them from (n, final, j) to (0, start, 0), once to
// count the path's arcs and add their weights from the END, w1 + (w2 + (... + (wn + 0))) -- the weight reported (decode.hip's
// header) -- and once to write the arcs in path order.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <numeric>
#include <string>
#include <vector>
#include "decode.hpp"
#include "engine.hpp"

namespace {
// one lane per (line, rank j): slot line * K + j, idle if j >= n_paths[line].  kWrite = false counts the path's arcs into
// len[slot] and adds their weights from the end into logw[slot]; kWrite = true writes the arcs in path order at
// path[path_off[slot] ..).  bp_rank == nullptr: every rank is 0 (K = 1)
template <bool kWrite>
__global__ void decode_walk_kernel(uint32_t n_lines, uint32_t n_states, uint32_t K, uint32_t final_state, uint64_t n_arcs,
                                   const uint64_t* off, const uint64_t* bp_off, const uint32_t* bp_arc, const uint16_t* bp_rank,
                                   const uint32_t* n_paths, const uint32_t* a_src, const uint8_t* a_eps, const double* a_w,
                                   uint32_t* len, double* logw, const uint64_t* path_off, uint32_t* path, int* err) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;  // (a chunk has at most 2^24 slots: the path driver's cap)
  if (slot >= n_lines * K) return;
  const uint32_t line = slot / K;
  uint32_t r = slot % K;
  if (r >= n_paths[line]) return;
  uint32_t i = (uint32_t)(off[line + 1] - off[line]), q = final_state;
  const uint32_t* ba = bp_arc + bp_off[line];
  const uint16_t* br = bp_rank ? bp_rank + bp_off[line] : nullptr;
  const uint64_t cap = (uint64_t)(i + 1) * n_states;  // no path of the trellis is longer
  const uint32_t n_path = kWrite ? len[slot] : 0;
  uint32_t steps = 0;
  double w = 0.0;
  while (true) {
    const size_t at = ((size_t)i * n_states + q) * K + r;
    const uint32_t a = ba[at];
    if (a == kNone) break;
    const uint32_t rs = br ? br[at] : 0;
    if (a >= n_arcs || steps >= cap || (kWrite && steps >= n_path) || (!a_eps[a] && i == 0) || rs >= K) {
      atomicOr(err, kErrWalk);
      return;
    }
    ++steps;
    if (kWrite) path[path_off[slot] + n_path - steps] = a;
    w = a_w[a] + w;
    q = a_src[a];
    r = rs;
    if (!a_eps[a]) --i;
  }
  if (i != 0 || q != 0 || r != 0) atomicOr(err, kErrWalk);
  if (!kWrite) {
    len[slot] = steps;
    logw[slot] = w;
  }
}
}  // namespace

namespace carmel_hip {
int DecodeChunk::begin() {
  HIPCHK(hipEventRecord(d->ev0, d->stream));
  return CARMEL_HIP_OK;
}

int DecodeChunk::end() {
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(d->ev1, d->stream));
  return CARMEL_HIP_OK;
}

int DecodeChunk::wait() {
  HIPCHK(hipStreamSynchronize(d->stream));
  float t = 0;
  HIPCHK(hipEventElapsedTime(&t, d->ev0, d->ev1));
  ms += t;
  return CARMEL_HIP_OK;
}

int decode_check_lines(const char* who, uint64_t n_lines, const uint64_t* off) {
  for (uint64_t l = 0; l < n_lines; ++l)
    if (off[l + 1] < off[l] || off[l + 1] - off[l] >= kNone) return fail(CARMEL_HIP_ERR_ARG, std::string(who) + ": bad line offsets");
  return CARMEL_HIP_OK;
}

int decode_chunks_by_cost(carmel_hip_decoder* d, uint64_t n_lines, const uint64_t* off, const uint32_t* sym, const uint64_t* off2,
                          const uint32_t* sym2, bool lds, const std::function<uint64_t(uint64_t)>& cost, uint64_t cap,
                          const std::function<int(DecodeChunk&)>& body) {
  HIPCHK(hipSetDevice(d->device));
  hipStream_t s = d->stream;
  DecodeChunk c{d};
  c.lds = lds;
  c.ms = 0;
  uint64_t budget = 1ull << 30;
  if (const char* v = lib_opt("decode_chunk_bytes")) budget = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10));
  DevBuf<uint64_t> d_off, d_off2;
  DevBuf<uint32_t> d_sym, d_sym2, d_order;
  for (c.lo = 0; c.lo < n_lines; c.lo = c.hi) {
    uint64_t bytes = cost(c.lo);
    c.hi = c.lo + 1;
    while (c.hi < n_lines && c.hi - c.lo < cap && bytes + cost(c.hi) <= budget) bytes += cost(c.hi++);
    c.n = (uint32_t)(c.hi - c.lo);
    std::vector<uint64_t> h_off(c.n + 1), h_off2, h_cost(c.n);
    for (uint32_t l = 0; l <= c.n; ++l) h_off[l] = off[c.lo + l] - off[c.lo];
    for (uint32_t l = 0; l < c.n; ++l) h_cost[l] = cost(c.lo + l);
    std::vector<uint32_t> order(c.n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return h_cost[x] > h_cost[y]; });
    HIPCHK(d_off.upload(h_off, s));
    const std::vector<uint32_t> h_sym(sym + off[c.lo], sym + off[c.hi]);  // (named: the copy is asynchronous)
    HIPCHK(d_sym.upload(h_sym, s));
    HIPCHK(d_order.upload(order, s));
    std::vector<uint32_t> h_sym2;
    if (off2) {
      h_off2.resize(c.n + 1);
      for (uint32_t l = 0; l <= c.n; ++l) h_off2[l] = off2[c.lo + l] - off2[c.lo];
      h_sym2.assign(sym2 + off2[c.lo], sym2 + off2[c.hi]);
      HIPCHK(d_off2.upload(h_off2, s));
      HIPCHK(d_sym2.upload(h_sym2, s));
    }
    c.h_off = h_off.data();
    c.h_off2 = off2 ? h_off2.data() : nullptr;
    c.off2 = d_off2.p;
    c.sym2 = d_sym2.p;
    c.L = DecodeLines{d_off.p, d_sym.p, d_order.p, nullptr};
    if (const int rc = body(c)) return rc;
  }
  d->last_ms = c.ms;
  return CARMEL_HIP_OK;
}

int decode_chunks(carmel_hip_decoder* d, uint64_t n_lines, const uint64_t* off, const uint32_t* sym, uint64_t a, uint64_t b,
                  uint64_t cap, uint64_t row_doubles, const std::function<int(DecodeChunk&)>& body) {
  const bool lds = row_doubles <= kLdsStates && !lib_opt_off("decode_lds");
  DevBuf<double> d_rows;
  return decode_chunks_by_cost(
      d, n_lines, off, sym, nullptr, nullptr, lds,
      [&](uint64_t l) { return (off[l + 1] - off[l]) * a + b + (lds ? 0 : 16ull * row_doubles); }, cap, [&](DecodeChunk& c) {
        if (!lds) {
          HIPCHK(d_rows.alloc((size_t)c.n * 2 * row_doubles));
          c.L.rows = d_rows.p;
        }
        return body(c);
      });
}

std::vector<uint64_t> decode_collect_paths(const DecodeChunk& c, uint32_t K, const std::vector<uint32_t>& np,
                                           const std::vector<uint32_t>& len, const std::vector<double>& lw, uint64_t base,
                                           uint64_t* line_paths, std::vector<double>& logw, std::vector<uint64_t>& path_off) {
  const uint32_t n = c.n;
  // the slots of ranks a line does not have are empty paths: the arcs come back compact and in (line, rank) order
  std::vector<uint64_t> h_poff((uint64_t)n * K + 1, 0);
  for (uint32_t l = 0; l < n; ++l)
    for (uint32_t j = 0; j < K; ++j) {
      const uint64_t at = (uint64_t)l * K + j;
      h_poff[at + 1] = h_poff[at] + (j < np[l] ? len[at] : 0);
    }
  for (uint32_t l = 0; l < n; ++l) {
    for (uint32_t j = 0; j < np[l]; ++j) {
      const uint64_t at = (uint64_t)l * K + j;
      logw.push_back(lw[at]);
      path_off.push_back(base + h_poff[at + 1]);
    }
    line_paths[c.lo + l + 1] = line_paths[c.lo + l] + np[l];
  }
  return h_poff;
}

int decode_paths(carmel_hip_decoder* d, const char* who, uint32_t K, bool ranked, TrellisLaunch launch, uint64_t n_lines,
                 const uint64_t* off, const uint32_t* sym, uint64_t* line_paths, std::vector<double>& logw,
                 std::vector<uint64_t>& path_off, std::vector<uint32_t>& arcs) {
  const uint32_t Q = d->n_states;
  const uint64_t QK = (uint64_t)Q * K;
  const uint64_t slot_bytes = QK * (ranked ? 6 : 4);  // a (position, state, rank): the arc id, and the rank if there is one
  const std::string bad = std::string(who) + ": inconsistent back-pointers";
  HIPCHK(hipSetDevice(d->device));  // (d_err below is allocated before the chunk driver sets it)
  logw.clear();
  path_off.assign(1, 0);
  arcs.clear();
  line_paths[0] = 0;
  DevBuf<uint64_t> d_bpoff, d_poff;
  DevBuf<uint32_t> d_bparc, d_np, d_len, d_path;
  DevBuf<uint16_t> d_bprank;
  DevBuf<double> d_logw;
  DevBuf<int> d_err;
  HIPCHK(d_err.alloc(1));
  return decode_chunks(d, n_lines, off, sym, slot_bytes, slot_bytes, (1u << 24) / K, QK, [&](DecodeChunk& c) {
    hipStream_t s = d->stream;
    const uint32_t n = c.n;
    const uint64_t n_slots = (uint64_t)n * K;
    std::vector<uint64_t> h_bpoff(n + 1, 0);
    for (uint32_t l = 0; l < n; ++l) h_bpoff[l + 1] = h_bpoff[l] + (c.h_off[l + 1] - c.h_off[l] + 1) * QK;
    HIPCHK(d_bpoff.upload(h_bpoff, s));
    HIPCHK(d_bparc.alloc(h_bpoff[n]));
    if (ranked) HIPCHK(d_bprank.alloc(h_bpoff[n]));
    HIPCHK(d_np.alloc(n));
    HIPCHK(d_len.alloc(n_slots));
    HIPCHK(d_logw.alloc(n_slots));
    HIPCHK(hipMemsetAsync(d_err.p, 0, sizeof(int), s));
    const DecodePaths P{d_bpoff.p, d_bparc.p, d_bprank.p, d_np.p, d_err.p, K};
    const uint32_t wb = (uint32_t)((n_slots + 255) / 256);
    auto walk = [&](bool write) {
      (write ? decode_walk_kernel<true> : decode_walk_kernel<false>)<<<wb, 256, 0, s>>>(
          n, Q, K, d->final_state, d->n_arcs, c.L.off, P.bp_off, P.bp_arc, P.bp_rank, P.n_paths, d->a_src.p, d->a_eps.p, d->a_w.p,
          d_len.p, d_logw.p, d_poff.p, d_path.p, P.err);
    };
    if (const int rc = c.begin()) return rc;
    launch(d, c.lds, n, c.L, P, s);
    walk(false);
    if (const int rc = c.end()) return rc;
    std::vector<uint32_t> np(n), len(n_slots);
    std::vector<double> lw(n_slots);
    int err = 0;
    HIPCHK(hipMemcpyAsync(np.data(), d_np.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(len.data(), d_len.p, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(lw.data(), d_logw.p, n_slots * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    if (const int rc = c.wait()) return rc;
    if (err & kErrCycle)  // kbest.h:160-166
      return fail(CARMEL_HIP_ERR_UNSUPPORTED, "best_path_has_cycle: the best path has a cycle (an epsilon cycle of weight > 1)");
    if (err) return fail(CARMEL_HIP_ERR_STATE, bad);
    for (uint32_t l = 0; l < n; ++l)
      if (np[l] > K) return fail(CARMEL_HIP_ERR_STATE, bad);
    const uint64_t base = arcs.size();
    const std::vector<uint64_t> h_poff = decode_collect_paths(c, K, np, len, lw, base, line_paths, logw, path_off);
    if (!h_poff[n_slots]) return CARMEL_HIP_OK;
    HIPCHK(d_poff.upload(h_poff, s));
    HIPCHK(d_path.alloc(h_poff[n_slots]));
    if (const int rc = c.begin()) return rc;
    walk(true);
    if (const int rc = c.end()) return rc;
    arcs.resize(base + h_poff[n_slots]);
    HIPCHK(hipMemcpyAsync(arcs.data() + base, d_path.p, h_poff[n_slots] * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
    if (const int rc = c.wait()) return rc;
    return err ? fail(CARMEL_HIP_ERR_STATE, bad) : CARMEL_HIP_OK;
  });
}
}  // namespace carmel_hip
