// consolidate.hip — merging duplicate arcs on the GPU (carmel -C; carmel_hip_consolidate).  Free-standing like compose.hip: no
// decoder handle, because the front end consolidates before it pays for a decoder's tables.
//
// Replaces WFST::consolidateArcs (fst.cc:526-528) and State::reduce (state.h:248-278), called from carmel_main::minimize
// (carmel.cc:638-642), with --consolidate-max and --consolidate-unclamped (carmel.cc:1752-1753).  The rule, in the words of
// include/carmel_hip.h (tests/consolidate_ref.py restates it in Python):
// Inputs.  n_arcs arcs in arc-id order with src non-decreasing, as Wfst and Transducer::flatten give them; per arc src, dst,
//   in_sym, out_sym as u32, any value up to 0xfffffffe, and logw; mode 0 = sum, 1 = max; clamp 0 or 1, read in sum mode only.
// Existence.  An arc exists iff logw > -inf.  A NaN or +inf weight, src not non-decreasing, or n_arcs >= 0xffffffff is
//   CARMEL_HIP_ERR_ARG, and nothing is written.
// Segment.  All existing arcs with equal (src, dst, in_sym, out_sym), all four fields, full 32 bits each.  Tie groups play no
//   part (the reference's UnArc has none either).
// Representative.  The member with the lowest arc id (the reference keeps the first arc in list order and erases the later ones).
// Weight of a segment.  A segment of one member keeps that member's weight bit for bit, in every mode.  Max mode: the largest
//   member weight, a copy of a member's bits.  Sum mode: ln sum exp(w_i) with sweep_math.hpp's Lse, in the fixed order below.
//   With clamp, a result > 0.0 becomes 0.0 (the reference clamps after every add; for non-negative terms that is one clamp at
//   the end).
// Result.  n_kept is the number of segments; new arc j is the segment with the j-th smallest representative id, so the result
//   is still state-major with each state's survivors in first-occurrence order; kept_id[j] is that representative's old arc id,
//   kept_logw[j] the segment's weight, arc_map[a] the new index of arc a's segment or 0xffffffff for an arc that does not exist.
//   Entries of kept_id and kept_logw from n_kept on are not written.
// Deviations from the reference: the total order above replaces hash-table iteration side effects.  There are no others.
//
// Passes (no float atomics anywhere: a call returns the same bytes every time; no kernel uses scratch memory,
// tests/test_consolidate_host.py):
//  1. Key.  src is sorted already and dst / in_sym / out_sym rarely need 32 bits each: with bs, bd, bi, bo the bits of the
//     call's maxima, an arc's key is src << (bd + bi + bo) | dst << (bi + bo) | in << bo | out when bs + bd + bi + bo <= 63 --
//     lossless, every field has its own bits -- and an arc that does not exist gets bit bs + bd + bi + bo alone, which sorts
//     last; one stable hipcub::DeviceRadixSort::SortPairs of (key, arc id) over exactly those bits.  Otherwise two stable passes
//     least significant first over unpacked keys: (in << 32 | out), then (src << 32 | dst) with all ones for an arc that does
//     not exist (src is at most 0xfffffffe).  Stability leaves the ids ascending within a key.  The host knows how many arcs
//     exist; the sorted tail behind them is cut off.
//  2. Heads.  A sorted arc is a head when its key differs from its left neighbour's (the packed keys are compared, or in the
//     two-pass form the four fields); an inclusive scan of the flags, less one, numbers the segments, and the heads write their
//     segment's first position.  A head also flags its arc id as a representative.
//  3. Reduce.  A lane per segment of at most `consolidate_wave_members` members (option, default 64): the members in id order
//     through one Lse.  A wavefront per larger segment: lane l folds members l, l + 64, ... in id order through its own Lse,
//     then six shuffle steps (distance 32, 16, 8, 4, 2, 1) combine the (m, acc) pairs, lane k taking lane k + distance's:
//     (m, acc) <- (max, acc_hi + acc_lo * exp(m_lo - m_hi)).  Max mode is the same walk with a compare.  The two forms need not
//     agree bit for bit in sum mode; each is a fixed order.
//  4. Compact.  An exclusive scan of the representative flags over the old arc ids gives every representative its new index;
//     one pass over the sorted arcs writes arc_map, and the heads kept_id and kept_logw, with plain vector stores.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "engine.hpp"
#include "sweep_math.hpp"

namespace {

constexpr uint32_t kNoArc = 0xffffffffu;
constexpr uint32_t kWaveMembers = 64;  // option consolidate_wave_members
constexpr int kLanes = 64;

struct ConsArcs {  // the call's arcs on the device
  uint64_t n;
  const uint32_t *src, *dst, *in, *out;
  const double* logw;
};

__device__ __forceinline__ uint64_t cons_index() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }

// pass 1, packed form: every field in its own bits; `dead` is the one bit above them
__global__ void __launch_bounds__(256) consolidate_key_kernel(ConsArcs A, uint32_t sh_src, uint32_t sh_dst, uint32_t sh_in, uint64_t dead,
                                                              uint64_t* key, uint32_t* id) {
  const uint64_t i = cons_index();
  if (i >= A.n) return;
  const uint64_t k = ((uint64_t)A.src[i] << sh_src) | ((uint64_t)A.dst[i] << sh_dst) | ((uint64_t)A.in[i] << sh_in) | (uint64_t)A.out[i];
  key[i] = A.logw[i] > NEG_INF ? k : dead;
  id[i] = (uint32_t)i;
}

// pass 1, two-pass form: the low key of every arc in arc-id order ...
__global__ void __launch_bounds__(256) consolidate_key_lo_kernel(ConsArcs A, uint64_t* key, uint32_t* id) {
  const uint64_t i = cons_index();
  if (i >= A.n) return;
  key[i] = ((uint64_t)A.in[i] << 32) | (uint64_t)A.out[i];
  id[i] = (uint32_t)i;
}

// ... and the high key in the order the first sort left
__global__ void __launch_bounds__(256) consolidate_key_hi_kernel(ConsArcs A, const uint32_t* id, uint64_t* key) {
  const uint64_t i = cons_index();
  if (i >= A.n) return;
  const uint32_t a = id[i];
  key[i] = A.logw[a] > NEG_INF ? (((uint64_t)A.src[a] << 32) | (uint64_t)A.dst[a]) : ~0ull;
}

// pass 2: head flags over the n_live sorted arcs that exist, and the representatives' flags over the arc ids
template <bool kPacked>
__global__ void __launch_bounds__(256) consolidate_heads_kernel(ConsArcs A, uint64_t n_live, const uint64_t* key, const uint32_t* id,
                                                                uint32_t* flag, uint32_t* rep_flag) {
  const uint64_t i = cons_index();
  if (i >= n_live) return;
  const uint32_t a = id[i];
  bool head = i == 0;
  if (!head) {
    if (kPacked)
      head = key[i] != key[i - 1];
    else {
      const uint32_t b = id[i - 1];
      head = A.src[a] != A.src[b] || A.dst[a] != A.dst[b] || A.in[a] != A.in[b] || A.out[a] != A.out[b];
    }
  }
  flag[i] = head ? 1u : 0u;
  if (head) rep_flag[a] = 1u;
}

// the heads write their segment's first sorted position; the last sorted arc the number of segments and the end of the last one
__global__ void __launch_bounds__(256) consolidate_extent_kernel(uint64_t n_live, const uint32_t* flag, const uint32_t* seg, uint32_t* seg_start,
                                                                 uint32_t* counts) {
  const uint64_t i = cons_index();
  if (i >= n_live) return;
  if (flag[i]) seg_start[seg[i] - 1] = (uint32_t)i;  // (seg: the inclusive scan, so a segment's number plus one)
  if (i == n_live - 1) {
    const uint32_t n_seg = seg[i];
    seg_start[n_seg] = (uint32_t)n_live;
    counts[0] = n_seg;
  }
}

__device__ __forceinline__ double cons_finish(const carmel_hip::Lse& L, int clamp) {
  const double v = L.value();
  return clamp && v > 0.0 ? 0.0 : v;
}

// pass 3, lane form: a lane per segment; a segment of more than wave_members members goes on the wavefronts' list (counts[1])
__global__ void __launch_bounds__(256) consolidate_reduce_lane_kernel(const double* logw, const uint32_t* id, const uint32_t* seg_start,
                                                                      uint32_t* counts, uint32_t wave_members, int mode, int clamp,
                                                                      double* seg_w, uint32_t* big) {
  const uint64_t s = cons_index();
  if (s >= counts[0]) return;
  const uint32_t b = seg_start[s], e = seg_start[s + 1];
  if (e - b > wave_members) {
    big[atomicAdd(&counts[1], 1u)] = (uint32_t)s;  // (the list's order plays no part in any segment's weight)
    return;
  }
  if (e - b == 1) {
    seg_w[s] = logw[id[b]];
    return;
  }
  if (mode) {
    double best = logw[id[b]];
    for (uint32_t k = b + 1; k < e; ++k) {
      const double x = logw[id[k]];
      if (x > best) best = x;
    }
    seg_w[s] = best;
    return;
  }
  carmel_hip::Lse L;
  L.init();
  for (uint32_t k = b; k < e; ++k) L.add(logw[id[k]]);
  seg_w[s] = cons_finish(L, clamp);
}

// pass 3, wavefront form: the wavefronts share the list of large segments
__global__ void __launch_bounds__(256) consolidate_reduce_wave_kernel(const double* logw, const uint32_t* id, const uint32_t* seg_start,
                                                                      const uint32_t* counts, const uint32_t* big, int mode, int clamp,
                                                                      double* seg_w) {
  const uint32_t lane = threadIdx.x & (kLanes - 1);
  const uint32_t waves = gridDim.x * (blockDim.x / kLanes);
  const uint32_t n_big = counts[1];
  for (uint32_t k = blockIdx.x * (blockDim.x / kLanes) + threadIdx.x / kLanes; k < n_big; k += waves) {
    const uint32_t s = big[k];
    const uint32_t b = seg_start[s], e = seg_start[s + 1];
    if (mode) {
      double best = NEG_INF;
      for (uint32_t p = b + lane; p < e; p += kLanes) {
        const double x = logw[id[p]];
        if (x > best) best = x;
      }
      for (int d = kLanes / 2; d; d >>= 1) {
        const double other = __shfl_down(best, d, kLanes);
        if (other > best) best = other;
      }
      if (lane == 0) seg_w[s] = best;
      continue;
    }
    carmel_hip::Lse L;
    L.init();
    for (uint32_t p = b + lane; p < e; p += kLanes) L.add(logw[id[p]]);
    for (int d = kLanes / 2; d; d >>= 1) {
      const double om = __shfl_down(L.m, d, kLanes), oacc = __shfl_down(L.acc, d, kLanes);
      if (om == NEG_INF) {  // (a lane without members adds nothing)
      } else if (L.m == NEG_INF) {
        L.m = om;
        L.acc = oacc;
      } else if (om <= L.m)
        L.acc = L.acc + oacc * K_EXP(om - L.m);
      else {
        L.acc = oacc + L.acc * K_EXP(L.m - om);
        L.m = om;
      }
    }
    if (lane == 0) seg_w[s] = e - b == 1 ? L.m : cons_finish(L, clamp);
  }
}

// pass 4: every sorted arc that exists learns its segment's new index; the heads write the segment's row
__global__ void __launch_bounds__(256) consolidate_write_kernel(uint64_t n_live, const uint32_t* id, const uint32_t* seg, const uint32_t* seg_start,
                                                                const uint32_t* new_index, const double* seg_w, uint32_t* arc_map,
                                                                uint32_t* kept_id, double* kept_logw) {
  const uint64_t i = cons_index();
  if (i >= n_live) return;
  const uint32_t s = seg[i] - 1;
  const uint32_t b = seg_start[s];
  const uint32_t rep = id[b];
  const uint32_t j = new_index[rep];
  arc_map[id[i]] = j;
  if (i == b) {
    kept_id[j] = rep;
    kept_logw[j] = seg_w[s];
  }
}

uint32_t bits_of(uint32_t x) {
  uint32_t b = 0;
  while (x) {
    ++b;
    x >>= 1;
  }
  return b;
}

struct ConsStream {  // the call's stream and events
  hipStream_t s = nullptr;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  ~ConsStream() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
    if (s) (void)hipStreamDestroy(s);
  }
};

}  // namespace

extern "C" {

int carmel_hip_consolidate(int device, uint64_t n_arcs, const uint32_t* src, const uint32_t* dst, const uint32_t* in_sym,
                           const uint32_t* out_sym, const double* logw, int mode, int clamp, uint32_t* arc_map, uint32_t* kept_id,
                           double* kept_logw, uint64_t* n_kept, double* kernel_ms) {
  const std::string who = "carmel_hip_consolidate";
  if (!n_kept || (n_arcs && (!src || !dst || !in_sym || !out_sym || !logw || !arc_map || !kept_id || !kept_logw)))
    return fail(CARMEL_HIP_ERR_ARG, who + ": null argument");
  if ((mode != 0 && mode != 1) || (clamp != 0 && clamp != 1)) return fail(CARMEL_HIP_ERR_ARG, who + ": mode and clamp must be 0 or 1");
  if (n_arcs >= 0xffffffffull) return fail(CARMEL_HIP_ERR_ARG, who + ": arcs must be below 2^32 - 1");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(CARMEL_HIP_ERR_HIP, who + ": no HIP device: consolidation has no CPU fallback");
  // the inputs are checked before anything is written; the same walk finds the fields' maxima and counts the arcs that exist
  uint32_t max_dst = 0, max_in = 0, max_out = 0;
  uint64_t n_live = 0;
  for (uint64_t a = 0; a < n_arcs; ++a) {
    const double w = logw[a];
    if (std::isnan(w) || w == HUGE_VAL)
      return fail(CARMEL_HIP_ERR_ARG, who + ": arc " + std::to_string(a) + " has a weight that is not a number or is infinite");
    if (a && src[a] < src[a - 1]) return fail(CARMEL_HIP_ERR_ARG, who + ": arc " + std::to_string(a) + ": src must be non-decreasing");
    if (src[a] == kNoArc || dst[a] == kNoArc || in_sym[a] == kNoArc || out_sym[a] == kNoArc)
      return fail(CARMEL_HIP_ERR_ARG, who + ": arc " + std::to_string(a) + ": states and symbols must be at most 0xfffffffe");
    max_dst = std::max(max_dst, dst[a]);
    max_in = std::max(max_in, in_sym[a]);
    max_out = std::max(max_out, out_sym[a]);
    n_live += w > -HUGE_VAL;
  }
  if (kernel_ms) *kernel_ms = 0.0;
  if (!n_live) {
    if (n_arcs) std::memset(arc_map, 0xff, n_arcs * sizeof(uint32_t));
    *n_kept = 0;
    return CARMEL_HIP_OK;
  }
  HIPCHK(hipSetDevice(device));
  uint32_t wave_members = kWaveMembers;
  if (const char* v = lib_opt("consolidate_wave_members"))
    wave_members = (uint32_t)std::min<unsigned long long>(std::strtoull(v, nullptr, 10), 0xffffffffull);
  const uint32_t bs = bits_of(src[n_arcs - 1]), bd = bits_of(max_dst), bi = bits_of(max_in), bo = bits_of(max_out);
  const uint32_t key_bits = bs + bd + bi + bo;
  const bool packed = key_bits <= 63;

  ConsStream S;
  HIPCHK(hipStreamCreate(&S.s));
  for (hipEvent_t& e : S.ev) HIPCHK(hipEventCreate(&e));
  hipStream_t s = S.s;
  DevBuf<uint32_t> d_src, d_dst, d_in, d_out, id, flag, seg, seg_start, rep_flag, new_index, counts, big, d_arc_map, d_kept_id;
  DevBuf<double> d_logw, seg_w, d_kept_logw;
  DevBuf<uint64_t> key;
  DevBuf<uint8_t> tmp;
  HIPCHK(d_src.alloc(n_arcs));
  HIPCHK(d_dst.alloc(n_arcs));
  HIPCHK(d_in.alloc(n_arcs));
  HIPCHK(d_out.alloc(n_arcs));
  HIPCHK(d_logw.alloc(n_arcs));
  HIPCHK(key.alloc(2 * n_arcs));
  HIPCHK(id.alloc(2 * n_arcs));
  HIPCHK(flag.alloc(n_live));
  HIPCHK(seg.alloc(n_live));
  HIPCHK(seg_start.alloc(n_live + 1));
  HIPCHK(rep_flag.alloc(n_arcs));
  HIPCHK(new_index.alloc(n_arcs));
  HIPCHK(counts.alloc(2));
  HIPCHK(big.alloc(n_live));
  HIPCHK(seg_w.alloc(n_live));
  HIPCHK(d_arc_map.alloc(n_arcs));
  HIPCHK(d_kept_id.alloc(n_live));
  HIPCHK(d_kept_logw.alloc(n_live));
  size_t sort_bytes = 0, scan_live_bytes = 0, scan_arcs_bytes = 0;
  HIPCHK(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, key.p, key.p + n_arcs, id.p, id.p + n_arcs, n_arcs, 0, 64, s));
  HIPCHK(hipcub::DeviceScan::InclusiveSum(nullptr, scan_live_bytes, flag.p, seg.p, n_live, s));
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_arcs_bytes, rep_flag.p, new_index.p, n_arcs, s));
  size_t tmp_bytes = std::max<size_t>(std::max(sort_bytes, std::max(scan_live_bytes, scan_arcs_bytes)), 1);
  HIPCHK(tmp.alloc(tmp_bytes));
  const size_t u32s = n_arcs * sizeof(uint32_t);
  HIPCHK(hipMemcpyAsync(d_src.p, src, u32s, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_dst.p, dst, u32s, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_in.p, in_sym, u32s, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_out.p, out_sym, u32s, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d_logw.p, logw, n_arcs * sizeof(double), hipMemcpyHostToDevice, s));

  const ConsArcs A{n_arcs, d_src.p, d_dst.p, d_in.p, d_out.p, d_logw.p};
  const uint32_t arc_blocks = (uint32_t)((n_arcs + 255) / 256), live_blocks = (uint32_t)((n_live + 255) / 256);
  uint64_t* key_a = key.p;
  uint64_t* key_b = key.p + n_arcs;
  uint32_t* id_a = id.p;
  uint32_t* id_b = id.p + n_arcs;
  const uint32_t* sorted_id = nullptr;
  HIPCHK(hipEventRecord(S.ev[0], s));
  // 1. keys and the stable sort
  if (packed) {
    consolidate_key_kernel<<<arc_blocks, 256, 0, s>>>(A, bd + bi + bo, bi + bo, bo, 1ull << key_bits, key_a, id_a);
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, key_a, key_b, id_a, id_b, n_arcs, 0, (int)key_bits + 1, s));
    sorted_id = id_b;
  } else {
    consolidate_key_lo_kernel<<<arc_blocks, 256, 0, s>>>(A, key_a, id_a);
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, key_a, key_b, id_a, id_b, n_arcs, 0, 64, s));
    consolidate_key_hi_kernel<<<arc_blocks, 256, 0, s>>>(A, id_b, key_b);
    HIPCHK(hipcub::DeviceRadixSort::SortPairs(tmp.p, tmp_bytes, key_b, key_a, id_b, id_a, n_arcs, 0, 64, s));
    sorted_id = id_a;
  }
  HIPCHK(hipEventRecord(S.ev[1], s));
  // 2. heads, segment numbers, extents
  HIPCHK(hipMemsetAsync(rep_flag.p, 0, u32s, s));
  HIPCHK(hipMemsetAsync(counts.p, 0, 2 * sizeof(uint32_t), s));
  if (packed)
    consolidate_heads_kernel<true><<<live_blocks, 256, 0, s>>>(A, n_live, key_b, sorted_id, flag.p, rep_flag.p);
  else
    consolidate_heads_kernel<false><<<live_blocks, 256, 0, s>>>(A, n_live, nullptr, sorted_id, flag.p, rep_flag.p);
  HIPCHK(hipcub::DeviceScan::InclusiveSum(tmp.p, tmp_bytes, flag.p, seg.p, n_live, s));
  consolidate_extent_kernel<<<live_blocks, 256, 0, s>>>(n_live, flag.p, seg.p, seg_start.p, counts.p);
  HIPCHK(hipEventRecord(S.ev[2], s));
  // 3. the segments' weights
  consolidate_reduce_lane_kernel<<<live_blocks, 256, 0, s>>>(d_logw.p, sorted_id, seg_start.p, counts.p, wave_members, mode, clamp, seg_w.p, big.p);
  consolidate_reduce_wave_kernel<<<(uint32_t)std::min<uint64_t>((n_live + 3) / 4, 4096), 256, 0, s>>>(d_logw.p, sorted_id, seg_start.p, counts.p, big.p,
                                                                                                    mode, clamp, seg_w.p);
  HIPCHK(hipEventRecord(S.ev[3], s));
  // 4. the new order and the outputs
  HIPCHK(hipcub::DeviceScan::ExclusiveSum(tmp.p, tmp_bytes, rep_flag.p, new_index.p, n_arcs, s));
  HIPCHK(hipMemsetAsync(d_arc_map.p, 0xff, u32s, s));
  consolidate_write_kernel<<<live_blocks, 256, 0, s>>>(n_live, sorted_id, seg.p, seg_start.p, new_index.p, seg_w.p, d_arc_map.p, d_kept_id.p,
                                                       d_kept_logw.p);
  HIPCHK(hipEventRecord(S.ev[4], s));
  HIPCHK(hipGetLastError());
  uint32_t h_counts[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(h_counts, counts.p, sizeof h_counts, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const uint64_t kept = h_counts[0];
  if (!kept || kept > n_live) return fail(CARMEL_HIP_ERR_STATE, who + ": inconsistent segment count");
  // (the caller's buffers are written last, and only by a call that succeeds so far: through buffers of the library's own)
  std::vector<uint32_t> h_map(n_arcs), h_id(kept);
  std::vector<double> h_w(kept);
  HIPCHK(hipMemcpyAsync(h_map.data(), d_arc_map.p, u32s, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h_id.data(), d_kept_id.p, kept * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h_w.data(), d_kept_logw.p, kept * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  float ms[4] = {0, 0, 0, 0};
  for (int k = 0; k < 4; ++k) HIPCHK(hipEventElapsedTime(&ms[k], S.ev[k], S.ev[k + 1]));
  std::memcpy(arc_map, h_map.data(), u32s);
  std::memcpy(kept_id, h_id.data(), kept * sizeof(uint32_t));
  std::memcpy(kept_logw, h_w.data(), kept * sizeof(double));
  *n_kept = kept;
  if (kernel_ms) *kernel_ms = (double)ms[0] + ms[1] + ms[2] + ms[3];
  if (lib_opt("timing") && std::atoi(lib_opt("timing")))
    fprintf(stderr, "timing: consolidate passes %s key+sort %.3f ms, heads %.3f ms, reduce %.3f ms (%u by wavefronts), compact %.3f ms\n",
            packed ? "packed" : "two-pass", ms[0], ms[1], ms[2], h_counts[1], ms[3]);
  return CARMEL_HIP_OK;
}

}  // extern "C"
