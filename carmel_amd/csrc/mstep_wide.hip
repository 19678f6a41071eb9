// mstep_wide.hip -- the one-pass window M-step (mstep_window_kernel, kernels.hip: read its comments first) in batched form.
//
// The same results, bit for bit: per parameter the same operations in the same order (members added in ascending
// parameter order, v / sn or v * remain / sn, the library's log and exp, max |lin - exp(old)| as the bit pattern of a
// non-negative double).  What differs is how the memory system is used:
//   * a workgroup handles PIECES of 1024 consecutive parameters (+ one halo of 2 * span per piece, not one per 256) and
//     walks them with a grid of as many workgroups as the device holds at once (eight per CU), every global load of a piece
//     issued as one batch: 30 KB per workgroup in flight instead of 7.7;
//   * the counts (prior, snapshot weights) of a piece are fetched 16 bytes per lane, the codes 4 bytes per lane, and go
//     to LDS with equally wide writes; the per-parameter phase is strided by 256 so that it reads LDS without bank
//     conflicts and its own old weight and mask 8 and 4 bytes per lane;
//   * the step's result leaves from this launch: no mstep_max_final_kernel behind it (below: "the last workgroup").
#include <hip/hip_runtime.h>
#include "kernels.hpp"
#include "sweep_math.hpp"

#define WIDE_PIECE 1024
#define WIDE_HALO 64  // MSTEP_WINDOW_MAX: LDS slot of parameter k of a piece starting at k0 is k - k0 + WIDE_HALO, whatever the span

namespace carmel_hip {
namespace {
// what one thread fetches for one piece
template <bool NEED_LW, int MODE>
struct WideRegs {
  double2 c[2], p[2], l[2];  // counts / prior / snapshot weights of parameters k0 + 2 * (t + 256 h) and the next one
  uint32_t code[2];          // their two codes
  double hc, hp, hl;         // halo element of thread t < 2 * span
  uint16_t hcode;
  double old[4];             // own parameters k0 + t + 256 q: old weight and member masks
  uint32_t m32[4], l32[4];
  unsigned long long m64[4], l64[4];
};

template <bool FULL>
__device__ __forceinline__ double2 wide_ld2(const double* p, uint64_t k, uint64_t n) {
  double2 r = make_double2(0.0, 0.0);
  if (FULL || k + 1 < n)
    r = *reinterpret_cast<const double2*>(p + k);
  else if (k < n)
    r.x = p[k];
  return r;
}
// parameter of halo thread t: the span parameters before the piece, then the span behind it
__device__ __forceinline__ bool wide_halo(uint64_t k0, uint32_t span, uint64_t n, uint64_t& k, uint32_t& slot) {
  const uint32_t t = threadIdx.x;
  if (t >= 2 * span) return false;
  if (t < span) {
    slot = WIDE_HALO - span + t;
    if (k0 + t < span) return false;
    k = k0 + t - span;
  } else {
    slot = WIDE_HALO + WIDE_PIECE + (t - span);
    k = k0 + WIDE_PIECE + (t - span);
  }
  return k < n;
}

// every global load of the piece, issued as one batch.  FULL: the piece and its halo lie inside the table (all but the first
// and the last piece or two) -- no lane has anything to check
template <bool FULL, bool NEED_LW, int MODE>
__device__ __forceinline__ void wide_load_as(WideRegs<NEED_LW, MODE>& R, const MstepArgs& M, int use_counts, uint32_t span, uint64_t k0) {
  const uint32_t t = threadIdx.x;
  const bool prior = use_counts && M.prior;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint64_t k = k0 + 2 * (t + 256 * h);
    R.code[h] = 0xffffffffu;  // (no parameter: no norm group)
    if (FULL || k + 1 < M.n)
      R.code[h] = *reinterpret_cast<const uint32_t*>(M.code16 + k);
    else if (k < M.n)
      R.code[h] = 0xffff0000u | M.code16[k];
    R.c[h] = use_counts ? wide_ld2<FULL>(M.counts, k, M.n) : make_double2(0.0, 0.0);
    R.p[h] = prior ? wide_ld2<FULL>(M.prior, k, M.n) : make_double2(0.0, 0.0);
    if (NEED_LW) R.l[h] = wide_ld2<FULL>(M.lw_src, k, M.n);
  }
  uint64_t hk = 0;
  uint32_t slot;
  R.hcode = 0xffffu;
  R.hc = R.hp = R.hl = 0.0;
  if (wide_halo(k0, span, M.n, hk, slot)) {  // (FULL: every thread below 2 * span)
    R.hcode = M.code16[hk];
    if (use_counts) R.hc = M.counts[hk];
    if (prior) R.hp = M.prior[hk];
    if (NEED_LW) R.hl = M.lw_src[hk];
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const uint64_t k = k0 + t + 256 * q;
    const bool in = FULL || k < M.n;
    R.old[q] = in ? M.logw[k] : 0.0;
    if (MODE == 0) {
      R.m32[q] = in ? M.mask32[k] : 0u;
      if (NEED_LW) R.l32[q] = in ? M.lockmask32[k] : 0u;
    } else if (MODE == 1) {
      R.m64[q] = in ? M.mask64[k] : 0ull;
      if (NEED_LW) R.l64[q] = in ? M.lockmask64[k] : 0ull;
    }
  }
}

template <bool NEED_LW, int MODE>
__device__ __forceinline__ void wide_load(WideRegs<NEED_LW, MODE>& R, const MstepArgs& M, int use_counts, uint32_t span, uint64_t k0) {
  if (k0 >= span && k0 + WIDE_PIECE + span <= M.n)  // (uniform)
    wide_load_as<true>(R, M, use_counts, span, k0);
  else
    wide_load_as<false>(R, M, use_counts, span, k0);
}

// mstep_value of a staged parameter (mstep_window_kernel's, expression for expression)
template <bool NEED_LW>
__device__ __forceinline__ double wide_value(const MstepArgs& M, int use_counts, uint16_t code, double cv, double pv, double lw, uint64_t k,
                                             uint16_t& g) {
  double v = 0.0;
  g = 0xffffu;
  if (code != 0xffffu) {
    g = code;
    const bool locked = (g & 0x4000u) != 0;
    v = (NEED_LW && (locked || !use_counts)) ? exp(lw) : cv + pv;
    if (M.add_count) v += M.add_count[M.norm_of[k]];
  }
  return v;
}

template <bool NEED_LW, int MODE>
__device__ __forceinline__ void wide_stage(const WideRegs<NEED_LW, MODE>& R, const MstepArgs& M, int use_counts, uint32_t span, uint64_t k0,
                                           double* v_sh, uint16_t* g_sh) {
  const uint32_t t = threadIdx.x;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t j = 2 * (t + 256 * h);
    uint16_t g0, g1;
    double2 v;
    v.x = wide_value<NEED_LW>(M, use_counts, (uint16_t)(R.code[h] & 0xffffu), R.c[h].x, R.p[h].x, NEED_LW ? R.l[h].x : 0.0, k0 + j, g0);
    v.y = wide_value<NEED_LW>(M, use_counts, (uint16_t)(R.code[h] >> 16), R.c[h].y, R.p[h].y, NEED_LW ? R.l[h].y : 0.0, k0 + j + 1, g1);
    *reinterpret_cast<double2*>(v_sh + WIDE_HALO + j) = v;
    *reinterpret_cast<uint32_t*>(g_sh + WIDE_HALO + j) = (uint32_t)g0 | ((uint32_t)g1 << 16);
  }
  uint64_t hk = 0;
  uint32_t slot = 0;
  const bool in = wide_halo(k0, span, M.n, hk, slot);
  if (t < 2 * span) {  // (a halo slot outside the table holds "no group, nothing to add", as in mstep_window_kernel)
    uint16_t g;
    v_sh[slot] = wide_value<NEED_LW>(M, use_counts, in ? R.hcode : (uint16_t)0xffffu, R.hc, R.hp, NEED_LW ? R.hl : 0.0, hk, g);
    g_sh[slot] = g;
  }
}

// the per-parameter phase of mstep_window_kernel for one own parameter of the thread: k, in LDS slot me
template <bool NEED_LW, int MODE>
__device__ __forceinline__ double wide_update_one(const MstepArgs& M, uint32_t span, uint64_t k, uint32_t me, double old, uint32_t m32, uint32_t l32,
                                                  unsigned long long m64, unsigned long long l64, const double* v_sh, const uint16_t* g_sh,
                                                  double mx) {
  if (k >= M.n) return mx;
  const uint16_t gid = g_sh[me];
  if (gid == 0xffffu) {  // member normalised by NONE keeps its weights (cascade.h:339-350)
    if (M.save_old == 1) M.old_logw[k] = old;
    return mx;
  }
  const uint16_t want = gid & 0x3fffu;
  double sn = 0.0, sl = 0.0;
  if (MODE == 0) {  // the members are known: add them up in ascending order (the order of the scan below)
    for (uint32_t m = m32; m; m &= m - 1) sn += v_sh[me + (uint32_t)__builtin_ctz(m) - 15u];
    if (NEED_LW)
      for (uint32_t m = l32; m; m &= m - 1) sl += v_sh[me + (uint32_t)__builtin_ctz(m) - 15u];
  } else if (MODE == 1) {
    for (unsigned long long m = m64; m; m &= m - 1) sn += v_sh[me + (uint32_t)__builtin_ctzll(m) - 31u];
    if (NEED_LW)
      for (unsigned long long m = l64; m; m &= m - 1) sl += v_sh[me + (uint32_t)__builtin_ctzll(m) - 31u];
  } else
    for (uint32_t j = me - span; j <= me + span; ++j) {
      const uint16_t gj = g_sh[j];
      if (gj == 0xffffu || (gj & 0x3fffu) != want) continue;
      if (gj & 0x4000u)
        sl += v_sh[j];
      else
        sn += v_sh[j];
    }
  // new weight straight from the sums: one division, one log (and one exp for the old weight) per parameter
  if (M.save_old == 1) M.old_logw[k] = old;
  const double v = v_sh[me];
  double nw;
  if (gid & 0x4000u) {
    nw = v > 0.0 ? log(v) : NEG_INF;
  } else {
    const double remain = 1.0 - sl;
    const bool ok = remain > 0.0 && sn > 0.0 && v > 0.0;
    const double lin = ok ? (sl == 0.0 ? v / sn : v * remain / sn) : 0.0;  // a lone arc: v / v == 1 exactly
    nw = ok ? log(lin) : NEG_INF;
    mx = fmax(mx, fabs(lin - exp(M.save_old ? old : M.old_logw[k])));
  }
  M.logw[k] = nw;
  return mx;
}
// ... for the four of them (unrolled: the compiler interleaves the four log / exp / divide chains; rolled, with the operands
// rotating through one register each, the kernel was 4 us slower on the headline model)
template <bool NEED_LW, int MODE>
__device__ __forceinline__ double wide_update(const WideRegs<NEED_LW, MODE>& R, const MstepArgs& M, uint32_t span, uint64_t k0, const double* v_sh,
                                              const uint16_t* g_sh, double mx) {
#pragma unroll
  for (uint32_t q = 0; q < 4; ++q) {
    const uint32_t j = threadIdx.x + 256 * q;
    mx = wide_update_one<NEED_LW, MODE>(M, span, k0 + j, WIDE_HALO + j, R.old[q], R.m32[q], R.l32[q], R.m64[q], R.l64[q], v_sh, g_sh, mx);
  }
  return mx;
}

// MODE: how a parameter finds its group's members -- 0: mask32 (span <= 15), 1: mask64 (16 .. 31), 2: the scan
template <bool NEED_LW, int MODE>
__global__ __launch_bounds__(256) void mstep_wide_kernel(MstepArgs M, int use_counts, uint32_t span, uint32_t n_pieces) {
  __shared__ __attribute__((aligned(16))) double v_sh[WIDE_PIECE + 2 * WIDE_HALO];
  __shared__ __attribute__((aligned(16))) uint16_t g_sh[WIDE_PIECE + 2 * WIDE_HALO];  // MstepArgs::code16
  __shared__ unsigned long long shm[5];
  double mx = 0.0;
  WideRegs<NEED_LW, MODE> R = {};
  // (the loads of a piece are NOT issued a piece ahead: holding two pieces in registers costs three of the eight resident
  // workgroups per CU, and those hide more latency than the prefetch does -- 85 us against 73 on the headline model)
  for (uint32_t piece = blockIdx.x; piece < n_pieces; piece += gridDim.x) {  // (n_pieces + the grid stays below 2^32: mstep_wide_can)
    const uint64_t k0 = (uint64_t)piece * WIDE_PIECE;
    wide_load(R, M, use_counts, span, k0);
    wide_stage(R, M, use_counts, span, k0, v_sh, g_sh);
    __syncthreads();
    mx = wide_update(R, M, span, k0, v_sh, g_sh, mx);
    __syncthreads();  // (the next piece overwrites the LDS tile)
  }
  // the workgroup's largest change goes to one of MSTEP_WIDE_SLOTS partial slots by atomicMax (a few adds per address) ...
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_down(mx, o, 64));
  if ((threadIdx.x & 63) == 0) shm[threadIdx.x >> 6] = (unsigned long long)__double_as_longlong(mx);
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long m = shm[0];  // non-negative doubles order like their bit patterns
    for (int k = 1; k < 4; ++k) m = shm[k] > m ? shm[k] : m;
    // Nothing but atomics is handed over, so there is no release fence: at agent scope it writes back the whole L2 of the XCD --
    // every weight the kernel has stored so far -- once per workgroup (measured: 1.1 us per arrival, the kernel at twice its
    // time).  Instead the atomicMax is a returning one and the thread waits for its value: the maximum has been performed at
    // device scope before this workgroup's ticket exists, and the last workgroup reads the slots after it has seen every ticket.
    if (m) {
      const unsigned long long was = __hip_atomic_fetch_max(M.max_partial + (blockIdx.x % MSTEP_WIDE_SLOTS), m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      asm volatile("s_waitcnt vmcnt(0)" ::"v"(was) : "memory");
    }
    // ... and the workgroup takes a ticket.  Nobody waits for anybody; whoever draws the last ticket finishes the step.  The
    // workgroups arrive at MSTEP_WIDE_SHARDS counters (128 bytes apart) and the last of each at the root, so that no word
    // sees more than a few hundred arrivals.
    const uint32_t shard = blockIdx.x % MSTEP_WIDE_SHARDS;
    const uint32_t expect = (gridDim.x - shard + MSTEP_WIDE_SHARDS - 1) / MSTEP_WIDE_SHARDS;  // workgroups b with b % SHARDS == shard
    const uint32_t roots = gridDim.x < MSTEP_WIDE_SHARDS ? gridDim.x : MSTEP_WIDE_SHARDS;
    unsigned long long* const sc = M.ticket + 16 * (shard + 1);
    bool last = false;
    if (__hip_atomic_fetch_add(sc, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == expect - 1ull) {
      __hip_atomic_store(sc, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next M-step
      last = __hip_atomic_fetch_add(M.ticket, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == roots - 1ull;
    }
    shm[4] = last;
  }
  __syncthreads();
  if (!shm[4]) return;
  // the last workgroup: what mstep_max_final_kernel does in a launch of its own.  The slots are read AND cleared by atomic
  // exchanges, which are ordered with the other workgroups' atomicMax on whatever XCD those ran (the L2s of different XCDs
  // are not coherent: a plain load could return a stale line).
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  unsigned long long m = 0;
  for (uint32_t k = threadIdx.x; k < MSTEP_WIDE_SLOTS; k += 256) {
    const unsigned long long v = __hip_atomic_exchange(M.max_partial + k, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    m = v > m ? v : m;
  }
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_down(m, o, 64);
    m = other > m ? other : m;
  }
  __syncthreads();  // (shm[4] has been read by everybody)
  if ((threadIdx.x & 63) == 0) shm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) m = shm[k] > m ? shm[k] : m;
    __hip_atomic_store(M.ticket, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // for the next M-step
    *M.max_change_bits = m;
    if (M.box) {  // the host's mailbox: the value, then the sequence number it waits for
      __hip_atomic_store(M.box, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(M.box + 1, M.box_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// the grid: one workgroup per piece, but no more than the device holds at once (or than the caller says); the rest is the loop
template <bool NEED_LW, int MODE>
hipError_t wide_launch(const MstepArgs& M, int use_counts, uint32_t grid_cap, hipStream_t s) {
  static uint32_t resident[64];  // per device, asked once
  if (!grid_cap) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64 || !resident[dev]) {
      int per_cu = 0, cus = 0;
      e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, mstep_wide_kernel<NEED_LW, MODE>, 256, 0);
      if (e != hipSuccess) return e;
      e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
      if (e != hipSuccess) return e;
      grid_cap = (uint32_t)(per_cu > 0 ? per_cu : 1) * (uint32_t)(cus > 0 ? cus : 1);
      if (dev >= 0 && dev < 64) resident[dev] = grid_cap;
    } else
      grid_cap = resident[dev];
  }
  const uint64_t n_pieces = (M.n + WIDE_PIECE - 1) / WIDE_PIECE;
  const uint32_t grid = (uint32_t)(n_pieces < grid_cap ? n_pieces : grid_cap);
  hipLaunchKernelGGL((mstep_wide_kernel<NEED_LW, MODE>), dim3(grid), dim3(256), 0, s, M, use_counts, M.window_span, (uint32_t)n_pieces);
  return hipGetLastError();
}
}  // namespace

bool mstep_wide_can(const MstepArgs& M, int use_counts) {
  if (!M.n || !M.window_span || M.window_span > WIDE_HALO || (M.n_ties && M.tie_of) || M.dig_alpha || M.n_ranges || M.block_first ||
      !M.ticket)
    return false;
  if ((M.n + WIDE_PIECE - 1) / WIDE_PIECE > 0x7fffffffull) return false;
  // the 16-byte (counts, prior, snapshot) and 4-byte (codes) loads need their tables aligned; an external count table may not be
  auto mis = [](const void* p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1)) != 0; };
  return !(mis(M.code16, 4) || (use_counts && (mis(M.counts, 16) || mis(M.prior, 16))) || mis(M.lw_src, 16));
}

hipError_t launch_mstep_wide(const MstepArgs& M, int use_counts, uint32_t grid_cap, hipStream_t s) {
  if (!mstep_wide_can(M, use_counts)) return hipErrorInvalidValue;
  const int mode = M.mask32 ? 0 : M.mask64 ? 1 : 2;
  if (M.lw_src)
    return mode == 0 ? wide_launch<true, 0>(M, use_counts, grid_cap, s)
         : mode == 1 ? wide_launch<true, 1>(M, use_counts, grid_cap, s)
                     : wide_launch<true, 2>(M, use_counts, grid_cap, s);
  return mode == 0 ? wide_launch<false, 0>(M, use_counts, grid_cap, s)
       : mode == 1 ? wide_launch<false, 1>(M, use_counts, grid_cap, s)
                   : wide_launch<false, 2>(M, use_counts, grid_cap, s);
}
}  // namespace carmel_hip
