// forest.hip — forest-em's packed AND/OR derivation forests on the GPU: inside, normalised outside, expected rule
// counts, the EM M-step over normalisation groups, and the Gibbs sampler (inside with proposal probabilities +
// top-down choice).
//
// Replaces /root/reference/forest-em/forest.hpp (inside_rec :636-697, compute_norm_outside :439-491,
// visit_inside_norm_outside :417-438, choose_random :725-758, compute_inside(W) :768-816) and
// forest-em.hpp (estimate :561-578, maximize :626-655, Gibbs glue :694-766); graehl/shared/normalize.hpp:123-164.
//
// Layout: one forest per LANE, 64 forests per wavefront (forests are small: config 5 has ~50 nodes each).  A forest
// is flattened on the host into two record streams over its non-reference nodes renumbered in POST-ORDER (children
// and shared sub-forests before the nodes that use them; a back-reference simply resolves to the shared node):
//   inside stream : per node a header {AND?, rule id} followed by one record per child {child index}
//   outside stream: the same per node, nodes in reverse post-order
// and the 64 streams of a group are interleaved record by record so every wave-wide load is one 512-byte row.
// inside[] (and outside[]) live in the lane's own LDS column(s).  Expected counts reuse the two-phase scheme of the
// lattice path: one posterior per AND node into post[], then count_reduce_kernel with rules in the role of arcs.
// The host side -- the handle, EM and Viterbi entry points, the sampler's schedules -- lives in forest_host.cpp and
// forest_gibbs.cpp; csrc/forest.hpp is what the two sides share, the launch_forest_* at the end of this file what they
// call.  (A `forest.hpp:LINE` in the comments below cites the reference's forest-em/forest.hpp.)
#include <algorithm>
#include "forest.hpp"
#include "rng.hpp"

namespace carmel_hip {

#define F_NEG_INF (-__builtin_huge_val())

__device__ __forceinline__ double f_lwadd(double a, double b) {
  if (a == F_NEG_INF) return b;
  if (b == F_NEG_INF) return a;
  double d = a - b;
  if (d > 36.0) return a;
  if (d < -36.0) return b;
  if (d < 0) return b + log1p(exp(d));
  return a + log1p(exp(-d));
}

// inside over the lane's stream with the rule weights.  The records run three chunks of four ahead of the fold and an
// AND header's weight -- a gather that depends on its record -- one chunk ahead: a wave is alone on its SIMD most of the
// time (two columns of LDS per forest bound the occupancy), nobody else hides the two round trips.
#define FE_CHUNK 4
__device__ __forceinline__ void f_inside(const ForestArgs& A, const FGroup& g, int lane, double* col) {
  const uint2* __restrict__ st = A.ins_stream + g.stream_base + lane;
  const double* __restrict__ lw = A.rule_logw;
  const uint32_t last = g.maxlen - 1;
  uint32_t d = 0;
  bool is_and = false;
  double acc = 0.0, m = F_NEG_INF, sum = 0.0;
  uint2 r[FE_CHUNK], r1[FE_CHUNK], r2[FE_CHUNK];
  double w[FE_CHUNK], w1[FE_CHUNK];
#define FE_LOAD(R, base) \
  _Pragma("unroll") for (int j = 0; j < FE_CHUNK; ++j) R[j] = st[(size_t)min((base) + j, last) * 64];
  // (only an AND header's second word is a rule id: every other record reads entry 0 and ignores it)
#define FE_GATHER(W, R)                                                                                          \
  _Pragma("unroll") for (int j = 0; j < FE_CHUNK; ++j)                                                           \
      W[j] = lw[(R[j].x & (F_VALID | F_HEADER | F_AND)) == (F_VALID | F_HEADER | F_AND) ? R[j].y : 0u];
  FE_LOAD(r, 0u)
  FE_LOAD(r1, (uint32_t)FE_CHUNK)
  FE_GATHER(w, r)
  for (uint32_t k0 = 0; k0 < g.maxlen; k0 += FE_CHUNK) {
    if (k0) {
#pragma unroll
      for (int j = 0; j < FE_CHUNK; ++j) {
        r[j] = r1[j];
        r1[j] = r2[j];
        w[j] = w1[j];
      }
    }
    FE_LOAD(r2, k0 + 2u * FE_CHUNK)
    FE_GATHER(w1, r1)
#pragma unroll
    for (int j = 0; j < FE_CHUNK; ++j) {
      if (k0 + j > last || !(r[j].x & F_VALID)) continue;
      if (r[j].x & F_HEADER) {
        is_and = (r[j].x & F_AND) != 0;
        if (is_and)
          acc = w[j];
        else {
          m = F_NEG_INF;
          sum = 0.0;
        }
      } else {
        const double v = col[(size_t)(r[j].x & F_IDX) * 64];
        if (is_and)
          acc += v;
        else if (v != F_NEG_INF) {  // streaming logsumexp over the OR's children
          if (v <= m)
            sum += exp(v - m);
          else {
            sum = (m == F_NEG_INF) ? 1.0 : sum * exp(m - v) + 1.0;
            m = v;
          }
        }
      }
      if (r[j].x & F_LAST) {
        col[(size_t)d * 64] = is_and ? acc : (sum == 1.0 ? m : (sum > 0.0 ? m + log(sum) : F_NEG_INF));
        ++d;
      }
    }
  }
#undef FE_LOAD
#undef FE_GATHER
}

// EM E-step: inside, normalised outside, posteriors of AND nodes.  LDS: two columns per lane (inside, outside).
// GCOL: the columns live in global memory (A.gcol) -- forests with more nodes than LDS holds, e.g. the derivation
// lattices carmel --fem-forest exports (tens of thousands of nodes each); still one lane per forest.
template <bool GCOL>
__global__ __launch_bounds__(64) void forest_estimate_kernel(ForestArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const FGroup g = A.groups[A.first_group + blockIdx.x];
  const int lane = threadIdx.x;
  const bool active = (uint32_t)lane < g.n_lanes;
  const uint32_t n = active ? A.lane_nodes[g.lane_base + lane] : 0u;
  double* colbase = GCOL ? A.gcol + (size_t)blockIdx.x * A.gcol_stride : lds;
  double* ins = colbase + lane;
  double* out = colbase + (size_t)g.max_nodes * 64 + lane;
  f_inside(A, g, lane, ins);
  double lp = F_NEG_INF;
  if (active) {
    lp = ins[(size_t)(n - 1) * 64];
    A.forest_logprob[A.lane_forest[g.lane_base + lane]] = lp;
    for (uint32_t s = 0; s < n; ++s) out[(size_t)s * 64] = F_NEG_INF;
    if (lp != F_NEG_INF) out[(size_t)(n - 1) * 64] = -lp;  // norm_outside[root] = 1 / inside[root]
  }
  const uint2* __restrict__ st = A.out_stream + g.stream_base + lane;
  double* __restrict__ post = A.post + g.stream_base + lane;
  bool is_and = false;
  double op = F_NEG_INF, ip = F_NEG_INF;
  const uint32_t last = g.maxlen - 1;
  uint2 rr[FE_CHUNK], rr1[FE_CHUNK], rr2[FE_CHUNK];  // three chunks of records in flight, as in the inside pass
#define FE_LOAD(R, base) \
  _Pragma("unroll") for (int j = 0; j < FE_CHUNK; ++j) R[j] = st[(size_t)min((base) + j, last) * 64];
  FE_LOAD(rr, 0u)
  FE_LOAD(rr1, (uint32_t)FE_CHUNK)
  for (uint32_t k0 = 0; k0 < g.maxlen; k0 += FE_CHUNK) {
    if (k0) {
#pragma unroll
      for (int j = 0; j < FE_CHUNK; ++j) {
        rr[j] = rr1[j];
        rr1[j] = rr2[j];
      }
    }
    FE_LOAD(rr2, k0 + 2u * FE_CHUNK)
#pragma unroll
   for (int j = 0; j < FE_CHUNK; ++j) {
    const uint32_t k = k0 + j;
    const uint2 r = rr[j];
    if (k > last || !(r.x & F_VALID)) continue;
    if (r.x & F_HEADER) {
      const uint32_t p = r.x & F_IDX;
      is_and = (r.x & F_AND) != 0;
      op = out[(size_t)p * 64];
      ip = ins[(size_t)p * 64];
      if (is_and) post[(size_t)k * 64] = (lp != F_NEG_INF && op != F_NEG_INF) ? exp(ip + op) : 0.0;
    } else if (lp != F_NEG_INF && op != F_NEG_INF) {
      const uint32_t c = r.x & F_IDX;
      double contrib = op;
      if (is_and) {
        if (ip == F_NEG_INF) continue;  // 0/0 guard of forest.hpp:470
        contrib = op + ip - ins[(size_t)c * 64];
      }
      out[(size_t)c * 64] = f_lwadd(out[(size_t)c * 64], contrib);
    }
   }
  }
#undef FE_LOAD
  double s_lp = (active && lp != F_NEG_INF) ? lp : 0.0, s_n = (active && lp != F_NEG_INF) ? 1.0 : 0.0,
         s_z = (active && lp == F_NEG_INF) ? 1.0 : 0.0;
  for (int o = 32; o > 0; o >>= 1) {
    s_lp += __shfl_down(s_lp, o, 64);
    s_n += __shfl_down(s_n, o, 64);
    s_z += __shfl_down(s_z, o, 64);
  }
  if (lane == 0) {
    unsafeAtomicAdd(A.scalars + 0, s_lp);
    unsafeAtomicAdd(A.scalars + 1, s_n);
    unsafeAtomicAdd(A.scalars + 2, s_z);
  }
}

// The same E-step with inside / outside values as mantissa x 2^exponent pairs (as forest_sample_kernel<.., EXT>): a product is
// a multiply and an integer add, the OR fold / the outside accumulation an aligned add, an AND child's share a divide --
// where the log domain spends an exp and a log1p per child.  12 bytes per value instead of 8 (columns: inside mantissas,
// outside mantissas, then the two exponent columns); differences to the log-domain kernel are rounding (1e-16 relative).
struct FExt {
  double m;  // 0 (the value zero) or in [0.5, 1)
  int e;
};
__device__ __forceinline__ FExt fx_norm(double v, int e) {
  int t;
  FExt r;
  r.m = frexp(v, &t);
  r.e = v == 0.0 ? 0 : e + t;
  return r;
}
__device__ __forceinline__ FExt fx_add(FExt a, FExt b) {  // a + b, either may be zero
  if (a.m == 0.0) return b;
  if (b.m == 0.0) return a;
  const int dd = b.e - a.e;
  return dd <= 0 ? fx_norm(a.m + ldexp(b.m, dd), a.e) : fx_norm(ldexp(a.m, -dd) + b.m, b.e);
}
// a rule's weight from its natural log without leaving the range of a double: 2^(w log2 e) = 2^k x 2^f
__device__ __forceinline__ FExt fx_from_ln(double lnw) {
  FExt r;
  if (lnw == F_NEG_INF) {
    r.m = 0.0;
    r.e = 0;
    return r;
  }
  const double l2 = lnw * 1.4426950408889634074, k = floor(l2);
  return fx_norm(exp2(l2 - k), (int)k);
}
__global__ __launch_bounds__(64) void forest_estimate_ext_kernel(ForestArgs A) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const FGroup g = A.groups[A.first_group + blockIdx.x];
  const int lane = threadIdx.x;
  const bool active = (uint32_t)lane < g.n_lanes;
  const uint32_t n = active ? A.lane_nodes[g.lane_base + lane] : 0u;
  const uint32_t rows = g.max_nodes;
  double* im = lds + lane;
  double* om = lds + (size_t)rows * 64 + lane;
  int* ie = (int*)(lds + (size_t)2 * rows * 64) + lane;
  int* oe = ie + (size_t)rows * 64;
  const uint32_t last = g.maxlen - 1;
  {  // inside (f_inside's pipeline: records three chunks ahead, AND headers' weights one chunk ahead)
    const uint2* __restrict__ st = A.ins_stream + g.stream_base + lane;
    const double* __restrict__ lw = A.rule_logw;
    uint32_t d = 0;
    bool is_and = false;
    FExt acc = {0.0, 0}, sum = {0.0, 0};
    uint2 r[FE_CHUNK], r1[FE_CHUNK], r2[FE_CHUNK];
    double w[FE_CHUNK], w1[FE_CHUNK];
#define FE_LOAD(R, base) \
  _Pragma("unroll") for (int j = 0; j < FE_CHUNK; ++j) R[j] = st[(size_t)min((base) + j, last) * 64];
#define FE_GATHER(W, R)                                                                                          \
  _Pragma("unroll") for (int j = 0; j < FE_CHUNK; ++j)                                                           \
      W[j] = lw[(R[j].x & (F_VALID | F_HEADER | F_AND)) == (F_VALID | F_HEADER | F_AND) ? R[j].y : 0u];
    FE_LOAD(r, 0u)
    FE_LOAD(r1, (uint32_t)FE_CHUNK)
    FE_GATHER(w, r)
    for (uint32_t k0 = 0; k0 < g.maxlen; k0 += FE_CHUNK) {
      if (k0) {
#pragma unroll
        for (int j = 0; j < FE_CHUNK; ++j) {
          r[j] = r1[j];
          r1[j] = r2[j];
          w[j] = w1[j];
        }
      }
      FE_LOAD(r2, k0 + 2u * FE_CHUNK)
      FE_GATHER(w1, r1)
#pragma unroll
      for (int j = 0; j < FE_CHUNK; ++j) {
        // without branches, as the sampler's fold: every candidate is computed, selects keep the one that applies, the
        // node's running value is stored at every record (the last store stays)
        const uint32_t rx = r[j].x;
        if (k0 + j <= last && (rx & F_VALID)) {
          const bool hdr = (rx & F_HEADER) != 0, child = !hdr;
          const size_t c = (size_t)min(rx & F_IDX, rows - 1) * 64;  // (a header's low bits are not a row: read and ignored)
          const double vm = im[c];
          const int ve = ie[c];
          const FExt h = fx_from_ln(w[j]);
          int pe, se;
          const double pm = frexp(acc.m * vm, &pe);
          const int dd = ve - sum.e;
          const bool le = dd <= 0;
          const double lo = le ? vm : sum.m, hi = le ? sum.m : vm;
          const double sm = frexp(hi + ldexp(lo, le ? dd : -dd), &se);
          const bool fold_and = child && is_and, fold_or = child && !is_and && vm != 0.0, sum0 = sum.m == 0.0;
          is_and = hdr ? (rx & F_AND) != 0 : is_and;
          const bool take_h = hdr && is_and;
          acc.e = take_h ? h.e : fold_and ? (acc.m * vm == 0.0 ? 0 : acc.e + ve + pe) : acc.e;
          acc.m = take_h ? h.m : fold_and ? pm : acc.m;
          const int nsum_e = sum0 ? ve : (le ? sum.e : ve) + se;
          const double nsum = sum0 ? vm : sm;
          sum.e = hdr ? 0 : fold_or ? nsum_e : sum.e;
          sum.m = hdr ? 0.0 : fold_or ? nsum : sum.m;
          im[(size_t)d * 64] = is_and ? acc.m : sum.m;
          ie[(size_t)d * 64] = is_and ? acc.e : sum.e;
          d += (rx & F_LAST) ? 1u : 0u;
        }
      }
    }
#undef FE_LOAD
#undef FE_GATHER
  }
  double lp = F_NEG_INF;
  if (active) {
    const double rm = im[(size_t)(n - 1) * 64];
    const int re = ie[(size_t)(n - 1) * 64];
    if (rm != 0.0) lp = log(rm) + (double)re * 0.69314718055994530942;
    A.forest_logprob[A.lane_forest[g.lane_base + lane]] = lp;
    for (uint32_t q = 0; q < n; ++q) {
      om[(size_t)q * 64] = 0.0;
      oe[(size_t)q * 64] = 0;
    }
    if (rm != 0.0) {  // norm_outside[root] = 1 / inside[root]
      const FExt o = fx_norm(1.0 / rm, -re);
      om[(size_t)(n - 1) * 64] = o.m;
      oe[(size_t)(n - 1) * 64] = o.e;
    }
  }
  const uint2* __restrict__ st = A.out_stream + g.stream_base + lane;
  double* __restrict__ post = A.post + g.stream_base + lane;
  bool is_and = false;
  FExt op = {0.0, 0}, ip = {0.0, 0};
  uint2 rr[FE_CHUNK], rr1[FE_CHUNK], rr2[FE_CHUNK];
#define FE_LOAD(R, base) \
  _Pragma("unroll") for (int j = 0; j < FE_CHUNK; ++j) R[j] = st[(size_t)min((base) + j, last) * 64];
  FE_LOAD(rr, 0u)
  FE_LOAD(rr1, (uint32_t)FE_CHUNK)
  for (uint32_t k0 = 0; k0 < g.maxlen; k0 += FE_CHUNK) {
    if (k0) {
#pragma unroll
      for (int j = 0; j < FE_CHUNK; ++j) {
        rr[j] = rr1[j];
        rr1[j] = rr2[j];
      }
    }
    FE_LOAD(rr2, k0 + 2u * FE_CHUNK)
#pragma unroll
    for (int j = 0; j < FE_CHUNK; ++j) {
      const uint32_t k = k0 + j;
      const uint2 r = rr[j];
      if (k > last || !(r.x & F_VALID)) continue;
      // one straight line for headers and children alike (the lanes of a wave are at both): the row's four values are
      // read, a header keeps them as its node's, a child adds its share to them and stores them back
      const bool hdr = (r.x & F_HEADER) != 0;
      const size_t c = (size_t)min(r.x & F_IDX, rows - 1) * 64;
      const double cm_o = om[c], cm_i = im[c];
      const int ce_o = oe[c], ce_i = ie[c];
      if (hdr) {
        is_and = (r.x & F_AND) != 0;
        op.m = cm_o;
        op.e = ce_o;
        ip.m = cm_i;
        ip.e = ce_i;
        if (is_and) post[(size_t)k * 64] = (lp != F_NEG_INF && op.m != 0.0) ? ldexp(ip.m * op.m, ip.e + op.e) : 0.0;
      }
      // a child's share: the parent's outside value (OR), or outside x inside of the parent / inside of the child (AND;
      // 0/0 guard of forest.hpp:470: an AND parent of inside zero passes nothing on)
      const bool share = !hdr && lp != F_NEG_INF && op.m != 0.0 && !(is_and && ip.m == 0.0);
      int qe, se;
      const double qm = frexp(is_and ? op.m * ip.m / cm_i : op.m, &qe);
      const int q_e = (is_and ? op.e + ip.e - ce_i : op.e) + qe;
      const int dd = q_e - ce_o;
      const bool le = dd <= 0;
      const double lo = le ? qm : cm_o, hi = le ? cm_o : qm;
      const double sm = frexp(hi + ldexp(lo, le ? dd : -dd), &se);
      const bool cur0 = cm_o == 0.0;
      if (share) {
        om[c] = cur0 ? qm : sm;
        oe[c] = cur0 ? q_e : (le ? ce_o : q_e) + se;
      }
    }
  }
#undef FE_LOAD
  double s_lp = (active && lp != F_NEG_INF) ? lp : 0.0, s_n = (active && lp != F_NEG_INF) ? 1.0 : 0.0,
         s_z = (active && lp == F_NEG_INF) ? 1.0 : 0.0;
  for (int o = 32; o > 0; o >>= 1) {
    s_lp += __shfl_down(s_lp, o, 64);
    s_n += __shfl_down(s_n, o, 64);
    s_z += __shfl_down(s_z, o, 64);
  }
  if (lane == 0) {
    unsafeAtomicAdd(A.scalars + 0, s_lp);
    unsafeAtomicAdd(A.scalars + 1, s_n);
    unsafeAtomicAdd(A.scalars + 2, s_z);
  }
}

// Gibbs: resample every forest of the group (or, exact mode, the single forest A.serial_forest) against snap_x /
// snap_norm.  LDS per lane: the inside column.
template <bool GCOL>
__global__ __launch_bounds__(64) void forest_gibbs_kernel(ForestArgs A, uint32_t max_sample, uint32_t ins_rows,
                                                           uint32_t own_cap, uint32_t stack_lds) {
  extern __shared__ __attribute__((aligned(16))) double lds_all[];
  double* colbase = GCOL ? A.gcol + (size_t)blockIdx.x * A.gcol_stride : lds_all;
  double* aux = GCOL ? lds_all : lds_all + (size_t)ins_rows * 64;  // tables and stack follow the column when it is in LDS
  const FGroup g = A.groups[A.first_group + blockIdx.x];
  const int lane = threadIdx.x;
  bool active = (uint32_t)lane < g.n_lanes;
  if (A.serial_forest != 0xffffffffu) active = active && (g.lane_base + lane == A.serial_forest);
  const uint32_t n = active ? A.lane_nodes[g.lane_base + lane] : 0u;
  double* ins = colbase + lane;
  const uint32_t forest = active ? A.lane_forest[g.lane_base + lane] : 0u;
  // the lane's previous sample (counterfactual removal) is read straight from global memory; the traversal stack
  // lives at the tail of the forest's own sample buffer (recorded rules grow from the front, pending nodes from the
  // back: every pending node still owes at least one rule, so the two never meet)
  unsigned long long tr0 = A.trace ? __builtin_readcyclecounter() : 0, tr1 = 0, tr2 = 0, tr3 = 0;
  uint32_t own_len = 0;
  const uint32_t* own = A.old_rules + (active ? A.sample_off[forest] : 0);
  if (active && A.counterfactual) own_len = A.old_len[forest];
  // ... counted into a small open-addressing table in the lane's LDS column ({rule or norm-group id, uses}): every
  // proposal probability needs "how often does my previous sample use this rule / this group" (counterfactual CRP
  // counts), and scanning the sample for each AND node (two dependent global gathers per scanned rule) made this
  // kernel 15x slower than the estimate kernel on the same forests.  own_cap = table slots (a power of two, 0 = scan).
  // a lane whose sample is too long for its LDS column uses a table in global memory instead (FOREST_GHASH slots
  // per forest): the rare long derivation must not fall back to scanning -- one such lane held its wave 30x longer.
  // The two tables are handled by separate code (LDS / global address spaces), never through one generic pointer.
  uint32_t* ht_l = (uint32_t*)aux + lane;  // stride 64
  uint32_t* ht_g = A.ghash ? A.ghash + (size_t)forest * FOREST_GHASH : nullptr;  // stride 1
  const bool hashed_l = own_cap != 0 && own_len * 20 <= own_cap * 9;  // <= 2 keys per rule, load factor <= 0.9
  const bool hashed_g = !hashed_l && active && ht_g != nullptr && own_len * 20 <= FOREST_GHASH * 9;
  uint32_t gcap = 64;  // slots of the global table this lane uses: the smallest power of two with load factor <= 0.9
  while (gcap * 9 < own_len * 20) gcap <<= 1;
  const bool hashed = hashed_l || hashed_g;
#define FH_SLOT(key, mask) ((((key) * 2654435761u) >> 7) & (mask))
#define FH_ADD(tab, stride, mask, key_)                              \
  {                                                                  \
    const uint32_t key = (key_);                                     \
    for (uint32_t h = FH_SLOT(key, mask);; h = (h + 1) & (mask)) {   \
      const uint32_t cur = (tab)[(size_t)h * (stride)];              \
      if (cur == 0xffffffffu) {                                      \
        (tab)[(size_t)h * (stride)] = (key << 8) | 1u;               \
        break;                                                       \
      }                                                              \
      if ((cur >> 8) == key) {                                       \
        (tab)[(size_t)h * (stride)] = cur + 1u;                      \
        break;                                                       \
      }                                                              \
    }                                                                \
  }
  if (hashed_l) {
    const uint32_t mask = own_cap - 1;
    for (uint32_t i = 0; i < own_cap; ++i) ht_l[(size_t)i * 64] = 0xffffffffu;
    for (uint32_t q = 0; q < own_len; ++q) {
      const uint32_t rr = own[q], nr = A.p_norm[rr];
      FH_ADD(ht_l, 64, mask, rr)
      if (nr != F_NONORM) FH_ADD(ht_l, 64, mask, nr | 0x800000u)
    }
  } else if (hashed_g) {
    const uint32_t mask = gcap - 1;
    for (uint32_t i = 0; i < gcap; ++i) ht_g[i] = 0xffffffffu;
    for (uint32_t q = 0; q < own_len; ++q) {
      const uint32_t rr = own[q], nr = A.p_norm[rr];
      FH_ADD(ht_g, 1, mask, rr)
      if (nr != F_NONORM) FH_ADD(ht_g, 1, mask, nr | 0x800000u)
    }
  }
#undef FH_ADD
  auto own_uses = [&](uint32_t key) -> double {  // uses of a rule (key = id) or of a norm group (key = id | 1 << 23)
    if (hashed_l) {
      const uint32_t mask = own_cap - 1;
      for (uint32_t h = FH_SLOT(key, mask);; h = (h + 1) & mask) {
        const uint32_t cur = ht_l[(size_t)h * 64];
        if (cur == 0xffffffffu) return 0.0;
        if ((cur >> 8) == key) return (double)(cur & 0xffu);
      }
    } else {
      const uint32_t mask = gcap - 1;
      for (uint32_t h = FH_SLOT(key, mask);; h = (h + 1) & mask) {
        const uint32_t cur = ht_g[h];
        if (cur == 0xffffffffu) return 0.0;
        if ((cur >> 8) == key) return (double)(cur & 0xffu);
      }
    }
  };
  if (A.trace) tr1 = __builtin_readcyclecounter();
  // inside with proposal probabilities (forest.hpp:768-816)
  {
    const uint2* __restrict__ st = A.ins_stream + g.stream_base + lane;
    uint32_t d = 0;
    bool is_and = false;
    double acc = 0.0, sum = F_NEG_INF;
    for (uint32_t k = 0; k < g.maxlen; ++k) {
      const uint2 r = st[(size_t)k * 64];
      if (!active || !(r.x & F_VALID)) continue;
      if (r.x & F_HEADER) {
        is_and = (r.x & F_AND) != 0;
        if (is_and) {
          const uint32_t rule = r.y, nn = A.p_norm[rule];
          double pr;
          if (nn == F_NONORM)
            pr = A.p_prior[rule];
          else {
            double x = A.snap_x[rule], ns = A.snap_norm[nn];
            if (hashed) {
              x -= own_uses(rule);
              ns -= own_uses(nn | 0x800000u);
            } else {
              for (uint32_t q = 0; q < own_len; ++q) {
                const uint32_t rr = own[q];
                if (rr == rule) x -= 1.0;
                if (A.p_norm[rr] == nn) ns -= 1.0;
              }
            }
            pr = x / ns;
          }
          acc = log(pr);
        } else
          sum = F_NEG_INF;
      } else {
        const double v = ins[(size_t)(r.x & F_IDX) * 64];
        if (is_and)
          acc += v;
        else
          sum = f_lwadd(sum, v);  // the reference's pairwise OR fold (forest.hpp:790-797)
      }
      if (r.x & F_LAST) {
        ins[(size_t)d * 64] = is_and ? acc : sum;
        ++d;
      }
    }
  }
  if (A.trace) tr2 = __builtin_readcyclecounter();
  // top-down choice (forest.hpp:725-758) with an explicit stack; children are pushed in reverse so they pop in order
  double cheap = 0.0;
  if (active) {
    const uint2* __restrict__ st = A.ins_stream + g.stream_base + lane;
    const uint32_t* __restrict__ hp = A.hdr_pos + g.stream_base + lane;  // indexed [node * 64]
    uint32_t* outr = A.sample_rules + A.sample_off[forest];
    const uint32_t cap = (uint32_t)(A.sample_off[forest + 1] - A.sample_off[forest]);
    uint32_t* stack = outr + cap;  // deep part of the stack: stack[-1 - i]
    uint32_t* stk_sh = (uint32_t*)aux + (size_t)own_cap * 64 + lane;  // first stack_lds entries
#define FSTACK_PUSH(v)                                       \
  {                                                          \
    if (sp < stack_lds)                                      \
      stk_sh[(size_t)sp * 64] = (v);                         \
    else                                                     \
      stack[-(int)(sp - stack_lds) - 1] = (v);               \
    ++sp;                                                    \
  }
    uint32_t sp = 0, ns = 0, step = 0;
    FSTACK_PUSH(n - 1)
    while (sp) {
      --sp;
      // bit 31 of a stack entry: the node was reached through a back-reference, below which the reference chooses at
      // temperature 1 (forest.hpp:731-732 drops `power`)
      const uint32_t entry = sp < stack_lds ? stk_sh[(size_t)sp * 64] : stack[-(int)(sp - stack_lds) - 1];
      const uint32_t node = entry & F_IDX, cold = entry & 0x80000000u;
      const uint32_t h = hp[(size_t)node * 64];
      const uint2 hr = st[(size_t)h * 64];
      // children occupy records h+1 .. h+nch; the count rides in the header (no dependent scan of the records)
      uint32_t nch = (hr.x >> 20) & 0xffu;
      if (nch == 255u) {
        nch = 0;
        for (uint32_t k = h + 1;; ++k) {
          ++nch;
          if (st[(size_t)k * 64].x & F_LAST) break;
        }
      }
      if (hr.x & F_AND) {
        if (ns < max_sample) outr[ns] = hr.y;
        ++ns;
        for (uint32_t k = nch; k-- > 0;) {
          const uint2 cr = st[(size_t)(h + 1 + k) * 64];
          FSTACK_PUSH((cr.x & F_IDX) | cold | (cr.y & 0x80000000u))
        }
      } else {
        const double power = cold ? 1.0 : A.power;
        double norm = F_NEG_INF;
        for (uint32_t k = 0; k < nch; ++k) norm = f_lwadd(norm, ins[(size_t)(st[(size_t)(h + 1 + k) * 64].x & F_IDX) * 64] * power);
        double choice = gibbs_uniform(A.seed, A.iter, forest, step++);
        uint32_t pick = 0;
        for (uint32_t k = 0;; ++k) {
          pick = k;
          choice -= exp(ins[(size_t)(st[(size_t)(h + 1 + k) * 64].x & F_IDX) * 64] * power - norm);
          if (choice < 0 || k + 1 == nch) break;
        }
        const uint2 cr = st[(size_t)(h + 1 + pick) * 64];
        FSTACK_PUSH((cr.x & F_IDX) | cold | (cr.y & 0x80000000u))
      }
    }
#undef FSTACK_PUSH
    if (A.trace) tr3 = __builtin_readcyclecounter();
    A.sample_len[forest] = ns < max_sample ? ns : max_sample;
    for (uint32_t k = 0; k < ns && k < max_sample; ++k) {
      const uint32_t rule = outr[k], nn = A.p_norm[rule];
      double pr;
      if (nn == F_NONORM)
        pr = A.p_prior[rule];
      else {
        double x = A.snap_x[rule], nsum = A.snap_norm[nn];
        if (hashed) {
          x -= own_uses(rule);
          nsum -= own_uses(nn | 0x800000u);
        } else {
          for (uint32_t q = 0; q < own_len; ++q) {
            const uint32_t rr = own[q];
            if (rr == rule) x -= 1.0;
            if (A.p_norm[rr] == nn) nsum -= 1.0;
          }
        }
        pr = x / nsum;
      }
      cheap += log(pr);
    }
  }
  for (int o = 32; o > 0; o >>= 1) cheap += __shfl_down(cheap, o, 64);
  if (lane == 0) unsafeAtomicAdd(A.iter_out + 1, cheap);
  if (A.trace) {
    unsigned long long t3 = tr3;
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_down(t3, o, 64);
      t3 = other > t3 ? other : t3;
    }
    if (lane == 0) {
      unsigned long long* o = A.trace + (size_t)(A.first_group + blockIdx.x) * 8;
      o[0] = tr0; o[1] = tr1; o[2] = tr2; o[3] = t3; o[4] = __builtin_readcyclecounter(); o[5] = g.maxlen; o[6] = g.n_lanes;
    }
  }
}

// ---------------- parallel sweep, second formulation ----------------
// The sweep above spends its time in chains of dependent gathers made by one lane per forest (count tables, rule ->
// group -> counts per AND node, one node per round trip in the walk): at 1563 waves of 64 forests the chip idles.
// Here everything that does not depend on the recursion runs with one thread per record or per sample entry:
//   forest_proposal_kernel  one thread per AND header (a static list of them, forest after forest): proposal probability
//                           of its rule ((count - own uses) / (group sum - own uses), gibbs.hpp:589-592 with the block's
//                           own sample taken out).  Equal rules / equal norm groups within a forest form CLASSES
//                           (rec_cls, static); "own uses" = how many class words of the forest's previous sample
//                           (sample_cls, left by the recount) match -- a short scan, shared by the threads of a wave.
//   forest_sample_kernel    one lane per forest: inside pass as a pure stream (record + its p, three chunks in flight),
//                           top-down walk over 16-bit tables the inside pass leaves in LDS (LW; otherwise over the
//                           global stream, one round trip per visited node).
//   forest_recount_kernel   one thread per sample entry: rule ids and class words of the new sample, counts, proposal
//                           probability of the sample.
__global__ __launch_bounds__(256) void forest_proposal_kernel(ForestArgs A) {
  // one thread per AND header, from the static list of them ({position, group, classes, rule}: the records themselves are
  // not read, and the 55 % of the stream that is not an AND header is not visited)
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n_and) return;
  const FAnd e = A.and_list[i];
  const uint32_t rule = e.rule, nn = A.p_norm[rule];
  double pr;
  if (nn == F_NONORM)
    pr = A.p_prior[rule];
  else {
    // how often the forest's previous sample uses this rule / this norm group: a scan of the sample's class words.  The
    // list is ordered by forest, so the threads of a wave scan the same few samples together (the reads are broadcasts)
    const uint32_t c = e.cls, cr = c & 0xffffu, cn = c >> 16;
    const uint32_t* __restrict__ sc = A.sample_cls + A.sample_off[e.forest];
    const uint32_t len = A.old_len[e.forest];
    uint32_t own_r = 0, own_n = 0, j = 0;
    for (; j + 4 <= len; j += 4) {  // four words in flight
      const uint32_t w0 = sc[j], w1 = sc[j + 1], w2 = sc[j + 2], w3 = sc[j + 3];
      own_r += ((w0 & 0xffffu) == cr) + ((w1 & 0xffffu) == cr) + ((w2 & 0xffffu) == cr) + ((w3 & 0xffffu) == cr);
      own_n += ((w0 >> 16) == cn) + ((w1 >> 16) == cn) + ((w2 >> 16) == cn) + ((w3 >> 16) == cn);
    }
    for (; j < len; ++j) {
      const uint32_t w = sc[j];
      own_r += (w & 0xffffu) == cr ? 1u : 0u;
      own_n += (w >> 16) == cn ? 1u : 0u;
    }
    const double x = A.snap_x[rule] - (double)own_r;
    const double ns = A.snap_norm[nn] - (double)own_n;
    pr = x / ns;
  }
  A.rec_p[e.pos] = pr;
  if (!A.p_only) A.rec_logp[e.pos] = log(pr);
}

#define FS_CHUNK 4
// EXT (temperature 1): inside values as mantissa x 2^exponent (frexp / ldexp are single instructions) instead of
// logarithms -- a product is a multiply and an integer add, the OR fold an aligned add, a choice probability a
// multiply by the reciprocal of the node's own inside value: a few instructions where the log domain spends an exp
// and a log1p per child.  Differences to the log-domain fold are rounding (1e-16 relative).
//
// LW (walk tables in LDS): the top-down walk is a chain of dependent reads -- a node's record names its children -- and
// from the global stream each visited node costs a memory round trip (~2 500 cycles; the walk was 2/3 of a wave's time).
// The inside pass sees every record anyway, so it leaves the walk's view of the forest in LDS as 16-bit words: per node
// the slot of its first child (| 0x8000 = AND) and the stream position of its header, per child entry the child's node
// (| 0x8000 = reached through a back-reference).  The walk then reads LDS only (same order, same uniforms, same
// arithmetic: the same sample) and leaves the header positions of the chosen rules; forest_recount_kernel, which reads
// the records at those positions anyway, writes the rule ids into the sample.
template <bool GCOL, bool EXT, bool LW>
__global__ __launch_bounds__(64) void forest_sample_kernel(ForestArgs A, uint32_t max_sample, uint32_t ins_rows,
                                                            uint32_t stack_lds, uint32_t kid_rows) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  double* colbase = GCOL ? A.gcol + (size_t)blockIdx.x * A.gcol_stride : lds;
  // the stack follows the column(s) when they are in LDS (EXT: mantissas, then the exponents at half the size)
  double* aux = GCOL ? lds : lds + (size_t)ins_rows * 64 + (EXT ? (size_t)ins_rows * 32 : 0);
  const FGroup g = A.groups[A.first_group + blockIdx.x];
  const int lane = threadIdx.x;
  const bool active = (uint32_t)lane < g.n_lanes;
  const uint32_t n = active ? A.lane_nodes[g.lane_base + lane] : 0u;
  const uint32_t forest = active ? A.lane_forest[g.lane_base + lane] : 0u;
  double* ins = colbase + lane;                                           // ln inside, or its mantissa (EXT)
  int* ine = (int*)(colbase + (size_t)ins_rows * 64) + lane;              // EXT: its exponent
  // LW: 16-bit rows after the columns: first-child slot per node (+ one closing row), header position per node, child
  // entries, the walk's stack
  unsigned short* wt = (unsigned short*)aux + lane;
  unsigned short* ht = wt + (size_t)(ins_rows + 1) * 64;
  unsigned short* ct = ht + (size_t)ins_rows * 64;
  unsigned short* stk16 = ct + (size_t)kid_rows * 64;
  uint32_t slot = 0, hpos = 0;
  const uint2* __restrict__ st = A.ins_stream + g.stream_base + lane;
  const double* __restrict__ lp = (EXT ? A.rec_p : A.rec_logp) + g.stream_base + lane;
  const uint32_t last = g.maxlen - 1;
  unsigned long long tr0 = A.trace ? __builtin_readcyclecounter() : 0, tr2 = 0, tr3 = 0;
  // inside with the proposal probabilities (forest.hpp:768-816)
  {
    uint32_t d = 0;
    bool is_and = false;
    double acc = 0.0, sum = F_NEG_INF;
    int acc_e = 0, sum_e = 0;  // EXT: acc / sum are mantissas
    // three chunks of records in flight: the loads of chunk k + 2 are issued before chunk k is folded (a wave is alone
    // on its SIMD most of the time -- LDS bounds the occupancy --, so nobody else hides the stream's latency)
    uint2 r[FS_CHUNK], r1[FS_CHUNK], r2[FS_CHUNK];
    double p[FS_CHUNK], p1[FS_CHUNK], p2[FS_CHUNK];
#define FS_LOAD(R, P, base)                                  \
  _Pragma("unroll") for (int j = 0; j < FS_CHUNK; ++j) {     \
    const uint32_t k = min((base) + j, last);                \
    R[j] = st[(size_t)k * 64];                               \
    P[j] = lp[(size_t)k * 64];                               \
  }
    FS_LOAD(r, p, 0u)
    FS_LOAD(r1, p1, (uint32_t)FS_CHUNK)
    for (uint32_t k0 = 0; k0 < g.maxlen; k0 += FS_CHUNK) {
      if (k0) {
#pragma unroll
        for (int j = 0; j < FS_CHUNK; ++j) {
          r[j] = r1[j];
          p[j] = p1[j];
          r1[j] = r2[j];
          p1[j] = p2[j];
        }
      }
      FS_LOAD(r2, p2, k0 + 2u * FS_CHUNK)
#pragma unroll
      for (int j = 0; j < FS_CHUNK; ++j) {
        if constexpr (EXT && LW) {
          // the same fold without branches: a wave's lanes sit at headers, AND children and OR children alike, every
          // branch was taken by somebody and the jumps around them cost as much as the arithmetic.  All candidates
          // are computed (the same operations on the same operands as below), selects keep the one that applies; the
          // node's running value and header position are stored at every record, the last store stays.
          const uint32_t rx = r[j].x, ry = r[j].y;
          if (k0 + j <= last && active && (rx & F_VALID)) {
            const bool hdr = (rx & F_HEADER) != 0, child = !hdr;
            const uint32_t row = min(rx & F_IDX, ins_rows - 1);  // (a header's low bits are not a row: read and ignored)
            const double vm = ins[(size_t)row * 64];
            const int ve = ine[(size_t)row * 64];
            hpos = hdr ? k0 + j : hpos;
            unsigned short* tp = hdr ? wt + (size_t)d * 64 : ct + (size_t)slot * 64;
            *tp = (unsigned short)(hdr ? (slot | ((rx & F_AND) ? 0x8000u : 0u)) : ((rx & 0x7fffu) | ((ry >> 31) << 15)));
            ht[(size_t)d * 64] = (unsigned short)hpos;
            slot += child ? 1u : 0u;
            int he, pe, se;
            const double hm = frexp(p[j], &he);
            const double pm = frexp(acc * vm, &pe);
            const int dd = ve - sum_e;
            const bool le = dd <= 0;
            const double lo = le ? vm : sum, hi = le ? sum : vm;
            const double sm = frexp(hi + ldexp(lo, le ? dd : -dd), &se);
            const bool fold_and = child && is_and, fold_or = child && !is_and && vm != 0.0, sum0 = sum == 0.0;
            acc_e = hdr ? he : fold_and ? acc_e + ve + pe : acc_e;
            acc = hdr ? hm : fold_and ? pm : acc;
            const int nsum_e = sum0 ? ve : (le ? sum_e : ve) + se;
            const double nsum = sum0 ? vm : sm;
            sum_e = hdr ? 0 : fold_or ? nsum_e : sum_e;
            sum = hdr ? 0.0 : fold_or ? nsum : sum;
            is_and = hdr ? (rx & F_AND) != 0 : is_and;
            ins[(size_t)d * 64] = is_and ? acc : sum;
            ine[(size_t)d * 64] = is_and ? acc_e : sum_e;
            d += (rx & F_LAST) ? 1u : 0u;
          }
          continue;
        }
        if (k0 + j > last || !active || !(r[j].x & F_VALID)) continue;
        if (LW) {
          if (r[j].x & F_HEADER) {
            wt[(size_t)d * 64] = (unsigned short)(slot | ((r[j].x & F_AND) ? 0x8000u : 0u));
            ht[(size_t)d * 64] = (unsigned short)(k0 + j);
          } else {
            ct[(size_t)slot * 64] = (unsigned short)((r[j].x & 0x7fffu) | ((r[j].y >> 31) << 15));
            ++slot;
          }
        }
        if (EXT) {
          if (r[j].x & F_HEADER) {
            is_and = (r[j].x & F_AND) != 0;
            acc = frexp(p[j], &acc_e);
            sum = 0.0;
            sum_e = 0;
          } else {
            const double vm = ins[(size_t)(r[j].x & F_IDX) * 64];
            const int ve = ine[(size_t)(r[j].x & F_IDX) * 64];
            if (is_and) {
              int t;
              acc = frexp(acc * vm, &t);
              acc_e += ve + t;
            } else if (vm != 0.0) {
              if (sum == 0.0) {
                sum = vm;
                sum_e = ve;
              } else {
                const int dd = ve - sum_e;
                int t;
                if (dd <= 0)
                  sum = frexp(sum + ldexp(vm, dd), &t);
                else {
                  sum = frexp(ldexp(sum, -dd) + vm, &t);
                  sum_e = ve;
                }
                sum_e += t;
              }
            }
          }
          if (r[j].x & F_LAST) {
            ins[(size_t)d * 64] = is_and ? acc : sum;
            ine[(size_t)d * 64] = is_and ? acc_e : sum_e;
            ++d;
          }
          continue;
        }
        if (r[j].x & F_HEADER) {
          is_and = (r[j].x & F_AND) != 0;
          acc = p[j];
          sum = F_NEG_INF;
        } else {
          const double v = ins[(size_t)(r[j].x & F_IDX) * 64];
          if (is_and)
            acc += v;
          else
            sum = f_lwadd(sum, v);  // the reference's pairwise OR fold (forest.hpp:790-797)
        }
        if (r[j].x & F_LAST) {
          ins[(size_t)d * 64] = is_and ? acc : sum;
          ++d;
        }
      }
    }
  }
  if (A.trace) tr2 = __builtin_readcyclecounter();
  if (LW && active) {
    // the same walk over the LDS tables; stack entries: node | 0x8000 = below a back-reference
    wt[(size_t)n * 64] = (unsigned short)slot;
    uint32_t* outh = A.sample_hdr + A.sample_off[forest];
    const uint32_t cap = (uint32_t)(A.sample_off[forest + 1] - A.sample_off[forest]);
    uint32_t* stack = A.sample_rules + A.sample_off[forest] + cap;  // deep part of the stack: stack[-1 - i]
#define FSTACK_PUSH(v)                                       \
  {                                                          \
    if (sp < stack_lds)                                      \
      stk16[(size_t)sp * 64] = (unsigned short)(v);          \
    else                                                     \
      stack[-(int)(sp - stack_lds) - 1] = (v);               \
    ++sp;                                                    \
  }
    // `entry` = the node to visit next, kept in a register when it is the child just chosen or an AND node's first
    // child (what the stack would hand back at once); F_NONE = take it from the stack
    const uint32_t F_NONE = 0xffffffffu;
    uint32_t sp = 0, ns = 0, step = 0, entry = n - 1;
    // One turn of the loop = an OR node's choice AND the chosen AND node's expansion: the lanes of a wave sit at OR and at
    // AND nodes alike, so both halves are executed every turn anyway -- visiting the pair in one turn halves the turns.
    for (;;) {
      if (entry == F_NONE) {
        if (!sp) break;
        --sp;
        entry = sp < stack_lds ? (uint32_t)stk16[(size_t)sp * 64] : stack[-(int)(sp - stack_lds) - 1];
      }
      uint32_t me = entry & 0x7fffu, cold = entry & 0x8000u;
      uint32_t w0 = wt[(size_t)me * 64], w1 = wt[(size_t)(me + 1) * 64];
      uint32_t first = w0 & 0x7fffu, nch = (w1 & 0x7fffu) - first;
      if (!(w0 & 0x8000u)) {
        uint32_t pick = 0;
        if (EXT) {
          // the first four children's shares at once (rows past the node's children are read and ignored: every row
          // below kid_rows exists), then the reference's serial subtraction without branches: the same differences in
          // the same order, the first one below zero (or the last child) is the choice
          uint32_t ci4[4];
          double t4[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) ci4[q] = ct[(size_t)min(first + q, kid_rows - 1) * 64] & 0x7fffu;
          // (the shares are taken against u x the node's own value instead of dividing each by it: choice, children and
          // the node's value all in units of 2^ne -- the reference's comparison times a positive constant)
          const double zm = ins[(size_t)me * 64];
          const int ne = ine[(size_t)me * 64];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const uint32_t row = min(ci4[q], ins_rows - 1);
            t4[q] = ldexp(ins[(size_t)row * 64], ine[(size_t)row * 64] - ne);
          }
          double choice = gibbs_uniform(A.seed, A.iter, forest, step++) * zm;
          const double c0 = choice - t4[0], c1 = c0 - t4[1], c2 = c1 - t4[2], c3 = c2 - t4[3];
          const bool s0 = c0 < 0 || nch == 1, s1 = c1 < 0 || nch == 2, s2 = c2 < 0 || nch == 3, s3 = c3 < 0 || nch == 4;
          pick = s0 ? 0u : s1 ? 1u : s2 ? 2u : 3u;
          if (!(s0 || s1 || s2 || s3)) {
            choice = c3;
            for (uint32_t k = 4;; ++k) {
              pick = k;
              const uint32_t ci = ct[(size_t)(first + k) * 64] & 0x7fffu;
              choice -= ldexp(ins[(size_t)ci * 64], ine[(size_t)ci * 64] - ne);
              if (choice < 0 || k + 1 == nch) break;
            }
          }
        } else {
          const double power = cold ? 1.0 : A.power;
          double norm = ins[(size_t)me * 64];
          if (power != 1.0) {
            norm = F_NEG_INF;
            for (uint32_t k = 0; k < nch; ++k)
              norm = f_lwadd(norm, ins[(size_t)(ct[(size_t)(first + k) * 64] & 0x7fffu) * 64] * power);
          }
          double choice = gibbs_uniform(A.seed, A.iter, forest, step++);
          for (uint32_t k = 0;; ++k) {
            pick = k;
            choice -= exp(ins[(size_t)(ct[(size_t)(first + k) * 64] & 0x7fffu) * 64] * power - norm);
            if (choice < 0 || k + 1 == nch) break;
          }
        }
        entry = (uint32_t)ct[(size_t)(first + pick) * 64] | cold;
        me = entry & 0x7fffu;
        cold = entry & 0x8000u;
        w0 = wt[(size_t)me * 64];
        w1 = wt[(size_t)(me + 1) * 64];
        first = w0 & 0x7fffu;
        nch = (w1 & 0x7fffu) - first;
      }
      if (w0 & 0x8000u) {
        if (ns < max_sample) outh[ns] = ht[(size_t)me * 64];
        ++ns;
        for (uint32_t k = nch; k-- > 1;) FSTACK_PUSH((uint32_t)ct[(size_t)(first + k) * 64] | cold)
        entry = nch ? ((uint32_t)ct[(size_t)first * 64] | cold) : F_NONE;
      }
    }
#undef FSTACK_PUSH
    A.sample_len[forest] = ns < max_sample ? ns : max_sample;
  }
  // top-down choice (forest.hpp:725-758); stack entries: header position | bit 31 = below a back-reference
  if (!LW && active) {
    uint32_t* outr = A.sample_rules + A.sample_off[forest];
    uint32_t* outh = A.sample_hdr + A.sample_off[forest];
    const uint32_t cap = (uint32_t)(A.sample_off[forest + 1] - A.sample_off[forest]);
    uint32_t* stack = outr + cap;  // deep part of the stack: stack[-1 - i]
    uint32_t* stk_sh = (uint32_t*)aux + lane;
#define FSTACK_PUSH(v)                                       \
  {                                                          \
    if (sp < stack_lds)                                      \
      stk_sh[(size_t)sp * 64] = (v);                         \
    else                                                     \
      stack[-(int)(sp - stack_lds) - 1] = (v);               \
    ++sp;                                                    \
  }
    uint32_t sp = 0, ns = 0, step = 0;
    FSTACK_PUSH(A.hdr_pos[g.stream_base + (size_t)(n - 1) * 64 + lane])
    while (sp) {
      --sp;
      const uint32_t entry = sp < stack_lds ? stk_sh[(size_t)sp * 64] : stack[-(int)(sp - stack_lds) - 1];
      const uint32_t h = entry & 0x7fffffffu, cold = entry & 0x80000000u;
      const uint2 hr = st[(size_t)h * 64];
      uint2 c[4];  // the first children ride along with the header: one round trip per node
#pragma unroll
      for (int j = 0; j < 4; ++j) c[j] = st[(size_t)min(h + 1 + j, last) * 64];
      uint32_t nch = (hr.x >> 20) & 0xffu;
      if (nch == 255u) {
        nch = 0;
        for (uint32_t k = h + 1;; ++k) {
          ++nch;
          if (st[(size_t)k * 64].x & F_LAST) break;
        }
      }
      if (hr.x & F_AND) {
        if (ns < max_sample) {
          outr[ns] = hr.y;
          outh[ns] = h;
        }
        ++ns;
        for (uint32_t k = nch; k-- > 0;) {
          const uint2 cr = k < 4 ? (k == 0 ? c[0] : k == 1 ? c[1] : k == 2 ? c[2] : c[3]) : st[(size_t)(h + 1 + k) * 64];
          FSTACK_PUSH(cr.y | cold)
        }
      } else {
        uint32_t pick = 0;
        if (EXT) {  // temperature 1 throughout (the host picks this instantiation only then)
          const uint32_t me = hr.x & 0xfffffu;
          const double inv = 1.0 / ins[(size_t)me * 64];
          const int ne = ine[(size_t)me * 64];
          double choice = gibbs_uniform(A.seed, A.iter, forest, step++);
          for (uint32_t k = 0;; ++k) {
            pick = k;
            const uint2 cr = k < 4 ? (k == 0 ? c[0] : k == 1 ? c[1] : k == 2 ? c[2] : c[3]) : st[(size_t)(h + 1 + k) * 64];
            const uint32_t ci = cr.x & F_IDX;
            choice -= ldexp(ins[(size_t)ci * 64] * inv, ine[(size_t)ci * 64] - ne);
            if (choice < 0 || k + 1 == nch) break;
          }
        } else {
        const double power = cold ? 1.0 : A.power;
        // at temperature 1 the normaliser is the node's own inside value: the same fold over the same children
        double norm = ins[(size_t)(hr.x & 0xfffffu) * 64];
        if (power != 1.0) {
          norm = F_NEG_INF;
          for (uint32_t k = 0; k < nch; ++k) {
            const uint2 cr = k < 4 ? (k == 0 ? c[0] : k == 1 ? c[1] : k == 2 ? c[2] : c[3]) : st[(size_t)(h + 1 + k) * 64];
            norm = f_lwadd(norm, ins[(size_t)(cr.x & F_IDX) * 64] * power);
          }
        }
        double choice = gibbs_uniform(A.seed, A.iter, forest, step++);
        for (uint32_t k = 0;; ++k) {
          pick = k;
          const uint2 cr = k < 4 ? (k == 0 ? c[0] : k == 1 ? c[1] : k == 2 ? c[2] : c[3]) : st[(size_t)(h + 1 + k) * 64];
          choice -= exp(ins[(size_t)(cr.x & F_IDX) * 64] * power - norm);
          if (choice < 0 || k + 1 == nch) break;
        }
        }
        const uint2 cr = pick < 4 ? (pick == 0 ? c[0] : pick == 1 ? c[1] : pick == 2 ? c[2] : c[3]) : st[(size_t)(h + 1 + pick) * 64];
        FSTACK_PUSH(cr.y | cold)
      }
    }
#undef FSTACK_PUSH
    A.sample_len[forest] = ns < max_sample ? ns : max_sample;
  }
  if (A.trace) {
    tr3 = __builtin_readcyclecounter();
    unsigned long long t3 = tr3;
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = __shfl_down(t3, o, 64);
      t3 = other > t3 ? other : t3;
    }
    if (lane == 0) {
      unsigned long long* o = A.trace + (size_t)(A.first_group + blockIdx.x) * 8;
      o[0] = tr0; o[1] = tr0; o[2] = tr2; o[3] = t3; o[4] = __builtin_readcyclecounter(); o[5] = g.maxlen; o[6] = g.n_lanes;
    }
  }
}

// ---- several lanes per forest (parallel sweep, temperature 1) ----
// forest_sample_kernel is one forest per lane: a forest's inside values take a column of LDS per lane (40-110 KB per wave on
// config 5: two or three waves per CU, nobody to hide a wave's dependent LDS round trips behind) and a sweep costs what its
// slowest lane costs.  Here a forest gets FM_G lanes (FM_FPW = 64 / FM_G forests per wavefront) and a few hundred bytes of
// LDS: its tables (children lists, node order by HEIGHT) are copied in once, the inside pass goes height by height with the
// lanes over the nodes of a height (a node's children are all of lower height), and the walk is breadth-first: the lanes
// take the entries of the current frontier, an OR entry chooses one child, an AND entry records its rule and hands on all of
// its children; slots in the next frontier and in the sample come from a prefix sum over the lanes (no atomics: the order is
// the same in every run).  Arithmetic is forest_sample_kernel's EXT form (mantissa x 2^exponent).  ONE difference in the
// chain: the sequential walk draws its uniforms by the ORDER OF VISITS of a depth-first walk, which a breadth-first walk
// does not have -- the uniform of a visit is keyed by its position in the breadth-first order instead.  Every visit still has
// a uniform of its own (a shared sub-forest expanded twice chooses twice): the same kind of chain -- the stale-count sweep of
// forest-em.hpp:750-766 with other random numbers -- validated against the sweep's enumerated stationary distribution
// (tests/test_bench_workloads_gpu.py) instead of draw for draw.
__device__ __forceinline__ uint32_t fm_prefix(uint32_t v, uint32_t li, uint32_t& total) {
  // exclusive prefix sum over the FM_G lanes of a forest; total = the sum
  uint32_t x = v;
#pragma unroll
  for (int d = 1; d < FM_G; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, FM_G);
    if (li >= (uint32_t)d) x += y;
  }
  total = __shfl(x, FM_G - 1, FM_G);
  return x - v;
}
#define FM_EBIAS 2048
#if FM_G == 8
#define FM_TQ 4  // 16-byte pieces of the forest's table per lane in the first round of loads (x FM_G lanes x 8 words)
#define FM_SC 4  // class words of the previous sample per lane ...
#define FM_HR 8  // header rows per lane ...
#else
#define FM_TQ 8
#define FM_SC 8
#define FM_HR 12
#endif
#define FM_KP 4  // children of a node whose values the inside pass requests before it folds them
__global__ __launch_bounds__(64) void forest_sample_multi_kernel(ForestArgs A, FMultiArgs M, uint32_t max_sample) {
  extern __shared__ __attribute__((aligned(16))) double fm_lds[];
  const uint32_t sub = threadIdx.x / FM_G, li = threadIdx.x % FM_G;
  const unsigned long long tr0 = A.trace ? __builtin_readcyclecounter() : 0;
  unsigned long long tr1 = 0, tr2 = 0, tr3 = 0;
  const uint32_t slot = M.lane_lo + blockIdx.x * FM_FPW + sub;
  const uint32_t forest = slot < M.lane_hi ? A.lane_forest[slot] : 0xffffffffu;  // (rides along with the descriptor's loads)
  const bool active = forest != 0xffffffffu;
  // this forest's stretch of LDS: mantissas (f64), exponents (i32), header words (u32: row of the node's header record | the
  // exponent of an AND node's proposal probability + FM_EBIAS, bits 16..30 | bit 31 = AND), table + two frontiers (u16)
  const size_t per = (size_t)M.max_n * 16 + (((size_t)M.max_tab + 2 * (size_t)M.max_front) * 2 + 15) / 16 * 16;
  char* mine = (char*)fm_lds + per * sub;
  double* vm = (double*)mine;
  int* ve = (int*)(vm + M.max_n);
  uint32_t* hd = (uint32_t*)(ve + M.max_n);
  unsigned short* tb = (unsigned short*)(hd + M.max_n);
  unsigned short* fr0 = tb + M.max_tab;
  unsigned short* fr1 = fr0 + M.max_front;
  // ---- staging: three rounds of loads.  (1) the slot's descriptor; (2) the forest's tables (16 bytes a load), the length
  // and the first FM_SC x FM_G class words of its previous sample, the header rows of its first FM_HR x FM_G nodes; (3) the
  // snapshot counts of those rows' rules.  Forests with more nodes / longer samples continue in loops afterwards.
  const FGroup g = A.groups[active ? slot / 64 : M.lane_lo / 64];
  const uint32_t lane = slot % 64;
  uint4 d0 = make_uint4(0, 0, 0, 0), d1 = make_uint4(0, 0, 0, 0);
  if (active) {
    d0 = M.slots[2 * (size_t)slot];
    d1 = M.slots[2 * (size_t)slot + 1];
  }
  const uint32_t n = d1.w & 0x7fffu, words = d1.w >> 15;
  const unsigned short* __restrict__ src = M.tab + (((uint64_t)d0.y << 32) | d0.x);
  const uint4* __restrict__ hs = (const uint4*)(M.hdr + (((uint64_t)d0.w << 32) | d0.z));
  const uint32_t* __restrict__ sc = A.sample_cls + (((uint64_t)d1.y << 32) | d1.x);
  double* __restrict__ recp0 = A.rec_p + g.stream_base + lane;
  const bool own = M.own_proposal != 0;
  double* __restrict__ probp = M.prob + ((((uint64_t)d0.w << 32) | d0.z) >> 2);
  uint32_t plen = 0;
  uint32_t scq[FM_SC];
  uint4 hq[FM_HR];
  double sx[FM_HR], sn[FM_HR];
  {
    const uint4* __restrict__ s4 = (const uint4*)src;
    uint4* t4 = (uint4*)tb;
    const uint32_t w4 = (words + 7) / 8;
    uint4 tq[FM_TQ];
#pragma unroll
    for (int q = 0; q < FM_TQ; ++q) tq[q] = li + q * FM_G < w4 ? s4[li + q * FM_G] : make_uint4(0, 0, 0, 0);
    if (active && own) plen = A.old_len[forest];
#pragma unroll
    for (int q = 0; q < FM_SC; ++q) scq[q] = (active && own) ? sc[li + q * FM_G] : 0xffffffffu;  // (read past the sample: its capacity, or the padding)
#pragma unroll
    for (int q = 0; q < FM_HR; ++q) hq[q] = li + q * FM_G < n ? hs[li + q * FM_G] : make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int q = 0; q < FM_TQ; ++q)
      if (li + q * FM_G < w4) t4[li + q * FM_G] = tq[q];
    for (uint32_t k = li + FM_TQ * FM_G; k < w4; k += FM_G) t4[k] = s4[k];  // (tables beyond FM_TQ x FM_G x 8 words)
    if (own)
      for (uint32_t k = li; k < n; k += FM_G) ve[k] = 0;
    // round three: what the rows' probabilities need from the snapshot (or the probabilities themselves)
#pragma unroll
    for (int q = 0; q < FM_HR; ++q) {
      const uint4 h = hq[q];
      sx[q] = 0.0;
      sn[q] = 1.0;
      if (h.x & 0x80000000u) {
        if (!own)
          sx[q] = recp0[(size_t)(h.x & 0x7fffffffu) * 64];
        else if (h.w == F_NONORM)
          sx[q] = A.p_prior[h.y];
        else {
          sx[q] = A.snap_x[h.y];
          sn[q] = A.snap_norm[h.w];
        }
      }
    }
  }
  __syncthreads();
  if (active && own) {
    // how often the forest's previous sample uses each of its rule classes (low half) and norm-group classes (high half):
    // one pass over the sample's class words (forest_proposal_kernel scans them per rule); the exponents' rows hold the
    // counts until the inside pass writes them
#define FM_HIST(wd)                                                                                          \
  if ((wd) != 0xffffffffu) { /* (0xffffffff: a rule outside the normalisation groups) */                    \
    __hip_atomic_fetch_add(&ve[(wd) & 0xffffu], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);          \
    __hip_atomic_fetch_add(&ve[(wd) >> 16], 0x10000, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);        \
  }
#pragma unroll
    for (int q = 0; q < FM_SC; ++q)
      if (li + q * FM_G < plen) FM_HIST(scq[q])
    for (uint32_t j = li + FM_SC * FM_G; j < plen; j += FM_G) {
      const uint32_t wd = sc[j];
      FM_HIST(wd)
    }
#undef FM_HIST
  }
  __syncthreads();
  const uint32_t H = active ? tb[1] : 0u;
  if (active) {
    // an AND node's row: its proposal probability -- forest_proposal_kernel's (count - own uses) / (norm sum - own uses of the
    // group) -- as the mantissa where the node's value will be and the exponent in the header word (the exponents' rows
    // still hold the histogram); the recount reads the sampled rules' probabilities from rec_p
#define FM_ROW(k, hh, px, pn)                                                                                 \
  {                                                                                                          \
    uint32_t hw = (hh).x;                                                                                     \
    if (own) hw &= 0x80000000u; /* (the row of the header record: the one-per-lane kernels' business; here: a counter) */ \
    if (hw & 0x80000000u) {                                                                                  \
      double pr = (px);                                                                                       \
      if (own) {                                                                                             \
        if ((hh).w != F_NONORM) {                                                                             \
          const uint32_t own_r = (uint32_t)ve[(hh).z & 0xffffu] & 0xffffu, own_n = (uint32_t)ve[(hh).z >> 16] >> 16; \
          pr = ((px) - (double)own_r) / ((pn) - (double)own_n);                                              \
        }                                                                                                    \
        probp[k] = pr;                                                                                       \
      }                                                                                                      \
      int e;                                                                                                 \
      vm[k] = frexp(pr, &e);                                                                                 \
      hw |= (uint32_t)(e + FM_EBIAS) << 16;                                                                  \
    }                                                                                                        \
    hd[k] = hw;                                                                                              \
  }
#pragma unroll
    for (int q = 0; q < FM_HR; ++q)
      if (li + q * FM_G < n) FM_ROW(li + q * FM_G, hq[q], sx[q], sn[q])
    for (uint32_t k = li + FM_HR * FM_G; k < n; k += FM_G) {  // (forests beyond FM_HR x FM_G nodes: two more rounds)
      const uint4 h = hs[k];
      double x = 0.0, nrm = 1.0;
      if (h.x & 0x80000000u) {
        if (!own)
          x = recp0[(size_t)(h.x & 0x7fffffffu) * 64];
        else if (h.w == F_NONORM)
          x = A.p_prior[h.y];
        else {
          x = A.snap_x[h.y];
          nrm = A.snap_norm[h.w];
        }
      }
      FM_ROW(k, h, x, nrm)
    }
#undef FM_ROW
  }
  __syncthreads();
  if (A.trace) tr1 = __builtin_readcyclecounter();
  const unsigned short* lvl = tb + 4;
  const unsigned short* koff = lvl + H + 1;
  const unsigned short* kids = koff + n + 1;
  // ---- inside, height by height (forest.hpp:768-816 with the proposal probabilities) ----
  uint32_t Hmax = H;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) Hmax = max(Hmax, (uint32_t)__shfl_xor((int)Hmax, o, 64));
  for (uint32_t h = 0; h < Hmax; ++h) {
    if (h < H)
      for (uint32_t node = lvl[h] + li; node < lvl[h + 1]; node += FM_G) {  // (the nodes of a height: a range of ids)
        const uint32_t hw = hd[node], k0 = koff[node], k1 = koff[node + 1];
        // the first FM_KP children's values are requested together, before the fold (which is a chain): one LDS round trip
        // for the ids, one for the values, instead of two per child
        uint32_t cq[FM_KP];
        double mq[FM_KP];
        int eq[FM_KP];
#pragma unroll
        for (int i = 0; i < FM_KP; ++i) cq[i] = k0 + i < k1 ? (uint32_t)(kids[k0 + i] & 0x7fffu) : node;
#pragma unroll
        for (int i = 0; i < FM_KP; ++i) {
          mq[i] = vm[cq[i]];
          eq[i] = ve[cq[i]];
        }
        double m;
        int e;
        if (hw & 0x80000000u) {  // AND: its rule's proposal probability times its children
          m = vm[node];
          e = (int)((hw >> 16) & 0x7fffu) - FM_EBIAS;
#define FM_AND_FOLD(cm, ce)   \
  {                           \
    int t;                    \
    m = frexp(m * (cm), &t);  \
    e += (ce) + t;            \
  }
#pragma unroll
          for (int i = 0; i < FM_KP; ++i)
            if (k0 + i < k1) FM_AND_FOLD(mq[i], eq[i])
          for (uint32_t k = k0 + FM_KP; k < k1; ++k) {
            const uint32_t c = kids[k] & 0x7fffu;
            FM_AND_FOLD(vm[c], ve[c])
          }
#undef FM_AND_FOLD
        } else {  // OR: the sum of its children, aligned to the larger exponent
          m = 0.0;
          e = 0;
#define FM_OR_FOLD(cm_, ce_)                      \
  {                                               \
    const double cm = (cm_);                      \
    const int ce = (ce_);                         \
    if (cm != 0.0) {                              \
      if (m == 0.0) {                             \
        m = cm;                                   \
        e = ce;                                   \
      } else {                                    \
        const int dd = ce - e;                    \
        int t;                                    \
        if (dd <= 0)                              \
          m = frexp(m + ldexp(cm, dd), &t);       \
        else {                                    \
          m = frexp(ldexp(m, -dd) + cm, &t);      \
          e = ce;                                 \
        }                                         \
        e += t;                                   \
      }                                           \
    }                                             \
  }
#pragma unroll
          for (int i = 0; i < FM_KP; ++i)
            if (k0 + i < k1) FM_OR_FOLD(mq[i], eq[i])
          for (uint32_t k = k0 + FM_KP; k < k1; ++k) {
            const uint32_t c = kids[k] & 0x7fffu;
            FM_OR_FOLD(vm[c], ve[c])
          }
#undef FM_OR_FOLD
        }
        vm[node] = m;
        ve[node] = e;
      }
    __syncthreads();
  }
  if (A.trace) tr2 = __builtin_readcyclecounter();
  // ---- the walk, breadth first (forest.hpp:725-758) ----
  uint32_t nfr = active ? 1u : 0u, ns = 0, visited = 0;
  if (active && li == 0) fr0[0] = (unsigned short)(n - 1);
  __syncthreads();
  uint32_t* outh = active ? A.sample_hdr + A.sample_off[forest] : nullptr;
  unsigned short* cur = fr0;
  unsigned short* nxt = fr1;
  for (;;) {
    if (!__any(nfr != 0)) break;
    uint32_t nn = 0;  // entries of the next frontier so far
    for (uint32_t base = 0; __any(base < nfr); base += FM_G) {
      const uint32_t idx = base + li;
      const bool have = idx < nfr;
      uint32_t push = 0, rec = 0, node = 0, k0 = 0, pick = 0;
      bool is_and = false;
      if (have) {
        node = cur[idx] & 0x7fffu;
        const uint32_t hw = hd[node];
        k0 = koff[node];
        const uint32_t nch = koff[node + 1] - k0;
        is_and = (hw & 0x80000000u) != 0;
        if (is_and) {
          rec = 1;
          push = nch;
        } else if (nch) {
          // the reference's serial subtraction: the first child whose share takes the choice below zero, or the last
          // (the first FM_KP children's values requested together, as in the inside pass; the same differences in the same order)
          uint32_t cq[FM_KP];
          double mq[FM_KP];
          int eq[FM_KP];
#pragma unroll
          for (int i = 0; i < FM_KP; ++i) cq[i] = (uint32_t)i < nch ? (uint32_t)(kids[k0 + i] & 0x7fffu) : node;
#pragma unroll
          for (int i = 0; i < FM_KP; ++i) {
            mq[i] = vm[cq[i]];
            eq[i] = ve[cq[i]];
          }
          const int ne = ve[node];
          double choice = gibbs_uniform(A.seed, A.iter, forest, visited + idx) * vm[node];
          bool done = false;
#pragma unroll
          for (int i = 0; i < FM_KP; ++i)
            if (!done && (uint32_t)i < nch) {
              pick = (uint32_t)i;
              choice -= ldexp(mq[i], eq[i] - ne);
              done = choice < 0 || (uint32_t)i + 1 == nch;
            }
          for (uint32_t k = FM_KP; !done; ++k) {
            pick = k;
            const uint32_t c = kids[k0 + k] & 0x7fffu;
            choice -= ldexp(vm[c], ve[c] - ne);
            done = choice < 0 || k + 1 == nch;
          }
          push = 1;
        }
      }
      uint32_t tot_push, tot_rec;
      const uint32_t at = fm_prefix(push, li, tot_push), ar = fm_prefix(rec, li, tot_rec);
      if (have) {
        if (is_and) {
          if (ns + ar < max_sample) {
            outh[ns + ar] = own ? node : (hd[node] & 0xffffu);
            if (own && M.node_cnt) __hip_atomic_fetch_add(&hd[node], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
          }
          for (uint32_t k = 0; k < push; ++k)
            if (nn + at + k < M.max_front) nxt[nn + at + k] = kids[k0 + k];
        } else if (push) {
          if (nn + at < M.max_front) nxt[nn + at] = kids[k0 + pick];
        }
      }
      nn += tot_push;
      ns += tot_rec;
    }
    visited += nfr;
    __syncthreads();
    nfr = nn < M.max_front ? nn : M.max_front;
    unsigned short* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (active && li == 0) A.sample_len[forest] = ns < max_sample ? ns : max_sample;
  if (own && M.node_cnt && active) {  // every node of the forest says how often it was recorded (most: not at all)
    uint16_t* __restrict__ nc = M.node_cnt + ((((uint64_t)d0.w << 32) | d0.z) >> 2);
    for (uint32_t k = li; k < n; k += FM_G) nc[k] = (uint16_t)(hd[k] & 0xffffu);
  }
  if (A.trace) {
    tr3 = __builtin_readcyclecounter();
    uint32_t nmax = n, hmax = H, vmax = visited;
    for (int o = 32; o > 0; o >>= 1) {
      nmax = max(nmax, (uint32_t)__shfl_xor((int)nmax, o, 64));
      hmax = max(hmax, (uint32_t)__shfl_xor((int)hmax, o, 64));
      vmax = max(vmax, (uint32_t)__shfl_xor((int)vmax, o, 64));
    }
    if (threadIdx.x == 0) {
      unsigned long long* o = A.trace + ((size_t)M.lane_lo / FM_FPW + blockIdx.x) * 8;
      o[0] = tr0; o[1] = tr1; o[2] = tr2; o[3] = tr3; o[4] = tr3; o[5] = nmax; o[6] = hmax; o[7] = vmax;
    }
  }
}

// Viterbi (forest.hpp:507-632): max-product inside -- an AND node is its rule's weight times its children, an OR node
// keeps its FIRST best child (a later child must be strictly better, forest.hpp:547) -- and the best derivation walked
// from the root, recorded in pre-order as {rule, number of children} per AND node (what write_viterbi_rec prints).  One
// lane per forest over the same record streams as the E-step; GCOL: the column in global memory (forests beyond LDS).
template <bool GCOL>
__global__ __launch_bounds__(64) void forest_viterbi_kernel(ForestArgs A, uint32_t max_sample, uint32_t ins_rows,
                                                             uint32_t stack_lds, double* best_logprob) {
  extern __shared__ __attribute__((aligned(16))) double lds_all[];
  double* colbase = GCOL ? A.gcol + (size_t)blockIdx.x * A.gcol_stride : lds_all;
  double* aux = GCOL ? lds_all : lds_all + (size_t)ins_rows * 64;
  const FGroup g = A.groups[A.first_group + blockIdx.x];
  const int lane = threadIdx.x;
  if ((uint32_t)lane >= g.n_lanes) return;
  const uint32_t n = A.lane_nodes[g.lane_base + lane];
  const uint32_t forest = A.lane_forest[g.lane_base + lane];
  double* ins = colbase + lane;
  const uint2* __restrict__ st = A.ins_stream + g.stream_base + lane;
  {
    uint32_t d = 0;
    bool is_and = false, first = true;
    double acc = 0.0, best = F_NEG_INF;
    for (uint32_t k = 0; k < g.maxlen; ++k) {
      const uint2 r = st[(size_t)k * 64];
      if (!(r.x & F_VALID)) continue;
      if (r.x & F_HEADER) {
        is_and = (r.x & F_AND) != 0;
        acc = is_and ? A.rule_logw[r.y] : 0.0;
        best = F_NEG_INF;
        first = true;
      } else {
        const double v = ins[(size_t)(r.x & F_IDX) * 64];
        if (is_and)
          acc += v;
        else if (first || best < v)
          best = v;
        first = false;
      }
      if (r.x & F_LAST) {
        ins[(size_t)d * 64] = is_and ? acc : best;
        ++d;
      }
    }
  }
  best_logprob[forest] = ins[(size_t)(n - 1) * 64];
  const uint32_t* __restrict__ hp = A.hdr_pos + g.stream_base + lane;
  uint32_t* outr = A.sample_rules + A.sample_off[forest];
  uint32_t* outa = A.sample_hdr + A.sample_off[forest];
  const uint32_t cap = (uint32_t)(A.sample_off[forest + 1] - A.sample_off[forest]);
  uint32_t* stack = outr + cap;  // deep part of the stack: stack[-1 - i]
  uint32_t* stk_sh = (uint32_t*)aux + lane;
#define FSTACK_PUSH(v)                                       \
  {                                                          \
    if (sp < stack_lds)                                      \
      stk_sh[(size_t)sp * 64] = (v);                         \
    else                                                     \
      stack[-(int)(sp - stack_lds) - 1] = (v);               \
    ++sp;                                                    \
  }
  uint32_t sp = 0, ns = 0;
  FSTACK_PUSH(n - 1)
  while (sp) {
    --sp;
    const uint32_t node = sp < stack_lds ? stk_sh[(size_t)sp * 64] : stack[-(int)(sp - stack_lds) - 1];
    const uint32_t h = hp[(size_t)node * 64];
    const uint2 hr = st[(size_t)h * 64];
    uint32_t nch = (hr.x >> 20) & 0xffu;
    if (nch == 255u) {
      nch = 0;
      for (uint32_t k = h + 1;; ++k) {
        ++nch;
        if (st[(size_t)k * 64].x & F_LAST) break;
      }
    }
    if (hr.x & F_AND) {
      if (ns < max_sample) {
        outr[ns] = hr.y;
        outa[ns] = nch;
      }
      ++ns;
      for (uint32_t k = nch; k-- > 0;) FSTACK_PUSH(st[(size_t)(h + 1 + k) * 64].x & F_IDX)
    } else {
      uint32_t pick = 0;
      double best = ins[(size_t)(st[(size_t)(h + 1) * 64].x & F_IDX) * 64];
      for (uint32_t k = 1; k < nch; ++k) {
        const double v = ins[(size_t)(st[(size_t)(h + 1 + k) * 64].x & F_IDX) * 64];
        if (best < v) {
          best = v;
          pick = k;
        }
      }
      FSTACK_PUSH(st[(size_t)(h + 1 + pick) * 64].x & F_IDX)
    }
  }
#undef FSTACK_PUSH
  A.sample_len[forest] = ns < max_sample ? ns : max_sample;
}

// counts of a sweep's samples: x[rule] += 1, normsum[group] += 1 per use (the caller starts from the priors).
// A popular rule is used by a large share of the forests (the rule ids of real grammars, and of config 5, are Zipf
// distributed) and adds to one address serialise (~9 ns each: 10^5 uses of one rule = 1 ms), so a workgroup first
// counts in two LDS tables (slot = hash of the id, claimed by the first id that arrives; an id that finds its
// slot taken by another goes straight to global memory) and adds each claimed slot to global memory once.
// First formulation: 16 lanes per forest, a workgroup covers 64 forests at a time.  Second formulation (sweep2): the
// entries of 256 forests dealt out evenly; it also writes the sample's rule ids and class words (from the records at
// the positions the sampler left) and adds up the sample's ln proposal probability.
#define FRC_FORESTS 256u
__global__ __launch_bounds__(1024) void forest_recount_kernel(const uint64_t* sample_off, const uint32_t* sample_len,
                                                              uint32_t* rules, const uint32_t* p_norm, double* x,
                                                              double* normsum, uint32_t n_forests, ForestArgs A, int sweep2,
                                                              const uint32_t* slot_forest, uint32_t slot0, uint32_t slot1,
                                                              uint32_t n_slots0, uint32_t n_slots1, const uint32_t* node_hdr,
                                                              const double* node_prob, const uint4* node_slots) {
  // the two tables in dynamic LDS: n_slots0 {key, count} pairs for rules, n_slots1 for norm groups (powers of two)
  extern __shared__ uint32_t frc_lds[];
  uint32_t* const key0 = frc_lds;
  uint32_t* const cnt0 = key0 + n_slots0;
  uint32_t* const key1 = cnt0 + n_slots0;
  uint32_t* const cnt1 = key1 + n_slots1;
  __shared__ double cheap_sh[16];
  const bool count_here = !(sweep2 & 2);  // (bit 1: the counts are gathered from the nodes' use counts, forest_rule_gather_kernel)
  for (uint32_t i = threadIdx.x; i < n_slots0 && count_here; i += 1024) {
    key0[i] = 0xffffffffu;
    cnt0[i] = 0u;
  }
  for (uint32_t i = threadIdx.x; i < n_slots1 && count_here; i += 1024) {
    key1[i] = 0xffffffffu;
    cnt1[i] = 0u;
  }
  __syncthreads();
  auto add = [&](int t, uint32_t id, double* g) {
    if (!count_here) return;
    uint32_t* const key = t ? key1 : key0;
    uint32_t* const cnt = t ? cnt1 : cnt0;
    const uint32_t slot = (id * 2654435761u >> 9) & ((t ? n_slots1 : n_slots0) - 1);
    const uint32_t old = atomicCAS(&key[slot], 0xffffffffu, id);
    if (old == 0xffffffffu || old == id)
      atomicAdd(&cnt[slot], 1u);
    else
      unsafeAtomicAdd(g + id, 1.0);
  };
  double cheap = 0.0;
  // slot_forest: the forests of the lane slots [slot0, slot1) -- one launch class, recounted as soon as its sample kernel is
  // done, beside the other classes still sampling; otherwise all forests in corpus order
  const uint32_t i_begin = slot_forest ? slot0 : 0u, i_end = slot_forest ? slot1 : n_forests;
  if (sweep2) {
    // The entries of FRC_FORESTS forests at a time, dealt out evenly: a prefix sum of the sample lengths in LDS, entry e
    // belongs to the forest whose range holds it (binary search).  (Sixteen lanes per forest, forest after forest, left
    // a workgroup waiting for its largest sample four times in a row: 75-110 us for the classes of large forests.)
    __shared__ uint32_t pre[FRC_FORESTS + 1];
    __shared__ uint32_t fid[FRC_FORESTS];
    __shared__ uint32_t nbase[FRC_FORESTS];  // node_hdr: the forest's first node in node_hdr / node_prob
    for (uint32_t f0 = i_begin + blockIdx.x * FRC_FORESTS; f0 < i_end; f0 += gridDim.x * FRC_FORESTS) {
      __syncthreads();
      if (threadIdx.x < FRC_FORESTS) {
        const uint32_t i = f0 + threadIdx.x;
        const uint32_t f = i < i_end ? (slot_forest ? slot_forest[i] : i) : 0xffffffffu;
        fid[threadIdx.x] = f;
        pre[threadIdx.x + 1] = f == 0xffffffffu ? 0u : sample_len[f];
        if (node_hdr && f != 0xffffffffu) {
          const uint4 d0 = node_slots[2 * (size_t)(slot_forest ? i : A.lane_of_forest[f])];
          nbase[threadIdx.x] = (uint32_t)(((((uint64_t)d0.w) << 32) | d0.z) >> 2);
        }
      }
      if (threadIdx.x == 0) pre[0] = 0;
      __syncthreads();
      for (uint32_t o = 1; o < FRC_FORESTS; o <<= 1) {  // inclusive scan of pre[1 ..]
        uint32_t v = 0;
        if (threadIdx.x < FRC_FORESTS && threadIdx.x >= o) v = pre[threadIdx.x + 1 - o];
        __syncthreads();
        if (threadIdx.x < FRC_FORESTS) pre[threadIdx.x + 1] += v;
        __syncthreads();
      }
      const uint32_t total = pre[FRC_FORESTS];
      if (node_hdr) {
        // the sampler wrote NODE numbers: a sampled rule's id, class word and norm group are one 16-byte record of the forest's
        // header table, its probability one double beside it -- the forest's own lines, fetched once for all its entries
        for (uint32_t e0 = threadIdx.x; e0 < total; e0 += 4 * 1024) {
          size_t so[4];
          uint32_t nd[4];
          uint4 h[4];
          double pv[4];
          bool ok[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const uint32_t e = e0 + 1024u * q;
            ok[q] = e < total;
            uint32_t lo = 0, hi = FRC_FORESTS;
            while (hi - lo > 1) {
              const uint32_t mid = (lo + hi) >> 1;
              if (pre[mid] <= (ok[q] ? e : 0u))
                lo = mid;
              else
                hi = mid;
            }
            so[q] = ok[q] ? sample_off[fid[lo]] + (e - pre[lo]) : 0u;
            nd[q] = ok[q] ? nbase[lo] : 0u;
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) nd[q] += ok[q] ? A.sample_hdr[so[q]] : 0u;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            h[q] = ((const uint4*)node_hdr)[nd[q]];
            pv[q] = node_prob[nd[q]];
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (!ok[q]) continue;
            rules[so[q]] = h[q].y;
            A.sample_cls[so[q]] = h[q].w == F_NONORM ? 0xffffffffu : h[q].z;
            cheap += log(pv[q]);
            if (h[q].w == F_NONORM) continue;
            add(0, h[q].y, x);
            add(1, h[q].w, normsum);
          }
        }
      } else
      for (uint32_t e0 = threadIdx.x; e0 < total; e0 += 4 * 1024) {  // four entries per thread in flight
        size_t pos[4], so[4];
        uint32_t rule[4], nn[4], c[4];
        double lpv[4];
        bool ok[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint32_t e = e0 + 1024u * q;
          ok[q] = e < total;
          uint32_t lo = 0, hi = FRC_FORESTS;  // the last forest slot whose range starts at or before e
          while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (pre[mid] <= (ok[q] ? e : 0u))
              lo = mid;
            else
              hi = mid;
          }
          const uint32_t f = ok[q] ? fid[lo] : 0u;  // (a range that holds an entry belongs to a real forest)
          const uint32_t slot = ok[q] ? (slot_forest ? f0 + lo : A.lane_of_forest[f]) : 0u;
          const FGroup g = A.groups[slot >> 6];
          so[q] = sample_off[f] + (ok[q] ? e - pre[lo] : 0u);
          pos[q] = g.stream_base + (slot & 63u);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) pos[q] += (size_t)(ok[q] ? A.sample_hdr[so[q]] : 0u) * 64;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          rule[q] = A.ins_stream[pos[q]].y;
          lpv[q] = A.p_only ? A.rec_p[pos[q]] : A.rec_logp[pos[q]];
          c[q] = A.rec_cls[pos[q]];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) nn[q] = ok[q] ? p_norm[rule[q]] : F_NONORM;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (!ok[q]) continue;
          rules[so[q]] = rule[q];
          A.sample_cls[so[q]] = nn[q] == F_NONORM ? 0xffffffffu : c[q];
          cheap += A.p_only ? log(lpv[q]) : lpv[q];
          if (nn[q] == F_NONORM) continue;
          add(0, rule[q], x);
          add(1, nn[q], normsum);
        }
      }
    }
  } else
  for (uint32_t f0 = i_begin + blockIdx.x * 64; f0 < i_end; f0 += gridDim.x * 64) {
    const uint32_t i = f0 + (threadIdx.x >> 4);
    if (i >= i_end) continue;
    const uint32_t f = slot_forest ? slot_forest[i] : i;
    if (f == 0xffffffffu) continue;  // an empty lane slot
    const uint64_t so = sample_off[f];
    const uint32_t* r = rules + so;
    const uint32_t len = sample_len[f];
    for (uint32_t k = threadIdx.x & 15u; k < len; k += 16) {
      const uint32_t rule = r[k], nn = p_norm[rule];
      if (nn == F_NONORM) continue;
      add(0, rule, x);
      add(1, nn, normsum);
    }
  }
  if (sweep2) {
    for (int o = 32; o > 0; o >>= 1) cheap += __shfl_down(cheap, o, 64);
    if ((threadIdx.x & 63) == 0) cheap_sh[threadIdx.x >> 6] = cheap;
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n_slots0 && count_here; i += 1024)
    if (cnt0[i]) unsafeAtomicAdd(x + key0[i], (double)cnt0[i]);
  for (uint32_t i = threadIdx.x; i < n_slots1 && count_here; i += 1024)
    if (cnt1[i]) unsafeAtomicAdd(normsum + key1[i], (double)cnt1[i]);
  if (sweep2 && threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 16; ++i) t += cheap_sh[i];
    unsafeAtomicAdd(A.iter_out + 1, t);
  }
}
// ---- the parallel sweep's counts WITHOUT atomics (round 6).  The recount above ends in one device-scope atomic per distinct
// rule and norm group of every 256 forests -- ~4 M a sweep on config 5, most of them rules of the Zipf tail that no LDS table
// folds -- and those atomics, not its reads, are what it takes 85 us for.  But which nodes carry a rule never changes: the
// sampler leaves per node how often it recorded it (FMultiArgs::node_cnt, two bytes a node, every node written every sweep),
// and a rule's uses are the sum over ITS nodes (inv_off / inv_node, built with the forests): a gather through a static index,
// one thread a rule; rules on more than FRG_COLD nodes in pieces of FRG_PIECE, a workgroup each, added with integer atomics
// (a few hundred a sweep).  The norm groups' sums are sums over their rules' integers; both meet their priors in ONE rounding
// (prior + uses), whatever the order the samples came in -- the atomics' sums depended on it.
__global__ __launch_bounds__(256) void forest_rule_gather_kernel(const uint32_t* __restrict__ inv_off, const uint32_t* __restrict__ inv_node,
                                                                 const uint16_t* __restrict__ node_cnt, uint32_t* __restrict__ rule_cnt,
                                                                 uint32_t n_rules, const uint32_t* __restrict__ pieces, uint32_t n_pieces,
                                                                 uint32_t cold_blocks, uint32_t n_inv) {
  if (blockIdx.x >= cold_blocks) {  // four pieces a workgroup: {rule, first, end} each
    const uint32_t pc = (blockIdx.x - cold_blocks) * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (pc >= n_pieces) return;
    const uint32_t r = pieces[3 * pc], j0 = pieces[3 * pc + 1], j1 = pieces[3 * pc + 2];
    uint32_t nd[FRG_PIECE / 64], c = 0;
#pragma unroll
    for (int q = 0; q < (int)(FRG_PIECE / 64); ++q) nd[q] = j0 + lane + 64u * q < j1 ? inv_node[j0 + lane + 64u * q] : 0xffffffffu;
#pragma unroll
    for (int q = 0; q < (int)(FRG_PIECE / 64); ++q)
      if (nd[q] != 0xffffffffu) c += node_cnt[nd[q]];
    for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o, 64);
    if (lane == 0 && c) atomicAdd(rule_cnt + r, c);
    return;
  }
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rules) return;
  const uint32_t j0 = inv_off[r], j1 = inv_off[r + 1];
  if (j1 - j0 > FRG_COLD) return;  // (its pieces add into rule_cnt[r], zero since the last sweep's apply)
  if (j1 == j0) return;  // (a rule on no node: its count stays zero)
  uint32_t nd[FRG_COLD], c = 0;
#pragma unroll
  for (int q = 0; q < (int)FRG_COLD; ++q) nd[q] = j0 + (uint32_t)q < j1 ? inv_node[j0 + (uint32_t)q] : 0xffffffffu;
#pragma unroll
  for (int q = 0; q < (int)FRG_COLD; ++q)
    if (nd[q] != 0xffffffffu) c += node_cnt[nd[q]];
  rule_cnt[r] = c;
}
// the norm groups' sums from their rules' use counts (the rules' own new counts: forest_commit_kernel, in rule order).  Eight
// lanes a group (config 5: eight rules a group on average).
__global__ __launch_bounds__(256) void forest_group_sum_kernel(const uint64_t* __restrict__ group_off, const uint32_t* __restrict__ group_rule,
                                                               uint64_t n_groups, const uint32_t* __restrict__ rule_cnt,
                                                               const double* __restrict__ prior_norm, double* __restrict__ normsum) {
  const uint64_t g = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
  const uint32_t li = threadIdx.x & 7u;
  const bool on = g < n_groups;
  const uint64_t j0 = on ? group_off[g] : 0, j1 = on ? group_off[g + 1] : 0;
  uint32_t sum = 0;
  for (uint64_t j = j0 + li; j < j1; j += 8) sum += rule_cnt[group_rule[j]];
  sum += __shfl_xor(sum, 1, 8);
  sum += __shfl_xor(sum, 2, 8);
  sum += __shfl_xor(sum, 4, 8);
  if (on && li == 0) normsum[g] = prior_norm[g] + (double)sum;
}
// reset_x / reset_norm (may be null): the count buffers of the NEXT sweep start from the priors -- set here, by the thread
// that has just read the slot, instead of two copies behind the kernel
__global__ void forest_commit_kernel(double* new_x, double* p_x, double* p_s, double* p_tmax, const uint32_t* p_norm,
                                     double time, uint64_t n, const double* reset_x, double* next_norm,
                                     const double* reset_norm, uint64_t n_norm, uint32_t* rule_cnt = nullptr,
                                     const double* prior = nullptr) {
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_norm && next_norm;
       p += (uint64_t)gridDim.x * blockDim.x)
    next_norm[p] = reset_norm[p];
  for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (uint64_t)gridDim.x * blockDim.x) {
    if (p_norm[p] == F_NONORM) continue;
    double nx;
    if (rule_cnt) {  // the sweep's use counts, gathered (forest_rule_gather_kernel): the new count in one rounding; cleared for the next sweep
      nx = prior[p] + (double)rule_cnt[p];
      rule_cnt[p] = 0u;
    } else {
      nx = new_x[p];
      if (reset_x) new_x[p] = reset_x[p];
    }
    const double d = nx - p_x[p];
    const double moret = time - p_tmax[p];
    if (moret > 0) {
      p_tmax[p] = time;
      p_s[p] += moret * p_x[p];
    } else if (moret < 0)
      p_s[p] += d * (-moret);
    p_x[p] += d;
  }
}

// M-step (normalize.hpp:123-164): per group w = (count) / (sum + add_k); zero-count group -> uniform or zero
__global__ void forest_mstep_kernel(double* rule_logw, const double* counts, double prior, const uint64_t* group_off,
                                    const uint32_t* group_rule, uint64_t n_groups, double add_k, int zero_zero,
                                    unsigned long long* max_bits) {
  double mx = 0.0;
  for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t j0 = group_off[g], j1 = group_off[g + 1];
    double sum = 0.0;
    for (uint64_t j = j0; j < j1; ++j) sum += counts[group_rule[j]] + prior;
    for (uint64_t j = j0; j < j1; ++j) {
      const uint32_t r = group_rule[j];
      double nw;
      if (sum > 0.0) {
        const double c = counts[r] + prior;
        nw = c > 0.0 ? log(c / (sum + add_k)) : F_NEG_INF;
      } else
        nw = zero_zero ? F_NEG_INF : -log((double)(j1 - j0));
      mx = fmax(mx, fabs(exp(nw) - exp(rule_logw[r])));
      rule_logw[r] = nw;
    }
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_down(mx, o, 64));
  if ((threadIdx.x & 63) == 0 && mx > 0.0) atomicMax(max_bits, (unsigned long long)__double_as_longlong(mx));
}


// ---- dynamic LDS (forest.hpp) ----
bool forest_cols_exceed_lds(uint32_t max_nodes) { return forest_estimate_lds_bytes(max_nodes) > F_LDS_LIMIT; }
size_t forest_estimate_lds_bytes(uint32_t max_nodes) { return (size_t)max_nodes * 64 * sizeof(double) * 2; }
size_t forest_estimate_ext_lds_bytes(uint32_t max_nodes) { return (size_t)max_nodes * 64 * 24; }
FEstepKind forest_estep_kind(uint32_t max_nodes) {
  if (forest_cols_exceed_lds(max_nodes)) return F_ESTEP_GCOL;
  return forest_estimate_ext_lds_bytes(max_nodes) <= F_LDS_LIMIT ? F_ESTEP_EXT : F_ESTEP_LOG;
}
const char* forest_estep_kind_name(FEstepKind k) { return k == F_ESTEP_EXT ? "ext" : k == F_ESTEP_LOG ? "log" : "gcol"; }
size_t forest_gibbs_lds_bytes(bool gcol, uint32_t ins_rows, uint32_t own_cap, uint32_t stack_lds) {
  return (gcol ? 0 : (size_t)ins_rows * 64 * 8) + (size_t)own_cap * 64 * 4 + (size_t)stack_lds * 64 * 4;
}
size_t forest_sample_lds_bytes(uint32_t max_nodes, bool ext, uint32_t stack_lds) {
  return (size_t)max_nodes * 64 * (ext ? 12 : 8) + (size_t)stack_lds * 64 * 4;
}
size_t forest_sample_lw_lds_bytes(uint32_t max_nodes, bool ext, uint32_t kid_rows, uint32_t stack_lds) {
  return (size_t)max_nodes * 64 * (ext ? 12 : 8) + ((size_t)2 * max_nodes + 1 + kid_rows + stack_lds) * 64 * 2;
}
size_t forest_multi_lds_bytes(uint32_t max_n, uint32_t max_tab, uint32_t max_front) {
  return (size_t)max_n * 16 + (((size_t)max_tab + 2 * (size_t)max_front) * 2 + 15) / 16 * 16;
}

// ---- launchers (forest.hpp) ----
// a kernel that asks for more dynamic LDS than the default limit has the limit raised first
template <class K>
static void f_raise_lds(K kernel, size_t bytes) {
  if (bytes > 64 * 1024) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

hipError_t launch_forest_estimate(const ForestArgs& A, bool gcol, uint32_t n_groups, uint32_t max_nodes, hipStream_t s) {
  if (gcol)
    hipLaunchKernelGGL(forest_estimate_kernel<true>, dim3(n_groups), dim3(64), 0, s, A);
  else {
    const size_t lds = forest_estimate_lds_bytes(max_nodes);
    f_raise_lds(forest_estimate_kernel<false>, lds);
    hipLaunchKernelGGL(forest_estimate_kernel<false>, dim3(n_groups), dim3(64), lds, s, A);
  }
  return hipGetLastError();
}
hipError_t launch_forest_estimate_ext(const ForestArgs& A, uint32_t n_groups, uint32_t max_nodes, hipStream_t s) {
  const size_t lds = forest_estimate_ext_lds_bytes(max_nodes);
  f_raise_lds(forest_estimate_ext_kernel, lds);
  hipLaunchKernelGGL(forest_estimate_ext_kernel, dim3(n_groups), dim3(64), lds, s, A);
  return hipGetLastError();
}

hipError_t launch_forest_proposal(const ForestArgs& A, hipStream_t s) {
  if (!A.n_and) return hipSuccess;
  hipLaunchKernelGGL(forest_proposal_kernel, dim3((unsigned)((A.n_and + 255) / 256)), dim3(256), 0, s, A);
  return hipGetLastError();
}

template <bool GCOL, bool EXT, bool LW>
static hipError_t f_launch_sample(const ForestArgs& A, const FSampleLaunch& L, size_t bytes, hipStream_t s) {
  f_raise_lds(forest_sample_kernel<GCOL, EXT, LW>, bytes);
  hipLaunchKernelGGL((forest_sample_kernel<GCOL, EXT, LW>), dim3(L.n_groups), dim3(64), bytes, s, A, L.max_sample, L.max_nodes,
                     L.stack_lds, L.kid_rows);
  return hipGetLastError();
}
hipError_t launch_forest_sample(const ForestArgs& A, const FSampleLaunch& L, hipStream_t s) {
  if (L.gcol) {  // (the columns in global memory: LDS holds the stack only; no LW form)
    const size_t stk = (size_t)L.stack_lds * 64 * 4;
    return L.ext ? f_launch_sample<true, true, false>(A, L, stk, s) : f_launch_sample<true, false, false>(A, L, stk, s);
  }
  if (L.lw) {
    const size_t b = forest_sample_lw_lds_bytes(L.max_nodes, L.ext, L.kid_rows, L.stack_lds);
    return L.ext ? f_launch_sample<false, true, true>(A, L, b, s) : f_launch_sample<false, false, true>(A, L, b, s);
  }
  const size_t b = forest_sample_lds_bytes(L.max_nodes, L.ext, L.stack_lds);
  return L.ext ? f_launch_sample<false, true, false>(A, L, b, s) : f_launch_sample<false, false, false>(A, L, b, s);
}

hipError_t launch_forest_sample_multi(const ForestArgs& A, const FMultiArgs& M, uint32_t max_sample, hipStream_t s) {
  hipLaunchKernelGGL(forest_sample_multi_kernel, dim3(forest_multi_workgroups(M)), dim3(64),
                     forest_multi_lds_bytes(M.max_n, M.max_tab, M.max_front) * FM_FPW, s, A, M, max_sample);
  return hipGetLastError();
}

hipError_t launch_forest_gibbs(const ForestArgs& A, bool gcol, uint32_t n_groups, uint32_t max_sample, uint32_t ins_rows,
                               uint32_t own_cap, uint32_t stack_lds, hipStream_t s) {
  const size_t lds = forest_gibbs_lds_bytes(gcol, ins_rows, own_cap, stack_lds);
  if (gcol) {
    f_raise_lds(forest_gibbs_kernel<true>, lds);
    hipLaunchKernelGGL(forest_gibbs_kernel<true>, dim3(n_groups), dim3(64), lds, s, A, max_sample, ins_rows, own_cap, stack_lds);
  } else {
    f_raise_lds(forest_gibbs_kernel<false>, lds);
    hipLaunchKernelGGL(forest_gibbs_kernel<false>, dim3(n_groups), dim3(64), lds, s, A, max_sample, ins_rows, own_cap, stack_lds);
  }
  return hipGetLastError();
}

hipError_t launch_forest_viterbi(const ForestArgs& A, bool gcol, uint32_t n_groups, uint32_t max_sample, uint32_t max_nodes,
                                 uint32_t stack_lds, double* best_logprob, hipStream_t s) {
  const size_t col = (size_t)max_nodes * 64 * sizeof(double), stk = (size_t)stack_lds * 64 * 4;
  if (gcol)
    hipLaunchKernelGGL(forest_viterbi_kernel<true>, dim3(n_groups), dim3(64), stk, s, A, max_sample, max_nodes, stack_lds, best_logprob);
  else {
    f_raise_lds(forest_viterbi_kernel<false>, col + stk);
    hipLaunchKernelGGL(forest_viterbi_kernel<false>, dim3(n_groups), dim3(64), col + stk, s, A, max_sample, max_nodes, stack_lds,
                       best_logprob);
  }
  return hipGetLastError();
}

// the recount's LDS tables: rules / norm groups (powers of two)
static const uint32_t FRC_SLOTS0 = 8192, FRC_SLOTS1 = 4096;
static const size_t FRC_BYTES = (size_t)(FRC_SLOTS0 + FRC_SLOTS1) * 8;
// groups per workgroup of a class's recount (fewer groups per workgroup = more workgroups, each adding its share of
// the popular rules to the same addresses: 1 and 2 measured slower than 4, 122 and 84 against 77 us for the last class)
static const uint32_t FRC_GROUPS = 4;
hipError_t prepare_forest_recount() {
  return hipFuncSetAttribute((const void*)forest_recount_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FRC_BYTES);
}
hipError_t launch_forest_recount(const FRecount& R, const ForestArgs& A, hipStream_t s) {
  const unsigned grid = R.slot_forest ? std::min<uint32_t>(std::max<uint32_t>((R.slot1 - R.slot0) / 64 / FRC_GROUPS, 1u), 2048u)
                                      : (unsigned)std::min<uint64_t>(((uint64_t)R.n_forests + 255) / 256, 2048);
  hipLaunchKernelGGL(forest_recount_kernel, dim3(grid), dim3(1024), FRC_BYTES, s, R.sample_off, R.sample_len, R.rules, R.p_norm, R.x,
                     R.normsum, R.n_forests, A, R.sweep2, R.slot_forest, R.slot0, R.slot1, FRC_SLOTS0, FRC_SLOTS1, R.node_hdr,
                     R.node_prob, R.node_slots);
  return hipGetLastError();
}

hipError_t launch_forest_rule_gather(const uint32_t* inv_off, const uint32_t* inv_node, const uint16_t* node_cnt, uint32_t* rule_cnt,
                                     uint32_t n_rules, const uint32_t* pieces, uint32_t n_pieces, uint32_t n_inv, hipStream_t s) {
  const uint32_t cold_blocks = (n_rules + 255) / 256;  // a thread per rule, then four pieces a workgroup
  hipLaunchKernelGGL(forest_rule_gather_kernel, dim3(cold_blocks + (n_pieces + 3) / 4), dim3(256), 0, s, inv_off, inv_node, node_cnt,
                     rule_cnt, n_rules, pieces, n_pieces, cold_blocks, n_inv);
  return hipGetLastError();
}
hipError_t launch_forest_group_sum(const uint64_t* group_off, const uint32_t* group_rule, uint64_t n_groups, const uint32_t* rule_cnt,
                                   const double* prior_norm, double* normsum, hipStream_t s) {
  hipLaunchKernelGGL(forest_group_sum_kernel, dim3((unsigned)((n_groups * 8 + 255) / 256)), dim3(256), 0, s, group_off, group_rule,
                     n_groups, rule_cnt, prior_norm, normsum);
  return hipGetLastError();
}
hipError_t launch_forest_commit(const FCommit& C, hipStream_t s) {
  hipLaunchKernelGGL(forest_commit_kernel, dim3((unsigned)((C.n + 255) / 256)), dim3(256), 0, s, C.new_x, C.p_x, C.p_s, C.p_tmax,
                     C.p_norm, C.time, C.n, C.reset_x, C.next_norm, C.reset_norm, C.n_norm, C.rule_cnt, C.prior);
  return hipGetLastError();
}
hipError_t launch_forest_mstep(double* rule_logw, const double* counts, double prior, const uint64_t* group_off,
                               const uint32_t* group_rule, uint64_t n_groups, double add_k, int zero_zero,
                               unsigned long long* max_bits, hipStream_t s) {
  const unsigned grid = (unsigned)std::min<uint64_t>((n_groups + 255) / 256, 4096);
  hipLaunchKernelGGL(forest_mstep_kernel, dim3(grid), dim3(256), 0, s, rule_logw, counts, prior, group_off, group_rule, n_groups,
                     add_k, zero_zero, max_bits);
  return hipGetLastError();
}

}  // namespace carmel_hip
