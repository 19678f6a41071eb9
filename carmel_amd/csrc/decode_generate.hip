// decode_generate.hip — batch generation: random paths (carmel -G n: WFST::randomPath, fst.h:708-757, carmel.cc:1446-1458) and
// random input/output pairs (carmel -g n: WFST::generate, fst.cc:24-79, carmel.cc:1459-1482) drawn from the machine itself, where
// every other decoder entry point conditions on given lines.  A forward random walk over the whole machine: no trellis, no line.
//
// The rule (DESIGN.md section 7 and include/carmel_hip.h state it in the same words; tests/decode_generate_ref.py restates it).
// Arcs.  Only arcs of weight > 0 (log weight > -inf) exist for generation.
// Lists.  JOINT mode has one list per state: its arcs by arc id.  CONDITIONAL mode has one list per (state, matched-side symbol):
//   that group's arcs by arc id; a state's groups are in ascending symbol id, epsilon (0) first; the matched side is the handle's
//   `side`, so side 0 is carmel's -g.
// Cumulative values of a list w_0 .. w_{m-1}.  M = max w_k, p_k = exp(w_k - M) by the host's std::exp, cum_k = cum_{k-1} + p_k in
//   f64, in list order, S = cum_{m-1} (decode_generate_tables.cpp; the device computes no exp at all).
// Choice with a uniform u.  t = u S, one f64 multiply.  The arc is the first k with cum_k > t; if there is none, because t rounded
//   up to S, the first k with cum_k == S.  An arc whose p_k underflowed to 0 is therefore never chosen.  The device finds k by
//   bisection and never scans.
// Attempt a = 0, 1, ... of path P (its index in the stream: first_path + its index in the call).  Start with s = 0, n = 0, repeat:
//   1. if s is the final state, accept;
//   2. if n == max_arcs, or s has no list, reject;
//   3. choose an arc -- JOINT: u = gibbs_uniform(seed, a, P, n), chosen in s's list; CONDITIONAL: G the number of s's groups,
//      g = min(G - 1, floor(gibbs_uniform(seed, a, P, 2n) G)), the arc chosen in group g with gibbs_uniform(seed, a, P, 2n + 1);
//   4. append the arc, set s to its destination, increment n.
//   The final state is tested before the cap, so a path of exactly max_arcs arcs is accepted.  A rejected attempt is followed by
//   a + 1; after max_tries rejected attempts the path has failed.  A path depends on (machine, weights, side, mode, seed, P,
//   max_arcs) alone: not on chunking, launch order, the other paths, or how a stream is cut into calls.
// Reported weight.  As everywhere in the decoders, the path's arcs' logs added from the END, w1 + (w2 + (... + (wn + 0))); the
//   empty path has 0.0.
//
// decode_generate_walk_kernel<mode, kWrite>: one lane per path, 256 lanes a workgroup.  The counting pass runs the attempt loop and
// leaves per path the accepted attempt, the length and a failed flag; the writing pass replays only the accepted attempt, writes
// the arcs in path order and then adds the reported weight by reading its own path back from the end.  Nothing is indexed per
// lane at run time (no scratch), and a lane's work is bounded by the arguments (max_arcs max_tries <= 2^24 steps), so no kernel
// can run away on a cyclic machine: epsilon cycles and 00 cycles are legal here.
// Paths go in chunks of at most 2^22; a chunk's writing pass is cut so that its path buffer fits decode_chunk_bytes.  The results
// go to the handle's path store (kb_logw / kb_off / kb_arcs).  decode_collect_paths is not used: it files a trellis' (line, rank)
// slots and takes the weights from the counting walk, and here there are no lines and the weight comes with the writing pass.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "decode.hpp"
#include "engine.hpp"
#include "rng.hpp"

namespace {
constexpr uint64_t kChunkPaths = 1ull << 22;

// what the walk kernel takes beside the tables: the n paths of one launch, path idx of it being P = first + idx of the stream
struct GenerateWalk {
  uint32_t n, final_state, max_arcs, max_tries;
  uint64_t seed, first, n_arcs;
  uint32_t* attempt;         // [n]: the accepted attempt (counting pass: written; writing pass: read)
  uint32_t* len;             // [n]: its arcs
  uint8_t* failed;           // [n]: max_tries attempts were rejected
  const uint64_t* path_off;  // the writing pass: [n + 1]
  uint32_t* path;
  const double* a_w;         // every arc's weight, by arc id
  double* logw;              // [n]: the reported weight
  int* err;
};

// the arc of list g that the uniform u chooses -> its index in the list arrays (the list is not empty)
__device__ inline uint32_t generate_choose(const GenerateTables& G, uint32_t g, double u) {
  const uint32_t a0 = G.list_arc[g], a1 = G.list_arc[g + 1];
  const double S = G.cum[a1 - 1];
  const double t = u * S;
  uint32_t lo = a0, hi = a1;  // the first k with cum_k > t
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (G.cum[mid] > t)
      hi = mid;
    else
      lo = mid + 1;
  }
  if (lo == a1) {  // t rounded up to S: the first k with cum_k == S
    lo = a0;
    hi = a1 - 1;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (G.cum[mid] >= S)
        hi = mid;
      else
        lo = mid + 1;
    }
  }
  return lo;
}

// attempt a of path P -> accepted; n: its arcs (of the accepted or the rejected walk).  kWrite: the arcs go to out[0 .. cap), and
// a walk that would pass cap (the counting pass' length) is cut short and reported as rejected
template <int kMode, bool kWrite>
__device__ inline bool generate_attempt(const GenerateTables& G, const GenerateWalk& W, uint32_t a, uint32_t P, uint32_t cap,
                                        uint32_t* out, uint32_t& n) {
  uint32_t s = 0;
  n = 0;
  while (true) {
    if (s == W.final_state) return true;
    if (n == W.max_arcs) return false;
    uint32_t g;
    double u;
    if (kMode == CARMEL_HIP_GENERATE_JOINT) {
      g = s;
      if (G.list_arc[g] == G.list_arc[g + 1]) return false;  // a dead end
      u = gibbs_uniform(W.seed, a, P, n);
    } else {
      const uint32_t g0 = G.st_grp[s], n_grp = G.st_grp[s + 1] - g0;
      if (!n_grp) return false;
      const uint32_t pick = (uint32_t)(gibbs_uniform(W.seed, a, P, 2 * n) * (double)n_grp);
      g = g0 + (pick < n_grp - 1 ? pick : n_grp - 1);
      u = gibbs_uniform(W.seed, a, P, 2 * n + 1);
    }
    const uint32_t k = generate_choose(G, g, u);
    if (kWrite) {
      if (n >= cap) return false;
      out[n] = G.id[k];
    }
    s = G.dst[k];
    ++n;
  }
}

template <int kMode, bool kWrite>
__global__ void __launch_bounds__(256) decode_generate_walk_kernel(GenerateTables G, GenerateWalk W) {
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;  // (a launch has at most 2^22 paths)
  if (idx >= W.n) return;
  const uint32_t P = (uint32_t)(W.first + idx);  // (first_path + n_paths <= 2^32: the entry point has checked)
  uint32_t n = 0;
  if (!kWrite) {
    uint32_t a = 0;
    bool ok = false;
    for (; a < W.max_tries; ++a) {
      ok = generate_attempt<kMode, false>(G, W, a, P, 0, nullptr, n);
      if (ok) break;
    }
    W.attempt[idx] = ok ? a : W.max_tries - 1;
    W.len[idx] = ok ? n : 0;
    W.failed[idx] = ok ? 0 : 1;
    return;
  }
  const uint32_t cap = W.len[idx];
  uint32_t* out = W.path + W.path_off[idx];
  if (!generate_attempt<kMode, true>(G, W, W.attempt[idx], P, cap, out, n) || n != cap) {
    atomicOr(W.err, kErrWalk);  // (the replay is not the walk that was counted)
    return;
  }
  double w = 0.0;
  for (uint32_t k = cap; k-- > 0;) {
    const uint32_t arc = out[k];
    if (arc >= W.n_arcs) {
      atomicOr(W.err, kErrWalk);
      return;
    }
    w = W.a_w[arc] + w;
  }
  W.logw[idx] = w;
}

int upload_generate_tables(carmel_hip_decoder* d) {
  if (d->gen_ready) return CARMEL_HIP_OK;
  const GenerateTablesHost H = build_generate_tables(d->n_states, d->src, d->dst, d->msym, d->logw);  // (lives until the copies are made)
  hipStream_t s = d->stream;
  hipError_t err = hipSuccess;
  int n32 = 0, n64 = 0;
  auto up32 = [&](const std::vector<uint32_t>& v) {
    DevBuf<uint32_t>& b = d->gen_u32[n32++];
    if (err == hipSuccess) err = b.upload(v, s);
    return b.p;
  };
  auto up64 = [&](const std::vector<double>& v) {
    DevBuf<double>& b = d->gen_f64[n64++];
    if (err == hipSuccess) err = b.upload(v, s);
    return b.p;
  };
  d->GJ = GenerateTables{nullptr, up32(H.joint.list_arc), up32(H.joint.id), up32(H.joint.dst), up64(H.joint.cum)};
  d->GC = GenerateTables{up32(H.st_grp), up32(H.cond.list_arc), up32(H.cond.id), up32(H.cond.dst), up64(H.cond.cum)};
  if (err != hipSuccess) return fail(CARMEL_HIP_ERR_HIP, std::string("carmel_hip_decoder_generate: ") + hipGetErrorString(err));
  HIPCHK(hipStreamSynchronize(s));
  d->gen_ready = true;
  return CARMEL_HIP_OK;
}
}  // namespace

extern "C" {

int carmel_hip_decoder_generate(carmel_hip_decoder* d, int mode, uint64_t n_paths, uint64_t first_path, uint64_t seed,
                                uint32_t max_arcs, uint32_t max_tries, uint32_t* tries) {
  const std::string who = "carmel_hip_decoder_generate";
  if (!d) return fail(CARMEL_HIP_ERR_ARG, who + ": bad argument");
  if (mode != CARMEL_HIP_GENERATE_JOINT && mode != CARMEL_HIP_GENERATE_CONDITIONAL)
    return fail(CARMEL_HIP_ERR_ARG, who + ": mode must be CARMEL_HIP_GENERATE_JOINT or CARMEL_HIP_GENERATE_CONDITIONAL");
  if (n_paths > (1ull << 32) || first_path > (1ull << 32) - n_paths)
    return fail(CARMEL_HIP_ERR_ARG, who + ": first_path + n_paths must be at most 2^32");
  if (max_arcs < 1 || max_arcs > (1u << 20)) return fail(CARMEL_HIP_ERR_ARG, who + ": max_arcs must be in 1 .. 2^20");
  if (max_tries < 1 || max_tries > 65536) return fail(CARMEL_HIP_ERR_ARG, who + ": max_tries must be in 1 .. 65536");
  if ((uint64_t)max_arcs * max_tries > (1ull << 24)) return fail(CARMEL_HIP_ERR_ARG, who + ": max_arcs x max_tries must be at most 2^24");
  HIPCHK(hipSetDevice(d->device));
  if (const int rc = upload_generate_tables(d)) return rc;
  hipStream_t s = d->stream;
  uint64_t budget = 1ull << 30;
  if (const char* v = lib_opt("decode_chunk_bytes")) budget = std::max<uint64_t>(1, std::strtoull(v, nullptr, 10));
  const bool joint = mode == CARMEL_HIP_GENERATE_JOINT;
  const GenerateTables& G = joint ? d->GJ : d->GC;
  std::vector<double> r_logw(n_paths, 0.0);
  std::vector<uint64_t> r_off(n_paths + 1, 0);
  std::vector<uint32_t> r_arcs, r_tries(n_paths);
  DevBuf<uint32_t> d_attempt, d_len, d_path;
  DevBuf<uint8_t> d_failed;
  DevBuf<uint64_t> d_poff;
  DevBuf<double> d_logw;
  DevBuf<int> d_err;
  HIPCHK(d_err.alloc(1));
  DecodeChunk c{d};
  c.ms = 0;
  for (uint64_t lo = 0; lo < n_paths; lo += kChunkPaths) {
    const uint32_t n = (uint32_t)std::min(kChunkPaths, n_paths - lo);
    HIPCHK(d_attempt.alloc(n));
    HIPCHK(d_len.alloc(n));
    HIPCHK(d_failed.alloc(n));
    HIPCHK(d_logw.alloc(n));
    HIPCHK(hipMemsetAsync(d_err.p, 0, sizeof(int), s));
    // the paths [at, at + m) of the chunk, counting or writing
    auto walk = [&](bool write, uint32_t at, uint32_t m) {
      const GenerateWalk W{m, d->final_state, max_arcs, max_tries, seed, first_path + lo + at, d->n_arcs, d_attempt.p + at,
                           d_len.p + at, d_failed.p + at, d_poff.p, d_path.p, d->a_w.p, d_logw.p + at, d_err.p};
      const uint32_t wb = (m + 255) / 256;
      if (joint)
        (write ? decode_generate_walk_kernel<CARMEL_HIP_GENERATE_JOINT, true>
               : decode_generate_walk_kernel<CARMEL_HIP_GENERATE_JOINT, false>)<<<wb, 256, 0, s>>>(G, W);
      else
        (write ? decode_generate_walk_kernel<CARMEL_HIP_GENERATE_CONDITIONAL, true>
               : decode_generate_walk_kernel<CARMEL_HIP_GENERATE_CONDITIONAL, false>)<<<wb, 256, 0, s>>>(G, W);
    };
    if (const int rc = c.begin()) return rc;
    walk(false, 0, n);
    if (const int rc = c.end()) return rc;
    std::vector<uint32_t> attempt(n), len(n);
    std::vector<uint8_t> failed(n);
    HIPCHK(hipMemcpyAsync(attempt.data(), d_attempt.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(len.data(), d_len.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(failed.data(), d_failed.p, n * sizeof(uint8_t), hipMemcpyDeviceToHost, s));
    if (const int rc = c.wait()) return rc;
    for (uint32_t p = 0; p < n; ++p) {
      if (failed[p])
        return fail(CARMEL_HIP_ERR_STATE, who + ": path " + std::to_string(first_path + lo + p) + " did not reach the final state in " +
                                              std::to_string(max_tries) + " attempts (max_tries) of at most " +
                                              std::to_string(max_arcs) + " arcs (max_arcs)");
      if (len[p] > max_arcs || attempt[p] >= max_tries) return fail(CARMEL_HIP_ERR_STATE, who + ": inconsistent generation walk");
      r_tries[lo + p] = attempt[p] + 1;
      r_off[lo + p + 1] = r_off[lo + p] + len[p];
    }
    // the writing pass, in cuts of paths whose arcs fit the budget (a path longer than it goes alone)
    for (uint32_t at = 0; at < n;) {
      uint32_t m = 0;
      std::vector<uint64_t> h_poff(1, 0);
      while (at + m < n && (m == 0 || (h_poff[m] + len[at + m]) * sizeof(uint32_t) <= budget)) {
        h_poff.push_back(h_poff[m] + len[at + m]);
        ++m;
      }
      const uint64_t n_cut = h_poff[m], base = r_arcs.size();
      if (n_cut) {  // (a cut of empty paths alone: their weight is the 0.0 they were given)
        int err = 0;
        HIPCHK(d_poff.upload(h_poff, s));
        HIPCHK(d_path.alloc(n_cut));
        if (const int rc = c.begin()) return rc;
        walk(true, at, m);
        if (const int rc = c.end()) return rc;
        r_arcs.resize(base + n_cut);
        HIPCHK(hipMemcpyAsync(r_arcs.data() + base, d_path.p, n_cut * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(r_logw.data() + lo + at, d_logw.p + at, m * sizeof(double), hipMemcpyDeviceToHost, s));
        HIPCHK(hipMemcpyAsync(&err, d_err.p, sizeof(int), hipMemcpyDeviceToHost, s));
        if (const int rc = c.wait()) return rc;
        if (err) return fail(CARMEL_HIP_ERR_STATE, who + ": inconsistent generation walk");
      }
      at += m;
    }
  }
  d->kb_logw.swap(r_logw);
  d->kb_off.swap(r_off);
  d->kb_arcs.swap(r_arcs);
  d->last_ms = c.ms;
  if (tries && n_paths) std::memcpy(tries, r_tries.data(), n_paths * sizeof(uint32_t));
  return CARMEL_HIP_OK;
}

}  // extern "C"
