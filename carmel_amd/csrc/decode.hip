// decode.hip — batch 1-best decoding (carmel -b -k 1: print_kbest / visit_kbest(1, ...), carmel.cc:378-398, fst.h:791) of many
// lines against one (composed) transducer, on a tropical-semiring (max, +) trellis over (line position i, state q), f64 log
// weights.  The reference composes each line with the machine and runs a reversed Dijkstra over the result (kbest.h:189,
// graph.cc:148-208); here nothing is composed per line: a line only selects which arcs may advance a position.
//
// Line-independent preparation (carmel_hip_decoder_create, and again on carmel_hip_decoder_set_weights): the host builds the
// tables of decode_tables.hpp -- the matched arcs in a CSR by symbol, the epsilon arcs by levels, each by destination and by
// source, and the epsilon arcs once more by the levels of the 00 subgraph for the pair decoders -- and upload_tables below copies
// every one of them to the device as it is.  Arcs of weight zero are dropped there: they are never taken.
//
// Per line (one wavefront = one workgroup of 64 lanes per line; lines launched longest first):
//   d_0 = 0 at the start state (0), -inf elsewhere, closed over the epsilon arcs;
//   d_{i+1}[q'] = max over arcs q -> q' labelled x_i of d_i[q] + w, then closed over the epsilon arcs;
//   every (i, q') that is set or improved records the arc id in a back-pointer array of (n + 1) x |Q| u32.
// The trellis adds in path order from the start (0 + w1 + w2 + ...): that is how it CHOOSES the path.  The weight it REPORTS is
// the chosen path's arcs added from the end, w1 + (w2 + (... + (wn + 0))), summed by the walk that recovers the path: the
// reference's best_w is the distance its reversed Dijkstra computes from the final state (kbest.h:203-213 dist[src], graph.cc
// shortestPathTreeTo), and the summary line multiplies those.  (The two orders differ in the last bit for some lines; with path
// order the cipher run's product misses the trace's last printed digit.)  A path printed with its weight (no -W) carries the
// path-order sum (fst.h path_print: w *= arc.weight), which the front end adds up from the arcs.
//
// Tie rule (independent of lane count and scheduling): for a destination state the candidates are taken in arc-id order and
// only a STRICTLY greater value replaces the one held, so the lowest arc id among equal candidates wins; the epsilon closure
// that follows replaces a value only if it is strictly greater, so a matched arc beats an epsilon path of equal weight, and an
// epsilon path of more levels beats one of fewer only if strictly better.  (The reference keeps the first strict improvement in
// the pop order of its reversed Dijkstra; that rule is not replicated.)
//
// d_i and d_{i+1} are two rows of |Q| doubles: in LDS when 16 |Q| bytes fit 64 KiB (|Q| <= 4096), otherwise in a global scratch
// buffer per line (the "global tier": correct, not fast).  The back-pointers are walked afterwards by one lane per line
// (decode_paths.hip's decode_walk_kernel), once to count a path's arcs and once to write them in path order.
// The tables, the handle, the constants and the host drivers are in decode.hpp, shared with the k-best decoder
// (decode_kbest.hip) and the all-paths sum (decode_sum.hip); this kernel alone closes a cyclic epsilon subgraph.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <vector>
#include "decode.hpp"
#include "engine.hpp"

namespace {
// close `row` (position i's values) over the epsilon arcs; `bpr` is that position's back-pointer row
__device__ void eps_close(const DecodeTables& T, double* row, uint32_t* bpr, int lane, int* err) {
  if (!T.eps_cyclic) {
    for (uint32_t L = 0; L < T.n_levels; ++L) {
      for (uint32_t e = T.lvl_ent[L] + lane; e < T.lvl_ent[L + 1]; e += kLanes) {
        const uint32_t q = T.ent_dst[e];
        double best = row[q];
        uint32_t barc = kNone;
        for (uint32_t k = T.ent_arc[e]; k < T.ent_arc[e + 1]; ++k) {
          const double v = row[T.e_src[k]] + T.e_w[k];
          if (v > best) {
            best = v;
            barc = T.e_id[k];
          }
        }
        if (barc != kNone) {
          row[q] = best;
          bpr[q] = barc;
        }
      }
      __syncthreads();
    }
    return;
  }
  // a cyclic epsilon subgraph: Bellman-Ford in arc-id order on one lane, |Q| rounds at most; a change in round |Q| means a cycle
  // that strictly improves a path (kbest.h:160-166 best_path_has_cycle)
  if (lane == 0) {
    bool changed = true;
    for (uint32_t round = 0; changed && round <= T.n_states; ++round) {
      changed = false;
      for (uint32_t k = 0; k < T.n_eps; ++k) {
        const double v = row[T.e_src[k]] + T.e_w[k];
        const uint32_t q = T.e_dst[k];
        if (v > row[q]) {
          row[q] = v;
          bpr[q] = T.e_id[k];
          changed = true;
        }
      }
      if (changed && round == T.n_states) atomicOr(err, kErrCycle);
    }
  }
  __syncthreads();
}

template <bool kLds>
__global__ void __launch_bounds__(kLanes) decode_trellis_kernel(DecodeTables T, DecodeLines D, DecodePaths P) {
  extern __shared__ double lds_rows[];
  const int lane = threadIdx.x;
  const uint32_t line = D.order[blockIdx.x];
  const uint32_t Q = T.n_states;
  double* cur = kLds ? lds_rows : D.rows + (size_t)line * 2 * Q;
  double* nxt = cur + Q;
  const uint64_t s0 = D.off[line];
  const uint32_t n = (uint32_t)(D.off[line + 1] - s0);
  uint32_t* bp = P.bp_arc + P.bp_off[line];
  const double ninf = -std::numeric_limits<double>::infinity();
  for (uint32_t q = lane; q < Q; q += kLanes) {
    cur[q] = q == 0 ? 0.0 : ninf;
    bp[q] = kNone;
  }
  __syncthreads();
  eps_close(T, cur, bp, lane, P.err);
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t* bpn = bp + (size_t)(i + 1) * Q;
    for (uint32_t q = lane; q < Q; q += kLanes) {
      nxt[q] = ninf;
      bpn[q] = kNone;
    }
    __syncthreads();
    const uint32_t x = D.sym[s0 + i];
    if (x < T.n_syms)  // (a symbol no arc matches leaves the row at -inf: no derivation)
      for (uint32_t g = T.sym_seg[x] + lane; g < T.sym_seg[x + 1]; g += kLanes) {
        double best = ninf;
        uint32_t barc = kNone;
        for (uint32_t k = T.seg_arc[g]; k < T.seg_arc[g + 1]; ++k) {
          const double v = cur[T.m_src[k]] + T.m_w[k];
          if (v > best) {
            best = v;
            barc = T.m_id[k];
          }
        }
        if (barc != kNone) {
          const uint32_t q = T.seg_dst[g];
          nxt[q] = best;
          bpn[q] = barc;
        }
      }
    __syncthreads();
    eps_close(T, nxt, bpn, lane, P.err);
    double* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (lane == 0) P.n_paths[line] = cur[T.final_state] > ninf;
}
}  // namespace

void carmel_hip::launch_decode_trellis(const carmel_hip_decoder* d, bool lds, uint32_t n, const DecodeLines& L, const DecodePaths& P,
                                       hipStream_t s) {
  if (lds)
    decode_trellis_kernel<true><<<n, kLanes, 16 * (size_t)d->n_states, s>>>(d->T, L, P);
  else
    decode_trellis_kernel<false><<<n, kLanes, 0, s>>>(d->T, L, P);
}

int carmel_hip_decoder::upload_tables() {
  const DecodeTablesHost H = build_decode_tables(n_states, src, dst, msym, osym, logw);  // (lives until the copies have been made)
  eps_cyclic = H.eps_cyclic;
  pair_levels = H.pair_levels;
  pair_cycle = H.pair_cycle;
  tab_u32.clear();
  tab_f64.clear();
  tab_u8.clear();
  hipStream_t s = stream;
  hipError_t err = hipSuccess;
  // a table into a buffer of its own at the end of `pool` -> where it is on the device (nullptr: the table is empty)
  auto up = [&](auto& pool, const auto& v) {
    pool.emplace_back();
    if (err == hipSuccess) err = pool.back().upload(v, s);
    return pool.back().p;
  };
  T = DecodeTables{n_states, final_state, H.n_syms, up(tab_u32, H.m.sym_seg), up(tab_u32, H.m.seg_state), up(tab_u32, H.m.seg_arc),
                   up(tab_u32, H.m.other), up(tab_f64, H.m.w), up(tab_u32, H.m.id), H.e.n_levels, H.eps_cyclic ? 1 : 0,
                   up(tab_u32, H.e.lvl_ent), up(tab_u32, H.e.ent_state), up(tab_u32, H.e.ent_arc), up(tab_u32, H.e.other),
                   up(tab_u32, H.e_dst), up(tab_f64, H.e.w), up(tab_u32, H.e.id), H.n_eps, up(tab_u32, H.e.st_ent)};
  TO = DecodeOutTables{up(tab_u32, H.om.sym_seg), up(tab_u32, H.om.seg_state), up(tab_u32, H.om.seg_arc), up(tab_u32, H.om.other),
                       up(tab_f64, H.om.w), up(tab_u32, H.om.id), up(tab_u32, H.oe.lvl_ent), up(tab_u32, H.oe.ent_state),
                       up(tab_u32, H.oe.ent_arc), up(tab_u32, H.oe.other), up(tab_f64, H.oe.w), up(tab_u32, H.oe.id),
                       up(tab_u8, H.oe.has)};
  TP = DecodePairTables{up(tab_u32, H.m.osym), H.pe.n_levels, H.m.max_seg, up(tab_u32, H.pe.lvl_ent), up(tab_u32, H.pe.ent_state),
                        up(tab_u32, H.pe.ent_arc), up(tab_u32, H.pe.other), up(tab_f64, H.pe.w), up(tab_u32, H.pe.id),
                        up(tab_u32, H.pe.osym), up(tab_u32, H.pe.st_ent)};
  TPO = DecodePairOutTables{TO.sym_seg, TO.seg_src, TO.seg_arc, TO.m_dst, TO.m_w, TO.m_id, up(tab_u32, H.om.osym), H.poe.n_levels,
                            H.om.max_seg, up(tab_u32, H.poe.lvl_ent), up(tab_u32, H.poe.ent_state), up(tab_u32, H.poe.ent_arc),
                            up(tab_u32, H.poe.other), up(tab_f64, H.poe.w), up(tab_u32, H.poe.id), up(tab_u32, H.poe.osym),
                            up(tab_u8, H.poe.has)};
  if (err != hipSuccess) return fail(CARMEL_HIP_ERR_HIP, std::string("upload_tables: ") + hipGetErrorString(err));
  HIPCHK(a_src.upload(src, s));
  HIPCHK(a_w.upload(logw, s));
  HIPCHK(a_eps.upload(H.a_eps, s));
  HIPCHK(a_flags.upload(H.a_flags, s));
  HIPCHK(eps_in.upload(H.e.has, s));
  HIPCHK(hipStreamSynchronize(s));
  return CARMEL_HIP_OK;
}

extern "C" {

int carmel_hip_decoder_create(carmel_hip_decoder** out, int device, uint32_t n_states, uint32_t final_state, uint64_t n_arcs,
                              const uint32_t* src, const uint32_t* dst, const uint32_t* in_sym, const uint32_t* out_sym,
                              const double* logw, int side) {
  if (!out || !n_states || final_state >= n_states || (side != 0 && side != 1) || n_arcs >= kNone ||
      (n_arcs && (!src || !dst || !in_sym || !out_sym || !logw)))
    return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decoder_create: bad argument");
  for (uint64_t k = 0; k < n_arcs; ++k)
    if (src[k] >= n_states || dst[k] >= n_states) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decoder_create: arc state out of range");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(CARMEL_HIP_ERR_HIP, "no HIP device: decoding has no CPU fallback");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<carmel_hip_decoder> d(new carmel_hip_decoder());
  d->device = device;
  d->side = side;
  d->n_states = n_states;
  d->final_state = final_state;
  d->n_arcs = n_arcs;
  d->src.assign(src, src + n_arcs);
  d->dst.assign(dst, dst + n_arcs);
  d->msym.assign(side ? out_sym : in_sym, (side ? out_sym : in_sym) + n_arcs);  // -r: the machine inverted
  d->osym.assign(side ? in_sym : out_sym, (side ? in_sym : out_sym) + n_arcs);
  d->logw.assign(logw, logw + n_arcs);
  HIPCHK(hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreate(&d->ev0));
  HIPCHK(hipEventCreate(&d->ev1));
  const int rc = d->upload_tables();
  if (rc) return rc;
  *out = d.release();
  return CARMEL_HIP_OK;
}

int carmel_hip_decoder_set_weights(carmel_hip_decoder* d, const double* logw) {
  if (!d || (d->n_arcs && !logw)) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decoder_set_weights: bad argument");
  HIPCHK(hipSetDevice(d->device));
  d->logw.assign(logw, logw + d->n_arcs);
  d->gen_ready = false;  // (the generation tables hold the old weights' sums: the next carmel_hip_decoder_generate rebuilds them)
  d->bp_ready = false;   // (and the next carmel_hip_decoder_best_paths its own)
  d->pr_ready = false;   // (and the next carmel_hip_decoder_prune)
  d->ms_ready = false;   // (and the next carmel_hip_decoder_machine_sums)
  return d->upload_tables();  // (which arcs have weight zero may have changed)
}

int carmel_hip_decode(carmel_hip_decoder* d, uint64_t n_lines, const uint64_t* off, const uint32_t* sym, double* best_logw,
                      uint64_t* path_off) {
  if (!d || !off || !best_logw || !path_off || (off[n_lines] && !sym))
    return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decode: bad argument");
  if (const int rc = decode_check_lines("carmel_hip_decode", n_lines, off)) return rc;
  d->paths.clear();
  std::vector<uint64_t> line_paths(n_lines + 1), p_off;
  std::vector<double> p_logw;
  const int rc = decode_paths(d, "carmel_hip_decode", 1, false, launch_decode_trellis, n_lines, off, sym, line_paths.data(), p_logw,
                              p_off, d->paths);
  if (rc) return rc;
  path_off[0] = 0;
  for (uint64_t l = 0; l < n_lines; ++l) {  // a line has one path or none
    const uint64_t p = line_paths[l];
    best_logw[l] = line_paths[l + 1] > p ? p_logw[p] : -std::numeric_limits<double>::infinity();
    path_off[l + 1] = p_off[line_paths[l + 1]];
  }
  return CARMEL_HIP_OK;
}

int carmel_hip_decoder_get_paths(carmel_hip_decoder* d, uint32_t* arcs) {
  if (!d || (!arcs && !d->paths.empty())) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decoder_get_paths: bad argument");
  if (!d->paths.empty()) std::memcpy(arcs, d->paths.data(), d->paths.size() * sizeof(uint32_t));
  return CARMEL_HIP_OK;
}

int carmel_hip_decoder_last_ms(carmel_hip_decoder* d, double* kernel_ms) {
  if (!d || !kernel_ms) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decoder_last_ms: bad argument");
  *kernel_ms = d->last_ms;
  return CARMEL_HIP_OK;
}

int carmel_hip_decoder_destroy(carmel_hip_decoder* d) {
  if (d) {
    (void)hipSetDevice(d->device);
    delete d;
  }
  return CARMEL_HIP_OK;
}

}  // extern "C"
