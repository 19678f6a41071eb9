// decode.hip — batch 1-best decoding (carmel -b -k 1: print_kbest / visit_kbest(1, ...), carmel.cc:378-398, fst.h:791) of many
// lines against one (composed) transducer, on a tropical-semiring (max, +) trellis over (line position i, state q), f64 log
// weights.  The reference composes each line with the machine and runs a reversed Dijkstra over the result (kbest.h:189,
// graph.cc:148-208); here nothing is composed per line: a line only selects which arcs may advance a position.
//
// Line-independent preparation (carmel_hip_decoder_create, on the host, uploaded once):
//   * the matched arcs (the matched side -- input, or output for side 1 -- is not *e*) in a CSR by symbol, each symbol's arcs
//     sorted by (dst, arc id) and cut into one segment per destination state;
//   * the epsilon arcs (matched side *e*) grouped into levels: level(q) = 1 + the largest level of an epsilon predecessor of q
//     (0 without one), an arc filed under the level of its destination.  If the epsilon subgraph has a cycle there are no
//     levels: the closure relaxes every epsilon arc in arc-id order, round after round, to a fixed point (at most |Q| rounds).
//   Arcs of weight zero are dropped here: they are never taken.
//   * for the pair decoder (decode_pairs.hip, DecodePairTables): the other side's symbol of every arc, and the epsilon arcs by the
//     levels of the subgraph of the arcs with epsilon on BOTH sides, which exist also when the levels above do not;
//   * the same arcs filed under their SOURCES (DecodeOutTables, for the backward pass of decode_posterior.hip): matched arcs by
//     (symbol, src, arc id), one segment per source; epsilon arcs by (level of src, src, arc id), one entry per source.
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
#include <algorithm>
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
  const double ninf = -std::numeric_limits<double>::infinity();
  const uint32_t Q = n_states;
  std::vector<uint32_t> matched, eps;
  uint32_t n_syms = 0;
  for (uint64_t k = 0; k < n_arcs; ++k) {
    if (!(logw[k] > ninf)) continue;  // zero-probability arcs are never taken
    if (msym[k] == 0)
      eps.push_back((uint32_t)k);
    else {
      matched.push_back((uint32_t)k);
      n_syms = std::max(n_syms, msym[k] + 1);
    }
  }
  // matched arcs: CSR by symbol, (symbol, dst, arc id) order, one segment per (symbol, dst)
  std::stable_sort(matched.begin(), matched.end(), [&](uint32_t a, uint32_t b) {
    return msym[a] != msym[b] ? msym[a] < msym[b] : dst[a] < dst[b];
  });
  std::vector<uint32_t> h_sym_seg(n_syms + 1, 0), h_seg_dst, h_seg_arc, h_msrc, h_mid;
  std::vector<double> h_mw;
  for (size_t j = 0; j < matched.size(); ++j) {
    const uint32_t k = matched[j];
    if (j == 0 || msym[k] != msym[matched[j - 1]] || dst[k] != dst[matched[j - 1]]) {
      h_seg_dst.push_back(dst[k]);
      h_seg_arc.push_back((uint32_t)j);
      h_sym_seg[msym[k] + 1]++;
    }
    h_msrc.push_back(src[k]);
    h_mw.push_back(logw[k]);
    h_mid.push_back(k);
  }
  h_seg_arc.push_back((uint32_t)matched.size());
  for (uint32_t x = 0; x < n_syms; ++x) h_sym_seg[x + 1] += h_sym_seg[x];
  // epsilon arcs: levels of a topological order (Kahn), or one list in arc-id order if the subgraph is cyclic
  std::vector<uint32_t> level(Q, 0), indeg(Q, 0);
  std::vector<std::vector<uint32_t> > outs(Q);
  for (uint32_t k : eps) {
    outs[src[k]].push_back(k);
    indeg[dst[k]]++;
  }
  std::vector<uint32_t> work;
  for (uint32_t q = 0; q < Q; ++q)
    if (!indeg[q]) work.push_back(q);
  size_t seen = 0;
  uint32_t n_levels = 0;
  while (seen < work.size()) {
    const uint32_t q = work[seen++];
    for (uint32_t k : outs[q]) {
      level[dst[k]] = std::max(level[dst[k]], level[q] + 1);
      n_levels = std::max(n_levels, level[dst[k]]);
      if (--indeg[dst[k]] == 0) work.push_back(dst[k]);
    }
  }
  eps_cyclic = seen < Q;
  std::vector<uint32_t> h_lvl_ent, h_ent_dst, h_ent_arc, h_esrc, h_edst, h_eid;
  std::vector<double> h_ew;
  if (eps_cyclic)
    n_levels = 0;  // eps stays in arc-id order
  else {
    std::stable_sort(eps.begin(), eps.end(), [&](uint32_t a, uint32_t b) {
      return level[dst[a]] != level[dst[b]] ? level[dst[a]] < level[dst[b]] : dst[a] < dst[b];
    });
    // levels 1 .. n_levels hold arcs (level 0 states have no epsilon predecessor)
    h_lvl_ent.assign(n_levels + 1, 0);
    for (size_t j = 0; j < eps.size(); ++j) {
      const uint32_t k = eps[j];
      if (j == 0 || dst[k] != dst[eps[j - 1]]) {
        h_ent_dst.push_back(dst[k]);
        h_ent_arc.push_back((uint32_t)j);
        h_lvl_ent[level[dst[k]]]++;  // (level >= 1: counted into slot level - 1 + 1)
      }
    }
    h_ent_arc.push_back((uint32_t)eps.size());
    for (uint32_t L = 0; L < n_levels; ++L) h_lvl_ent[L + 1] += h_lvl_ent[L];
  }
  std::vector<uint32_t> h_stent(Q, kNone);  // the sampler's walk finds a state's epsilon arcs through its entry
  for (size_t e = 0; e < h_ent_dst.size(); ++e) h_stent[h_ent_dst[e]] = (uint32_t)e;
  for (uint32_t k : eps) {
    h_esrc.push_back(src[k]);
    h_edst.push_back(dst[k]);
    h_ew.push_back(logw[k]);
    h_eid.push_back(k);
  }
  std::vector<uint8_t> h_aeps(n_arcs);
  for (uint64_t k = 0; k < n_arcs; ++k) h_aeps[k] = msym[k] == 0;
  std::vector<uint8_t> h_epsin(Q, 0);
  for (uint32_t k : eps) h_epsin[dst[k]] = 1;
  // the outgoing view (DecodeOutTables): matched arcs by (symbol, src, arc id), one segment per (symbol, src); epsilon arcs by
  // (level of src, src, arc id), one entry per source -- the same arcs, the same levels
  std::vector<uint32_t> omatched(matched), oeps;
  std::sort(omatched.begin(), omatched.end(), [&](uint32_t a, uint32_t b) {
    return msym[a] != msym[b] ? msym[a] < msym[b] : src[a] != src[b] ? src[a] < src[b] : a < b;
  });
  std::vector<uint32_t> h_osym_seg(n_syms + 1, 0), h_oseg_src, h_oseg_arc, h_omdst, h_omid;
  std::vector<double> h_omw;
  for (size_t j = 0; j < omatched.size(); ++j) {
    const uint32_t k = omatched[j];
    if (j == 0 || msym[k] != msym[omatched[j - 1]] || src[k] != src[omatched[j - 1]]) {
      h_oseg_src.push_back(src[k]);
      h_oseg_arc.push_back((uint32_t)j);
      h_osym_seg[msym[k] + 1]++;
    }
    h_omdst.push_back(dst[k]);
    h_omw.push_back(logw[k]);
    h_omid.push_back(k);
  }
  h_oseg_arc.push_back((uint32_t)omatched.size());
  for (uint32_t x = 0; x < n_syms; ++x) h_osym_seg[x + 1] += h_osym_seg[x];
  std::vector<uint32_t> h_olvl_ent(n_levels + 1, 0), h_oent_src, h_oent_arc, h_oedst, h_oeid, h_ostent(Q, kNone);
  std::vector<double> h_oew;
  std::vector<uint8_t> h_epsout(Q, 0);
  if (!eps_cyclic) {
    oeps = eps;
    std::sort(oeps.begin(), oeps.end(), [&](uint32_t a, uint32_t b) {
      return level[src[a]] != level[src[b]] ? level[src[a]] < level[src[b]] : src[a] != src[b] ? src[a] < src[b] : a < b;
    });
  }
  for (size_t j = 0; j < oeps.size(); ++j) {
    const uint32_t k = oeps[j];
    if (j == 0 || src[k] != src[oeps[j - 1]]) {
      h_ostent[src[k]] = (uint32_t)h_oent_src.size();
      h_oent_src.push_back(src[k]);
      h_oent_arc.push_back((uint32_t)j);
      h_olvl_ent[level[src[k]] + 1]++;  // (a source's level is below its destinations': at most n_levels - 1)
    }
    h_oedst.push_back(dst[k]);
    h_oew.push_back(logw[k]);
    h_oeid.push_back(k);
    h_epsout[src[k]] = 1;
  }
  h_oent_arc.push_back((uint32_t)oeps.size());
  for (uint32_t L = 0; L < n_levels; ++L) h_olvl_ent[L + 1] += h_olvl_ent[L];
  // the pair decoder's tables (DecodePairTables): the other side's symbols, and the epsilon arcs by the levels of the 00 subgraph
  // alone (Kahn again, over the arcs with epsilon on both sides); from the epsilon arcs in arc-id order, never from the levels above
  std::vector<uint32_t> h_mosym, peps, plevel(Q, 0), pindeg(Q, 0), h_plvl_ent, h_pent_dst, h_pent_arc, h_pesrc, h_peid, h_peosym;
  std::vector<double> h_pew;
  for (uint32_t k : matched) h_mosym.push_back(osym[k]);
  uint32_t max_seg = 0;
  for (uint32_t x = 0; x < n_syms; ++x) max_seg = std::max(max_seg, h_sym_seg[x + 1] - h_sym_seg[x]);
  for (uint64_t k = 0; k < n_arcs; ++k)
    if (logw[k] > ninf && msym[k] == 0) peps.push_back((uint32_t)k);
  std::vector<std::vector<uint32_t> > pouts(Q);
  for (uint32_t k : peps)
    if (osym[k] == 0) {
      pouts[src[k]].push_back(k);
      pindeg[dst[k]]++;
    }
  work.clear();
  for (uint32_t q = 0; q < Q; ++q)
    if (!pindeg[q]) work.push_back(q);
  pair_levels = 0;
  for (seen = 0; seen < work.size();) {
    const uint32_t q = work[seen++];
    for (uint32_t k : pouts[q]) {
      plevel[dst[k]] = std::max(plevel[dst[k]], plevel[q] + 1);
      pair_levels = std::max(pair_levels, plevel[dst[k]]);
      if (--pindeg[dst[k]] == 0) work.push_back(dst[k]);
    }
  }
  pair_cycle.clear();
  if (seen < Q) {  // name one cycle: from a state Kahn left, step to a predecessor it left too until a state repeats
    std::vector<uint32_t> pred(Q, kNone), mark(Q, kNone);
    for (uint32_t k : peps)
      if (osym[k] == 0 && pindeg[src[k]] && pindeg[dst[k]] && pred[dst[k]] == kNone) pred[dst[k]] = src[k];
    uint32_t q = 0;
    while (!pindeg[q]) ++q;
    uint32_t step = 0;
    for (; mark[q] == kNone; q = pred[q]) mark[q] = step++;
    std::string names = std::to_string(q);
    for (uint32_t r = pred[q]; r != q; r = pred[r]) names = std::to_string(r) + " -> " + names;
    pair_cycle = "states " + std::to_string(q) + " -> " + names;
    pair_levels = 0;
  } else {
    std::stable_sort(peps.begin(), peps.end(), [&](uint32_t a, uint32_t b) {
      return plevel[dst[a]] != plevel[dst[b]] ? plevel[dst[a]] < plevel[dst[b]] : dst[a] < dst[b];
    });
    h_plvl_ent.assign(peps.empty() ? 1 : pair_levels + 2, 0);
    for (size_t j = 0; j < peps.size(); ++j) {
      const uint32_t k = peps[j];
      if (j == 0 || dst[k] != dst[peps[j - 1]]) {
        h_pent_dst.push_back(dst[k]);
        h_pent_arc.push_back((uint32_t)j);
        h_plvl_ent[plevel[dst[k]] + 1]++;
      }
      h_pesrc.push_back(src[k]);
      h_pew.push_back(logw[k]);
      h_peid.push_back(k);
      h_peosym.push_back(osym[k]);
    }
    h_pent_arc.push_back((uint32_t)peps.size());
    for (size_t L = 0; L + 1 < h_plvl_ent.size(); ++L) h_plvl_ent[L + 1] += h_plvl_ent[L];
  }
  if (h_plvl_ent.empty()) h_plvl_ent.assign(1, 0);
  std::vector<uint32_t> h_pstent(Q, kNone);  // the pair sampler's walk finds a state's matched-side-epsilon arcs through its entry
  for (size_t e = 0; e < h_pent_dst.size(); ++e) h_pstent[h_pent_dst[e]] = (uint32_t)e;
  // their outgoing view (DecodePairOutTables): the other side's symbols beside the outgoing matched CSR above, and the same
  // epsilon arcs by (00 level of the source, source, arc id), one entry per source; nothing if the 00 arcs have a cycle
  std::vector<uint32_t> h_omosym, poeps, h_polvl_ent(1, 0), h_poent_src, h_poent_arc, h_poedst, h_poeid, h_poeosym;
  std::vector<double> h_poew;
  std::vector<uint8_t> h_poepsout(Q, 0);
  for (uint32_t k : omatched) h_omosym.push_back(osym[k]);
  uint32_t max_oseg = 0;
  for (uint32_t x = 0; x < n_syms; ++x) max_oseg = std::max(max_oseg, h_osym_seg[x + 1] - h_osym_seg[x]);
  if (pair_cycle.empty() && !peps.empty()) {
    poeps = peps;
    std::sort(poeps.begin(), poeps.end(), [&](uint32_t a, uint32_t b) {
      return plevel[src[a]] != plevel[src[b]] ? plevel[src[a]] < plevel[src[b]] : src[a] != src[b] ? src[a] < src[b] : a < b;
    });
    h_polvl_ent.assign(pair_levels + 2, 0);
    for (size_t j = 0; j < poeps.size(); ++j) {
      const uint32_t k = poeps[j];
      if (j == 0 || src[k] != src[poeps[j - 1]]) {
        h_poent_src.push_back(src[k]);
        h_poent_arc.push_back((uint32_t)j);
        h_polvl_ent[plevel[src[k]] + 1]++;
      }
      h_poedst.push_back(dst[k]);
      h_poew.push_back(logw[k]);
      h_poeid.push_back(k);
      h_poeosym.push_back(osym[k]);
      h_poepsout[src[k]] = 1;
    }
    for (size_t L = 0; L + 1 < h_polvl_ent.size(); ++L) h_polvl_ent[L + 1] += h_polvl_ent[L];
  }
  h_poent_arc.push_back((uint32_t)poeps.size());
  std::vector<uint8_t> h_aflags(n_arcs);
  for (uint64_t k = 0; k < n_arcs; ++k) h_aflags[k] = (msym[k] != 0 ? 1 : 0) | (osym[k] != 0 ? 2 : 0);
  hipStream_t s = stream;
  HIPCHK(p_m_osym.upload(h_mosym, s));
  HIPCHK(p_lvl_ent.upload(h_plvl_ent, s));
  HIPCHK(p_ent_dst.upload(h_pent_dst, s));
  HIPCHK(p_ent_arc.upload(h_pent_arc, s));
  HIPCHK(p_e_src.upload(h_pesrc, s));
  HIPCHK(p_e_w.upload(h_pew, s));
  HIPCHK(p_e_id.upload(h_peid, s));
  HIPCHK(p_e_osym.upload(h_peosym, s));
  HIPCHK(p_st_ent.upload(h_pstent, s));
  HIPCHK(a_flags.upload(h_aflags, s));
  HIPCHK(po_m_osym.upload(h_omosym, s));
  HIPCHK(po_lvl_ent.upload(h_polvl_ent, s));
  HIPCHK(po_ent_src.upload(h_poent_src, s));
  HIPCHK(po_ent_arc.upload(h_poent_arc, s));
  HIPCHK(po_e_dst.upload(h_poedst, s));
  HIPCHK(po_e_w.upload(h_poew, s));
  HIPCHK(po_e_id.upload(h_poeid, s));
  HIPCHK(po_e_osym.upload(h_poeosym, s));
  HIPCHK(po_eps_out.upload(h_poepsout, s));
  HIPCHK(sym_seg.upload(h_sym_seg, s));
  HIPCHK(seg_dst.upload(h_seg_dst, s));
  HIPCHK(seg_arc.upload(h_seg_arc, s));
  HIPCHK(m_src.upload(h_msrc, s));
  HIPCHK(m_w.upload(h_mw, s));
  HIPCHK(m_id.upload(h_mid, s));
  HIPCHK(lvl_ent.upload(h_lvl_ent, s));
  HIPCHK(ent_dst.upload(h_ent_dst, s));
  HIPCHK(ent_arc.upload(h_ent_arc, s));
  HIPCHK(e_src.upload(h_esrc, s));
  HIPCHK(e_dst.upload(h_edst, s));
  HIPCHK(e_w.upload(h_ew, s));
  HIPCHK(e_id.upload(h_eid, s));
  HIPCHK(a_src.upload(src, s));
  HIPCHK(a_w.upload(logw, s));
  HIPCHK(a_eps.upload(h_aeps, s));
  HIPCHK(eps_in.upload(h_epsin, s));
  HIPCHK(st_ent.upload(h_stent, s));
  HIPCHK(o_sym_seg.upload(h_osym_seg, s));
  HIPCHK(o_seg_src.upload(h_oseg_src, s));
  HIPCHK(o_seg_arc.upload(h_oseg_arc, s));
  HIPCHK(o_m_dst.upload(h_omdst, s));
  HIPCHK(o_m_w.upload(h_omw, s));
  HIPCHK(o_m_id.upload(h_omid, s));
  HIPCHK(o_lvl_ent.upload(h_olvl_ent, s));
  HIPCHK(o_ent_src.upload(h_oent_src, s));
  HIPCHK(o_ent_arc.upload(h_oent_arc, s));
  HIPCHK(o_e_dst.upload(h_oedst, s));
  HIPCHK(o_e_w.upload(h_oew, s));
  HIPCHK(o_e_id.upload(h_oeid, s));
  HIPCHK(eps_out.upload(h_epsout, s));
  HIPCHK(o_st_ent.upload(h_ostent, s));
  HIPCHK(hipStreamSynchronize(s));
  TO = DecodeOutTables{o_sym_seg.p, o_seg_src.p, o_seg_arc.p, o_m_dst.p, o_m_w.p,  o_m_id.p,  o_lvl_ent.p,
                       o_ent_src.p, o_ent_arc.p, o_e_dst.p,   o_e_w.p,   o_e_id.p, eps_out.p, o_st_ent.p};
  TP = DecodePairTables{p_m_osym.p, (uint32_t)h_plvl_ent.size() - 1, max_seg, p_lvl_ent.p, p_ent_dst.p, p_ent_arc.p, p_e_src.p,
                        p_e_w.p,    p_e_id.p, p_e_osym.p, p_st_ent.p};
  TPO = DecodePairOutTables{o_sym_seg.p,  o_seg_src.p,  o_seg_arc.p, o_m_dst.p, o_m_w.p,   o_m_id.p,    po_m_osym.p,
                            (uint32_t)h_polvl_ent.size() - 1, max_oseg, po_lvl_ent.p, po_ent_src.p, po_ent_arc.p, po_e_dst.p,
                            po_e_w.p, po_e_id.p, po_e_osym.p, po_eps_out.p};
  T = DecodeTables{Q, final_state, n_syms, sym_seg.p, seg_dst.p, seg_arc.p, m_src.p, m_w.p, m_id.p, n_levels, eps_cyclic ? 1 : 0,
                   lvl_ent.p, ent_dst.p, ent_arc.p, e_src.p, e_dst.p, e_w.p, e_id.p, (uint32_t)eps.size(), st_ent.p};
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
