// decode_tables.cpp — builds the decoders' tables (decode_tables.hpp): one routine for the levels, one that files arcs by
// symbol, one that files them by state, each called once per view.
#include "decode_tables.hpp"
#include <algorithm>
#include <array>
#include <limits>

namespace carmel_hip {
namespace {
typedef std::vector<uint32_t> U32s;

// `arcs` in (first(k), second[k], k) order: equal keys stay in arc-id order
template <class First>
U32s ordered(const U32s& arcs, First first, const U32s& second) {
  std::vector<std::array<uint32_t, 3> > keys;
  keys.reserve(arcs.size());
  for (uint32_t k : arcs) keys.push_back({first(k), second[k], k});
  std::sort(keys.begin(), keys.end());
  U32s out;
  out.reserve(arcs.size());
  for (const auto& key : keys) out.push_back(key[2]);
  return out;
}

struct Arcs {
  const U32s &src, &dst, &msym, &osym;
  const std::vector<double>& logw;
};

struct Levels {
  U32s level;  // per state: 1 + the largest level of a predecessor over `arcs`, 0 without one
  U32s indeg;  // what Kahn's queue left of the in-degrees: non-zero at the states on or behind a cycle
  uint32_t highest = 0;
  bool acyclic = true;  // every state was reached
};

Levels levels(uint32_t Q, const Arcs& a, const U32s& arcs) {
  Levels lv;
  lv.level.assign(Q, 0);
  lv.indeg.assign(Q, 0);
  std::vector<U32s> outs(Q);
  for (uint32_t k : arcs) {
    outs[a.src[k]].push_back(k);
    lv.indeg[a.dst[k]]++;
  }
  U32s work;
  for (uint32_t q = 0; q < Q; ++q)
    if (!lv.indeg[q]) work.push_back(q);
  size_t seen = 0;
  while (seen < work.size()) {
    const uint32_t q = work[seen++];
    for (uint32_t k : outs[q]) {
      const uint32_t r = a.dst[k];
      lv.level[r] = std::max(lv.level[r], lv.level[q] + 1);
      lv.highest = std::max(lv.highest, lv.level[r]);
      if (--lv.indeg[r] == 0) work.push_back(r);
    }
  }
  lv.acyclic = seen == Q;
  return lv;
}

// The arcs by (symbol, end[k], arc id), one segment per (symbol, end state); `other` is the arcs' other end.
FiledBySymbol file_by_symbol(const Arcs& a, const U32s& arcs, const U32s& end, const U32s& other, uint32_t n_syms) {
  FiledBySymbol f;
  f.sym_seg.assign(n_syms + 1, 0);
  const U32s by = ordered(arcs, [&](uint32_t k) { return a.msym[k]; }, end);
  for (size_t j = 0; j < by.size(); ++j) {
    const uint32_t k = by[j];
    if (j == 0 || a.msym[k] != a.msym[by[j - 1]] || end[k] != end[by[j - 1]]) {
      f.seg_state.push_back(end[k]);
      f.seg_arc.push_back((uint32_t)j);
      f.sym_seg[a.msym[k] + 1]++;
    }
    f.other.push_back(other[k]);
    f.w.push_back(a.logw[k]);
    f.id.push_back(k);
    f.osym.push_back(a.osym[k]);
  }
  f.seg_arc.push_back((uint32_t)by.size());
  for (uint32_t x = 0; x < n_syms; ++x) {
    f.max_seg = std::max(f.max_seg, f.sym_seg[x + 1]);
    f.sym_seg[x + 1] += f.sym_seg[x];
  }
  return f;
}

// The arcs by (level[end[k]], end[k], arc id), one entry per end state; `other` is the arcs' other end.  lvl_ent has n_slots
// slots and a state of level L is counted into slot L + shift, so that lvl_ent[L + shift - 1] .. lvl_ent[L + shift] are the
// entries of level L.  Without levels (level == nullptr) the arcs stay as they are listed and there are no entries.
FiledByState file_by_state(uint32_t Q, const Arcs& a, const U32s& arcs, const U32s& end, const U32s& other, const U32s* level,
                           uint32_t n_slots, uint32_t shift) {
  FiledByState f;
  f.n_levels = n_slots ? n_slots - 1 : 0;
  f.lvl_ent.assign(n_slots, 0);
  f.st_ent.assign(Q, kNone);
  f.has.assign(Q, 0);
  const U32s by = level ? ordered(arcs, [&](uint32_t k) { return (*level)[end[k]]; }, end) : arcs;
  for (size_t j = 0; j < by.size(); ++j) {
    const uint32_t k = by[j];
    if (level && (j == 0 || end[k] != end[by[j - 1]])) {
      f.st_ent[end[k]] = (uint32_t)f.ent_state.size();
      f.ent_state.push_back(end[k]);
      f.ent_arc.push_back((uint32_t)j);
      f.lvl_ent[(*level)[end[k]] + shift]++;
    }
    f.other.push_back(other[k]);
    f.w.push_back(a.logw[k]);
    f.id.push_back(k);
    f.osym.push_back(a.osym[k]);
    f.has[end[k]] = 1;
  }
  if (level) f.ent_arc.push_back((uint32_t)by.size());
  for (size_t L = 0; L + 1 < f.lvl_ent.size(); ++L) f.lvl_ent[L + 1] += f.lvl_ent[L];
  return f;
}
}  // namespace

DecodeTablesHost build_decode_tables(uint32_t n_states, const U32s& src, const U32s& dst, const U32s& msym, const U32s& osym,
                                     const std::vector<double>& logw) {
  const uint32_t Q = n_states;
  const Arcs a{src, dst, msym, osym, logw};
  const U32s none;
  DecodeTablesHost H;
  U32s matched, eps, eps00;
  for (size_t k = 0; k < logw.size(); ++k) {
    if (!(logw[k] > -std::numeric_limits<double>::infinity())) continue;  // zero-probability arcs are never taken
    if (msym[k] == 0) {
      eps.push_back((uint32_t)k);
      if (osym[k] == 0) eps00.push_back((uint32_t)k);
    } else {
      matched.push_back((uint32_t)k);
      H.n_syms = std::max(H.n_syms, msym[k] + 1);
    }
  }
  H.n_eps = (uint32_t)eps.size();
  H.m = file_by_symbol(a, matched, dst, src, H.n_syms);
  H.om = file_by_symbol(a, matched, src, dst, H.n_syms);
  // DecodeTables and DecodeOutTables: the levels of the whole epsilon subgraph.  Destinations are at levels 1 .. highest (slot =
  // level), sources at 0 .. highest - 1 (slot = level + 1), in highest + 1 slots.  A cycle: no levels, nothing in the outgoing view
  const Levels lv = levels(Q, a, eps);
  H.eps_cyclic = !lv.acyclic;
  const uint32_t n_levels = lv.acyclic ? lv.highest : 0;
  H.e = file_by_state(Q, a, eps, dst, src, lv.acyclic ? &lv.level : nullptr, lv.acyclic ? n_levels + 1 : 0, 0);
  H.oe = file_by_state(Q, a, lv.acyclic ? eps : none, src, dst, &lv.level, n_levels + 1, 1);
  for (uint32_t k : H.e.id) H.e_dst.push_back(dst[k]);
  // DecodePairTables and DecodePairOutTables: the same arcs by the levels of the 00 subgraph alone.  A state that only 0M arcs
  // enter is at level 0, so levels 0 .. highest occur at either end (slot = level + 1, highest + 2 slots; one slot without arcs)
  const Levels plv = levels(Q, a, eps00);
  H.pair_levels = plv.acyclic ? plv.highest : 0;
  if (!plv.acyclic) {  // name one cycle: from a state Kahn left, step to a predecessor it left too until a state repeats
    U32s pred(Q, kNone), mark(Q, kNone);
    for (uint32_t k : eps00)
      if (plv.indeg[src[k]] && plv.indeg[dst[k]] && pred[dst[k]] == kNone) pred[dst[k]] = src[k];
    uint32_t q = 0;
    while (!plv.indeg[q]) ++q;
    uint32_t step = 0;
    for (; mark[q] == kNone; q = pred[q]) mark[q] = step++;
    std::string names = std::to_string(q);
    for (uint32_t r = pred[q]; r != q; r = pred[r]) names = std::to_string(r) + " -> " + names;
    H.pair_cycle = "states " + std::to_string(q) + " -> " + names;
  }
  const U32s& peps = plv.acyclic ? eps : none;
  const uint32_t pair_slots = peps.empty() ? 1 : H.pair_levels + 2;
  H.pe = file_by_state(Q, a, peps, dst, src, plv.acyclic ? &plv.level : nullptr, pair_slots, 1);
  H.poe = file_by_state(Q, a, peps, src, dst, &plv.level, pair_slots, 1);
  H.a_eps.resize(logw.size());
  H.a_flags.resize(logw.size());
  for (size_t k = 0; k < logw.size(); ++k) {
    H.a_eps[k] = msym[k] == 0;
    H.a_flags[k] = (msym[k] != 0 ? 1 : 0) | (osym[k] != 0 ? 2 : 0);
  }
  return H;
}
}  // namespace carmel_hip
