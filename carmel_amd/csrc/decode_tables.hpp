// decode_tables.hpp — the line-independent tables of the batch decoders, built on the host from a machine's arcs: plain vectors, no
// device and no handle (decode_tables.cpp).  carmel_hip_decoder::upload_tables (decode.hip) copies them to the device as they are
// and points DecodeTables, DecodeOutTables, DecodePairTables and DecodePairOutTables (decode.hpp) at the copies.
//
// Arcs of weight zero (-inf) are dropped before anything else: they are never taken.  The rest are
//   * matched (the matched side's symbol is not *e*): a CSR by symbol, each symbol's arcs by (end state, arc id) and cut into one
//     segment per end state -- once by destination, once by source;
//   * epsilon (the matched side is *e*): by (level of the end state, end state, arc id), cut into one entry per end state, with an
//     index of the entries by level -- by destination and by source, and by two kinds of level:
//       - level(q) = 1 + the largest level of an epsilon predecessor of q (0 without one).  If the epsilon subgraph has a cycle
//         there are no levels: the incoming view keeps the arcs in arc-id order without entries, the outgoing view is empty;
//       - for the pair decoders the same over the arcs with epsilon on BOTH sides (00) alone, which exist also when the levels
//         above do not (a 0M self-loop); both views are empty if the 00 arcs have a cycle, which pair_cycle then names.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace carmel_hip {
constexpr uint32_t kNone = 0xffffffffu;

// matched arcs by (symbol, end state, arc id): per-arc arrays in that order, segments of one (symbol, end state) each
struct FiledBySymbol {
  std::vector<uint32_t> sym_seg;    // [n_syms + 1] -> segments
  std::vector<uint32_t> seg_state;  // [n_seg]
  std::vector<uint32_t> seg_arc;    // [n_seg + 1] -> arcs
  std::vector<uint32_t> other, id, osym;  // per arc: the state at its other end, its id, the other side's symbol
  std::vector<double> w;
  uint32_t max_seg = 0;  // the most segments a symbol has
};

// epsilon arcs by (level of the end state, end state, arc id): per-arc arrays in that order, entries of one end state each
struct FiledByState {
  uint32_t n_levels = 0;            // lvl_ent's slots but one
  std::vector<uint32_t> lvl_ent;    // [n_levels + 1] -> entries
  std::vector<uint32_t> ent_state;  // [n_ent]
  std::vector<uint32_t> ent_arc;    // [n_ent + 1] -> arcs
  std::vector<uint32_t> other, id, osym;  // per arc, as above
  std::vector<double> w;
  std::vector<uint32_t> st_ent;  // [n_states] -> the state's entry, or kNone
  std::vector<uint8_t> has;      // [n_states]: a listed arc ends (or starts) at the state
};

struct DecodeTablesHost {
  uint32_t n_syms = 0;      // 1 + the largest matched symbol
  bool eps_cyclic = false;  // the epsilon subgraph has a cycle
  uint32_t n_eps = 0;
  uint32_t pair_levels = 0;  // the highest 00 level
  std::string pair_cycle;    // empty, or "states q -> ... -> q": one cycle of the 00 arcs
  FiledBySymbol m, om;       // matched arcs by destination (DecodeTables, DecodePairTables), by source (the two outgoing views)
  FiledByState e, oe;        // epsilon arcs by destination (DecodeTables; has: eps_in), by source (DecodeOutTables; has: eps_out)
  FiledByState pe, poe;      // the same by the 00 levels (DecodePairTables, DecodePairOutTables)
  std::vector<uint32_t> e_dst;          // the destinations of e's arcs: the closure of a cyclic subgraph walks (e.other, e_dst)
  std::vector<uint8_t> a_eps, a_flags;  // per arc, dropped ones too: the matched symbol is *e*; bit 0 it is not, bit 1 the other is not
};

// msym / osym: every arc's symbol on the matched and on the other side; states are below n_states (the caller has checked)
DecodeTablesHost build_decode_tables(uint32_t n_states, const std::vector<uint32_t>& src, const std::vector<uint32_t>& dst,
                                     const std::vector<uint32_t>& msym, const std::vector<uint32_t>& osym,
                                     const std::vector<double>& logw);
}  // namespace carmel_hip
