// decode_generate_tables.hpp — the tables of batch generation (carmel -G / -g; decode_generate.hip), built on the host from a
// machine's arcs: plain vectors, no device and no handle (decode_generate_tables.cpp).  The handle copies them to the device as
// they are on its first carmel_hip_decoder_generate call and drops them on carmel_hip_decoder_set_weights.
//
// Only arcs of weight > 0 (log weight > -inf) exist for generation.  They are filed twice, by their SOURCE:
//   * joint (carmel -G): one list per state, its arcs by arc id;
//   * conditional (carmel -g): one list per (state, matched-side symbol), that group's arcs by arc id; a state's groups are in
//     ascending symbol id, epsilon (0) first.
// Beside every arc of a list w_0 .. w_{m-1} stands its cumulative value: with M = max w_k and p_k = exp(w_k - M) (std::exp),
// cum_k = cum_{k-1} + p_k in f64, in list order; the list's total S is cum_{m-1}.  A draw u chooses the first k with
// cum_k > u S, which the device finds by bisection.
#pragma once
#include <cstdint>
#include <vector>

namespace carmel_hip {
// lists of arcs, one after the other: list g is arcs list_arc[g] .. list_arc[g + 1]
struct GenerateLists {
  std::vector<uint32_t> list_arc;  // [n_lists + 1] -> arcs
  std::vector<uint32_t> id, dst;   // per arc: its id, its destination
  std::vector<double> cum;         // per arc: the cumulative value within its list
};

struct GenerateTablesHost {
  GenerateLists joint;             // list q is state q's: joint.list_arc has n_states + 1 slots
  std::vector<uint32_t> st_grp;    // [n_states + 1] -> the state's groups, which are cond's lists
  std::vector<uint32_t> grp_sym;   // [n_groups]: the group's matched-side symbol
  GenerateLists cond;
};

// msym: every arc's symbol on the matched side; states are below n_states (the caller has checked)
GenerateTablesHost build_generate_tables(uint32_t n_states, const std::vector<uint32_t>& src, const std::vector<uint32_t>& dst,
                                         const std::vector<uint32_t>& msym, const std::vector<double>& logw);
}  // namespace carmel_hip
