// decode_best_paths_tables.hpp — the tables of the K best paths of the whole machine (carmel -k n without -b; decode_best_paths.hip),
// built on the host from a machine's arcs: plain vectors, no device and no handle (decode_best_paths_tables.cpp).  The handle
// copies them to the device as they are on its first carmel_hip_decoder_best_paths call and drops them on
// carmel_hip_decoder_set_weights.
//
// Only arcs of log weight > -inf exist; symbols play no part.  They are filed twice:
//   * by DESTINATION, in arc-id order within a destination: (source, weight, arc id) -- what the select kernel merges;
//   * by SOURCE, destinations only -- what the commit kernel marks.
// positive_cycle_arc finds what makes the call refuse: an existing arc of log weight > 0 whose source and destination lie on a
// common cycle (the same strongly connected component of the existing arcs, or a self-loop).
#pragma once
#include <cstdint>
#include <vector>

namespace carmel_hip {
struct BestPathsTablesHost {
  std::vector<uint32_t> in_off;   // [n_states + 1] -> the arcs into the state
  std::vector<uint32_t> in_src, in_id;
  std::vector<double> in_w;
  std::vector<uint32_t> out_off;  // [n_states + 1] -> the arcs out of the state
  std::vector<uint32_t> out_dst;
};

// states are below n_states (the caller has checked)
BestPathsTablesHost build_best_paths_tables(uint32_t n_states, const std::vector<uint32_t>& src, const std::vector<uint32_t>& dst,
                                            const std::vector<double>& logw);

// -> the lowest id of an existing arc of log weight > 0 that lies on a cycle; -1: there is none.  H: the machine's tables (its out
// lists are the graph).  Tarjan's components, iterative (a machine of 10^6 states in a chain would overflow the stack of a
// recursive one), run only if a positive arc exists at all.
int64_t positive_cycle_arc(const BestPathsTablesHost& H, const std::vector<uint32_t>& src, const std::vector<uint32_t>& dst,
                           const std::vector<double>& logw);
}  // namespace carmel_hip
