// decode_best_paths_tables.cpp — builds the tables of decode_best_paths_tables.hpp: a counting sort of the existing arcs by
// destination and by source (stable, so arc-id order within a state), and Tarjan's strongly connected components without recursion.
#include "decode_best_paths_tables.hpp"
#include <algorithm>
#include <limits>

namespace carmel_hip {
namespace {
typedef std::vector<uint32_t> U32s;
constexpr uint32_t kUnseen = 0xffffffffu;

inline bool exists(double w) { return w > -std::numeric_limits<double>::infinity(); }
}  // namespace

BestPathsTablesHost build_best_paths_tables(uint32_t n_states, const U32s& src, const U32s& dst, const std::vector<double>& logw) {
  BestPathsTablesHost H;
  H.in_off.assign((size_t)n_states + 1, 0);
  H.out_off.assign((size_t)n_states + 1, 0);
  size_t n = 0;
  for (size_t k = 0; k < logw.size(); ++k)
    if (exists(logw[k])) {
      H.in_off[dst[k] + 1]++;
      H.out_off[src[k] + 1]++;
      ++n;
    }
  for (uint32_t q = 0; q < n_states; ++q) {
    H.in_off[q + 1] += H.in_off[q];
    H.out_off[q + 1] += H.out_off[q];
  }
  H.in_src.resize(n);
  H.in_id.resize(n);
  H.in_w.resize(n);
  H.out_dst.resize(n);
  U32s in_at(H.in_off.begin(), H.in_off.end() - 1), out_at(H.out_off.begin(), H.out_off.end() - 1);
  for (size_t k = 0; k < logw.size(); ++k)  // in arc-id order: a state's arcs stay in it
    if (exists(logw[k])) {
      const uint32_t i = in_at[dst[k]]++;
      H.in_src[i] = src[k];
      H.in_id[i] = (uint32_t)k;
      H.in_w[i] = logw[k];
      H.out_dst[out_at[src[k]]++] = dst[k];
    }
  return H;
}

int64_t positive_cycle_arc(const BestPathsTablesHost& H, const U32s& src, const U32s& dst, const std::vector<double>& logw) {
  const uint32_t n_states = (uint32_t)H.out_off.size() - 1;
  bool any = false;
  for (size_t k = 0; k < logw.size() && !any; ++k) any = exists(logw[k]) && logw[k] > 0.0;
  if (!any) return -1;
  U32s index(n_states, kUnseen), low(n_states, 0), comp(n_states, kUnseen), stack, at(n_states, 0);
  std::vector<uint32_t> call;  // the states whose out lists are being walked, innermost last
  uint32_t next_index = 0, n_comp = 0;
  for (uint32_t root = 0; root < n_states; ++root) {
    if (index[root] != kUnseen) continue;
    call.push_back(root);
    index[root] = low[root] = next_index++;
    stack.push_back(root);
    at[root] = H.out_off[root];
    while (!call.empty()) {
      const uint32_t q = call.back();
      if (at[q] < H.out_off[q + 1]) {
        const uint32_t t = H.out_dst[at[q]++];
        if (index[t] == kUnseen) {
          index[t] = low[t] = next_index++;
          stack.push_back(t);
          at[t] = H.out_off[t];
          call.push_back(t);
        } else if (comp[t] == kUnseen)  // (t is on the stack)
          low[q] = std::min(low[q], index[t]);
        continue;
      }
      call.pop_back();
      if (low[q] == index[q]) {
        uint32_t t;
        do {
          t = stack.back();
          stack.pop_back();
          comp[t] = n_comp;
        } while (t != q);
        ++n_comp;
      }
      if (!call.empty()) low[call.back()] = std::min(low[call.back()], low[q]);
    }
  }
  for (size_t k = 0; k < logw.size(); ++k)
    if (exists(logw[k]) && logw[k] > 0.0 && (src[k] == dst[k] || comp[src[k]] == comp[dst[k]])) return (int64_t)k;
  return -1;
}
}  // namespace carmel_hip
