// decode_generate_tables.cpp — builds the generation tables (decode_generate_tables.hpp): one routine that orders the arcs by
// (source, key, arc id) and closes a list wherever (source, key) changes, called once with no key (joint) and once with the
// matched-side symbol (conditional).
#include "decode_generate_tables.hpp"
#include <algorithm>
#include <array>
#include <cmath>
#include <limits>

namespace carmel_hip {
namespace {
typedef std::vector<uint32_t> U32s;

// The arcs by (src, key[k], arc id), one list per (src, key) -- per src alone without a key.  st_list [n_states + 1]: where each
// state's lists begin.
GenerateLists file_lists(uint32_t Q, const U32s& arcs, const U32s& src, const U32s& dst, const U32s* key, const std::vector<double>& logw,
                         U32s& st_list, U32s* list_key) {
  std::vector<std::array<uint32_t, 3> > keys;
  keys.reserve(arcs.size());
  for (uint32_t k : arcs) keys.push_back({src[k], key ? (*key)[k] : 0u, k});
  std::sort(keys.begin(), keys.end());
  GenerateLists f;
  st_list.assign(Q + 1, 0);
  for (size_t j = 0; j < keys.size(); ++j) {
    if (j == 0 || keys[j][0] != keys[j - 1][0] || keys[j][1] != keys[j - 1][1]) {
      f.list_arc.push_back((uint32_t)j);
      st_list[keys[j][0] + 1]++;
      if (list_key) list_key->push_back(keys[j][1]);
    }
    f.id.push_back(keys[j][2]);
    f.dst.push_back(dst[keys[j][2]]);
  }
  f.list_arc.push_back((uint32_t)keys.size());
  for (uint32_t q = 0; q < Q; ++q) st_list[q + 1] += st_list[q];
  // the cumulative values of every list, relative to the list's largest weight
  f.cum.resize(keys.size());
  for (size_t g = 0; g + 1 < f.list_arc.size(); ++g) {
    double M = -std::numeric_limits<double>::infinity();
    for (uint32_t j = f.list_arc[g]; j < f.list_arc[g + 1]; ++j) M = std::max(M, logw[f.id[j]]);
    double run = 0.0;
    for (uint32_t j = f.list_arc[g]; j < f.list_arc[g + 1]; ++j) {
      run += std::exp(logw[f.id[j]] - M);
      f.cum[j] = run;
    }
  }
  return f;
}
}  // namespace

GenerateTablesHost build_generate_tables(uint32_t n_states, const U32s& src, const U32s& dst, const U32s& msym,
                                         const std::vector<double>& logw) {
  U32s arcs;
  for (size_t k = 0; k < logw.size(); ++k)
    if (logw[k] > -std::numeric_limits<double>::infinity()) arcs.push_back((uint32_t)k);  // only arcs of weight > 0 exist
  GenerateTablesHost H;
  U32s st_joint;
  H.joint = file_lists(n_states, arcs, src, dst, nullptr, logw, st_joint, nullptr);
  // (a state without arcs has no joint list: the lists that exist are numbered in state order, so state q's is st_joint[q] if
  // st_joint[q + 1] > st_joint[q]; re-index so that list q is state q's, empty or not)
  U32s by_state(n_states + 1, 0);
  for (uint32_t q = 0; q <= n_states; ++q) by_state[q] = H.joint.list_arc[st_joint[q]];
  H.joint.list_arc.swap(by_state);
  H.cond = file_lists(n_states, arcs, src, dst, &msym, logw, H.st_grp, &H.grp_sym);
  return H;
}
}  // namespace carmel_hip
