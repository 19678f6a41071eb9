// decode_kbest.hip — batch k-best decoding (carmel -b -k n: print_kbest / WFST::visit_kbest(k, ...), carmel.cc:379-397,
// fst.h:791, kbest.h) of many lines against one (composed) transducer: the trellis of decode.hip with an ordered LIST of up to K
// values per (line position i, state q) instead of one value.  Here are the node (KbNode) and the entry point: the kernel around
// the node is decode_trellis.hpp's, the walk and the host drivers are decode_paths.hip's, tables and handle decode.hpp's.
//
// A derivation of a line is a path of the machine from state 0 to the final state whose matched-side symbols (without *e*) spell
// the line and that uses no arc of weight zero; two derivations differ if their arc-id sequences differ (equal printed strings
// are not merged, as in the reference).  Its VALUE is its arcs' weights added in path order from the start, ((0 + w1) + w2) + ...,
// the trellis value the 1-best kernel chooses by.  A line gets its min(K, number of derivations) best derivations, greatest
// value first.
//
// A candidate at node (i, q) is (arc a into q, rank r in the list of a's source node) with value list[src][r] + w(a); the source
// node is (i - 1, src) for a matched arc and (i, src) for an epsilon arc.  Candidates are ordered by
//   value, descending; then matched arcs before epsilon arcs; then arc id, ascending; then r, ascending
// and the node's list is the first K of them.  The order is total, so the lists do not depend on lane count, scheduling, chunking
// or the memory tier, and with K = 1 it is decode.hip's tie rule: rank 0 is the path carmel_hip_decode returns.
//
// Selection (kb_select): one lane owns a node and fills its list slot by slot.  It keeps no array per rank or per arc (K is a
// run-time value; such an array would live in scratch memory): a source list is sorted and rounding is monotone, so an arc's
// candidates are in candidate order by r, and the arc's next candidate is the first r whose candidate comes AFTER the one picked
// last -- found by bisecting the source list against the last picked key (kb_next).  A slot costs (arcs into q) x log2 K reads.
//
// Rows: a row is |Q| K doubles, a state's list padded with -inf (no value is -inf: arcs of weight zero are dropped, so the
// length of a list is where its -inf begin and no count is stored).  The two rows are in LDS when 16 |Q| K bytes fit 64 KiB
// (|Q| K <= 4096), otherwise in a global buffer per line; option decode_lds=0 forces the global tier.
//
// Back-pointers: per (i, q, rank) the arc id (u32) and the predecessor's rank (u16), two arrays of (n + 1) |Q| K entries per
// line, for the walk.  The lists are ordered by the path-order value and the walk reports a path's arcs added from the end, so a
// line's reported weights may fail to be monotone in the last bit.  A node that epsilon arcs enter selects among its matched
// and its epsilon arcs in one pass into its own, still empty, list (decode_trellis.hpp): nothing is merged in place.  Only
// acyclic epsilon subgraphs have levels: a cyclic one is refused for K > 1, and K = 1 then runs the 1-best trellis.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>
#include "decode_kbest_list.hpp"
#include "decode_trellis.hpp"
#include "engine.hpp"

namespace {
// (kMaxK, a candidate's tag and kb_next, the bisection for an arc's next candidate: decode_kbest_list.hpp, which
// decode_pairs_kbest.hip shares)

// fill one node's list: the first K candidates of the matched arcs [m0, m1) (sources in row `prev`) and the epsilon arcs [e0, e1)
// (sources in row `same`), into out / oarc / orank (the node's K slots)
__device__ void kb_select(const DecodeTables& T, uint32_t K, const double* prev, uint32_t m0, uint32_t m1, const double* same,
                          uint32_t e0, uint32_t e1, double* out, uint32_t* oarc, uint16_t* orank) {
  const double ninf = -std::numeric_limits<double>::infinity();
  double vl = 0.0;  // the candidate picked last: (vl, tagl, rl), from slot 1 on
  uint64_t tagl = 0;
  uint32_t rl = 0;
  for (uint32_t j = 0; j < K; ++j) {
    double bv = ninf;
    uint64_t btag = 0;
    uint32_t br = 0;
    for (uint32_t k = m0; k < m1; ++k) {  // (arc-id order: of equal values the first seen stays)
      const double* S = prev + (size_t)T.m_src[k] * K;
      const double w = T.m_w[k];
      const uint64_t tag = T.m_id[k];
      const uint32_t r = j ? kb_next(S, w, K, tag, vl, tagl, rl) : 0;  // (slot 0: every arc's first)
      if (r < K) {
        const double v = S[r] + w;
        if (v > bv) {
          bv = v;
          btag = tag;
          br = r;
        }
      }
    }
    for (uint32_t k = e0; k < e1; ++k) {
      const double* S = same + (size_t)T.e_src[k] * K;
      const double w = T.e_w[k];
      const uint64_t tag = kEpsTag | T.e_id[k];
      const uint32_t r = j ? kb_next(S, w, K, tag, vl, tagl, rl) : 0;  // (slot 0: every arc's first)
      if (r < K) {
        const double v = S[r] + w;
        if (v > bv) {
          bv = v;
          btag = tag;
          br = r;
        }
      }
    }
    if (!(bv > ninf)) break;
    out[j] = bv;
    oarc[j] = (uint32_t)btag;
    orank[j] = (uint16_t)br;
    vl = bv;
    tagl = btag;
    rl = br;
  }
}

// the skeleton's node: a list of K values a state, K (arc, rank) back-pointers a node
struct KbNode {
  DecodePaths P;
  __host__ __device__ uint32_t width() const { return P.K; }
  __device__ void begin(uint32_t line, int lane) {
    P.bp_arc += P.bp_off[line];
    P.bp_rank += P.bp_off[line];
    if (lane == 0) {  // (0, start, rank 0): where every walk ends
      P.bp_arc[0] = kNone;
      P.bp_rank[0] = 0;
    }
  }
  // (0, start) keeps its initial list: an epsilon path into state 0 at position 0 would close a cycle
  __device__ void fill(const DecodeTables& T, uint32_t pos, uint32_t q, const double* prev, uint32_t m0, uint32_t m1, double* same,
                       uint32_t e0, uint32_t e1, bool start) const {
    if (start) return;
    const size_t row = (size_t)pos * T.n_states * P.K, at = (size_t)q * P.K;  // slot (pos |Q| + q) K
    kb_select(T, P.K, prev, m0, m1, same, e0, e1, same + at, P.bp_arc + row + at, P.bp_rank + row + at);
  }
  __device__ void read_out(uint32_t line, const double* F) const {
    uint32_t c = 0;
    while (c < P.K && F[c] > -std::numeric_limits<double>::infinity()) ++c;
    P.n_paths[line] = c;
  }
};

void launch_kbest_trellis(const carmel_hip_decoder* d, bool lds, uint32_t n, const DecodeLines& L, const DecodePaths& P,
                          hipStream_t s) {
  launch_trellis(d, lds, n, L, KbNode{P}, s);
}
}  // namespace

extern "C" {

int carmel_hip_decode_kbest(carmel_hip_decoder* d, uint32_t k, uint64_t n_lines, const uint64_t* off, const uint32_t* sym,
                            uint64_t* line_paths) {
  const char* who = "carmel_hip_decode_kbest";
  if (!d || !off || !line_paths || (off[n_lines] && !sym)) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decode_kbest: bad argument");
  if (k < 1 || k > kMaxK) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decode_kbest: k must be in 1 .. 1024");
  if (const int rc = decode_check_lines(who, n_lines, off)) return rc;
  if (d->eps_cyclic && k > 1)
    return fail(CARMEL_HIP_ERR_UNSUPPORTED,
                "carmel_hip_decode_kbest: the epsilon arcs of the matched side have a cycle; k-best paths over an epsilon cycle "
                "are not supported (k = 1 is)");
  std::vector<double> r_logw;
  std::vector<uint64_t> r_off;
  std::vector<uint32_t> r_arcs;
  // k = 1 over a cyclic epsilon subgraph is the 1-best trellis, best_path_has_cycle included
  const int rc = d->eps_cyclic ? decode_paths(d, who, 1, false, launch_decode_trellis, n_lines, off, sym, line_paths, r_logw, r_off, r_arcs)
                               : decode_paths(d, who, k, true, launch_kbest_trellis, n_lines, off, sym, line_paths, r_logw, r_off, r_arcs);
  if (rc) return rc;
  d->kb_logw.swap(r_logw);
  d->kb_off.swap(r_off);
  d->kb_arcs.swap(r_arcs);
  return CARMEL_HIP_OK;
}

int carmel_hip_decoder_kbest_size(carmel_hip_decoder* d, uint64_t* n_paths, uint64_t* n_arcs) {
  if (!d || !n_paths || !n_arcs) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decoder_kbest_size: bad argument");
  *n_paths = d->kb_logw.size();
  *n_arcs = d->kb_arcs.size();
  return CARMEL_HIP_OK;
}

int carmel_hip_decoder_get_kbest(carmel_hip_decoder* d, double* path_logw, uint64_t* path_off, uint32_t* arcs) {
  if (!d || !path_off || (!path_logw && !d->kb_logw.empty()) || (!arcs && !d->kb_arcs.empty()))
    return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decoder_get_kbest: bad argument");
  if (!d->kb_logw.empty()) std::memcpy(path_logw, d->kb_logw.data(), d->kb_logw.size() * sizeof(double));
  if (!d->kb_arcs.empty()) std::memcpy(arcs, d->kb_arcs.data(), d->kb_arcs.size() * sizeof(uint32_t));
  path_off[0] = 0;
  for (size_t p = 1; p < d->kb_off.size(); ++p) path_off[p] = d->kb_off[p];
  return CARMEL_HIP_OK;
}

}  // extern "C"
