// decode_sum.hip — batch all-paths sums (carmel -b --sum: post_compose's WFST::sum_acyclic_paths per line, carmel.cc:555-599,
// fst.h:1183-1191, propagate_paths graehl/shared/graph.h:391-419) of many lines against one (composed) transducer: the trellis
// of decode.hip over (line position i, state q) in the log semiring (logsumexp, +) instead of the tropical one (max, +), f64.
// The reference composes each line with the machine and propagates path weights through the result in topological order; here
// nothing is composed per line and nothing is recorded per position: there are no back-pointers, a line costs its two rows.
// Here are the node (SumNode) and the entry point: the kernel around the node is decode_trellis.hpp's, the chunk driver
// decode_paths.hip's, tables and handle decode.hpp's.
//
// S(x) = ln of the sum, over the derivations of line x, of the product of their arcs' weights (derivation: decode_kbest.hip's
// header); -inf if x has none.  Node (i, q) has ONE streaming accumulator (sweep_math.hpp's Lse), owned by one lane, fed in a
// fixed order and read out once:
//   0.0 first, at node (0, start) only;
//   then the matched candidates row[i - 1][src] + w of the arcs into q labelled x_i, in arc-id order;
//   then the epsilon candidates row[i][src] + w of the epsilon arcs into q, in arc-id order (their sources are of strictly lower
//   epsilon level: final since the barrier that ended that level).
// A candidate of -inf adds nothing.  That order fixes every bit of S(x): it does not depend on the memory tier, the chunking, the
// launch order or the lane count (decode_trellis.hpp says why the kernel keeps to it).  A single derivation costs no exp and no
// log (acc stays 1): its sum is its arcs' weights added in path order.
//
// Rows: two rows of |Q| doubles.  Only acyclic epsilon subgraphs have levels (the reference's sum is "acyclic-correct only",
// carmel.cc:1787): a cyclic one is refused before any launch.
#include <hip/hip_runtime.h>
#include <vector>
#include "decode_sum_node.hpp"
#include "decode_trellis.hpp"
#include "engine.hpp"

namespace {
// the skeleton's node: one double a state
struct SumNode {
  double* sum;  // [n]
  __host__ __device__ uint32_t width() const { return 1; }
  __device__ void begin(uint32_t, int) {}
  __device__ void fill(const DecodeTables& T, uint32_t, uint32_t q, const double* prev, uint32_t m0, uint32_t m1, double* same,
                       uint32_t e0, uint32_t e1, bool start) const {
    same[q] = sum_node_value(T, prev, m0, m1, same, e0, e1, start);  // (decode_sum_node.hpp: shared with the sampler's forward pass)
  }
  __device__ void read_out(uint32_t line, const double* F) const { sum[line] = F[0]; }
};
}  // namespace

extern "C" {

int carmel_hip_decode_sum(carmel_hip_decoder* d, uint64_t n_lines, const uint64_t* off, const uint32_t* sym, double* sum_logw) {
  if (!d || !off || !sum_logw || (off[n_lines] && !sym)) return fail(CARMEL_HIP_ERR_ARG, "carmel_hip_decode_sum: bad argument");
  if (const int rc = decode_check_lines("carmel_hip_decode_sum", n_lines, off)) return rc;
  if (d->eps_cyclic)  // (the reference's sum is "acyclic-correct only", carmel.cc:1787: refused, not approximated)
    return fail(CARMEL_HIP_ERR_UNSUPPORTED,
                "carmel_hip_decode_sum: the epsilon arcs of the matched side have a cycle; the sum of all paths over an epsilon "
                "cycle is not supported");
  DevBuf<double> d_sum;
  // there are no back-pointers to hold: a line costs its symbols (and its global-tier rows)
  return decode_chunks(d, n_lines, off, sym, 4, 0, 1u << 24, d->n_states, [&](DecodeChunk& c) {
    HIPCHK(d_sum.alloc(c.n));
    if (const int rc = c.begin()) return rc;
    launch_trellis(d, c.lds, c.n, c.L, SumNode{d_sum.p}, d->stream);
    if (const int rc = c.end()) return rc;
    HIPCHK(hipMemcpyAsync(sum_logw + c.lo, d_sum.p, c.n * sizeof(double), hipMemcpyDeviceToHost, d->stream));
    return c.wait();
  });
}

}  // extern "C"
