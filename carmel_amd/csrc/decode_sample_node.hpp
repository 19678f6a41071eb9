// decode_sample_node.hpp — the node of the forward pass that keeps every row, shared by the posterior sampler (decode_sample.hip:
// its walk reads the rows) and the arc posteriors (decode_posterior.hip: its backward pass does): the sum's node arithmetic
// (decode_sum_node.hpp) in decode_trellis.hpp's kernel, and every node's value kept.  A line's (len + 1) |Q| doubles are in a
// global array: begin() fills them with -inf (the readers visit nodes the trellis never fills) and fill() stores each node's
// value beside the row the trellis keeps.  alpha[n][final] is bit for bit what carmel_hip_decode_sum returns for the line.
#pragma once
#include <limits>
#include "decode_sum_node.hpp"

namespace carmel_hip {
struct SampleNode {
  const uint64_t* a_off;  // [n + 1]: each line's (len + 1) x |Q| doubles
  double* alpha;
  uint32_t* has;  // [n]: the line has a derivation
  __host__ __device__ uint32_t width() const { return 1; }
  __device__ void begin(uint32_t line, int lane) {
    const uint64_t n = a_off[line + 1] - a_off[line];
    alpha += a_off[line];
    for (uint64_t s = lane; s < n; s += kLanes) alpha[s] = s == 0 ? 0.0 : -std::numeric_limits<double>::infinity();  // (0, start): 0.0
  }
  __device__ void fill(const DecodeTables& T, uint32_t pos, uint32_t q, const double* prev, uint32_t m0, uint32_t m1, double* same,
                       uint32_t e0, uint32_t e1, bool start) const {
    const double v = sum_node_value(T, prev, m0, m1, same, e0, e1, start);
    same[q] = v;
    alpha[(size_t)pos * T.n_states + q] = v;
  }
  __device__ void read_out(uint32_t line, const double* F) const { has[line] = F[0] > -std::numeric_limits<double>::infinity(); }
};
}  // namespace carmel_hip
