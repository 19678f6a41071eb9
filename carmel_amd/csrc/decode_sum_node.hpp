// decode_sum_node.hpp — the log-semiring value of one trellis node, shared by the all-paths sum (decode_sum.hip: SumNode) and the
// forward pass that keeps every row (decode_sample_node.hpp: SampleNode, the sampler's and the arc posteriors'), so that they agree bit for bit: ONE streaming accumulator
// (sweep_math.hpp's Lse), fed 0.0 first at node (0, start) only, then the matched candidates prev[src] + w of the arcs [m0, m1)
// in arc-id order, then the epsilon candidates same[src] + w of the arcs [e0, e1) in arc-id order, and read out once.  A
// candidate of -inf adds nothing; a node that nothing reaches is -inf.  (decode_sum.hip's header says what this order fixes.)
#pragma once
#include "decode.hpp"
#include "sweep_math.hpp"

namespace carmel_hip {
__device__ __forceinline__ double sum_node_value(const DecodeTables& T, const double* prev, uint32_t m0, uint32_t m1,
                                                 const double* same, uint32_t e0, uint32_t e1, bool start) {
  Lse a;
  a.init();
  if (start) a.add(0.0);
  for (uint32_t k = m0; k < m1; ++k) a.add(prev[T.m_src[k]] + T.m_w[k]);
  for (uint32_t k = e0; k < e1; ++k) a.add(same[T.e_src[k]] + T.e_w[k]);
  return a.value();
}
}  // namespace carmel_hip
