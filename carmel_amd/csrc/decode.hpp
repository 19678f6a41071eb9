// decode.hpp — what the 1-best decoder (decode.hip) and the k-best decoder (decode_kbest.hip) share: the prepared tables, the
// decoder handle and the constants.  The tables are built and uploaded by carmel_hip_decoder::upload_tables (decode.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>
#include "engine.hpp"

namespace carmel_hip {
constexpr uint32_t kNone = 0xffffffffu;
constexpr int kLanes = 64;
constexpr uint32_t kLdsStates = 4096;  // two rows of |Q| doubles in 64 KiB of LDS (k-best: |Q| K doubles a row, |Q| K <= 4096)
constexpr int kErrCycle = 1, kErrWalk = 2;

struct DecodeTables {
  uint32_t n_states, final_state, n_syms;  // n_syms: 1 + the largest matched symbol
  const uint32_t* sym_seg;   // [n_syms + 1] -> segments
  const uint32_t* seg_dst;   // [n_seg]
  const uint32_t* seg_arc;   // [n_seg + 1] -> matched arcs
  const uint32_t* m_src;     // matched arcs, by (symbol, dst, arc id)
  const double* m_w;
  const uint32_t* m_id;
  uint32_t n_levels;         // epsilon levels (acyclic); 0 and eps_cyclic: one list in arc-id order
  int eps_cyclic;
  const uint32_t* lvl_ent;   // [n_levels + 1] -> entries (one destination state each)
  const uint32_t* ent_dst;
  const uint32_t* ent_arc;   // [n_ent + 1] -> epsilon arcs
  const uint32_t* e_src;     // epsilon arcs, by (level, dst, arc id) -- or in arc-id order when cyclic
  const uint32_t* e_dst;
  const double* e_w;
  const uint32_t* e_id;
  uint32_t n_eps;
};
}  // namespace carmel_hip

struct carmel_hip_decoder {
  int device = 0;
  int side = 0;
  uint32_t n_states = 0, final_state = 0;
  uint64_t n_arcs = 0;
  std::vector<uint32_t> src, dst, msym;  // msym: the matched-side symbol of every arc
  std::vector<double> logw;
  bool eps_cyclic = false;
  DevBuf<uint32_t> sym_seg, seg_dst, seg_arc, m_src, m_id, lvl_ent, ent_dst, ent_arc, e_src, e_dst, e_id, a_src;
  DevBuf<double> m_w, e_w, a_w;
  DevBuf<uint8_t> a_eps;
  DevBuf<uint8_t> eps_in;  // [|Q|]: the state is the destination of an epsilon arc of non-zero weight (k-best: its epsilon level is >= 1)
  DecodeTables T;
  std::vector<uint32_t> paths;  // the last decode's paths (arc ids, path order)
  // the last k-best decode (carmel_hip_decode_kbest): every path's reported weight, the CSR of the paths' arcs, the arcs
  std::vector<double> kb_logw;
  std::vector<uint64_t> kb_off;
  std::vector<uint32_t> kb_arcs;
  double last_ms = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  ~carmel_hip_decoder() {
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
  }
  int upload_tables();
};
