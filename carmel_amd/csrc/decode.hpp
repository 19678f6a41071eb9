// decode.hpp — what the batch decoders (1-best decode.hip, k-best decode_kbest.hip, all-paths sums decode_sum.hip, posterior
// samples decode_sample.hip, arc posteriors decode_posterior.hip, pairs decode_pairs.hip, decode_pairs_posterior.hip,
// decode_pairs_sample.hip and decode_pairs_kbest.hip; generation, decode_generate.hip, and the whole machine's K best paths,
// decode_best_paths.hip, take the handle and the path store; its pruning, decode_prune.hip, and its sums over all paths,
// decode_machine_sums.hip, the handle) share: the prepared tables, the decoder
// handle, the constants, the arguments every trellis kernel takes, and the host drivers of decode_paths.hip -- the chunk driver of all entry points,
// the path driver of the two that return a trellis' recorded paths, and the assembly of a chunk's paths.  The tables are built on
// the host by build_decode_tables (decode_tables.hpp) and copied to the device by carmel_hip_decoder::upload_tables (decode.hip);
// the trellis kernel the k-best decoder and the sum share is decode_trellis.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <deque>
#include <functional>
#include <string>
#include <vector>
#include "decode_best_paths_tables.hpp"
#include "decode_generate_tables.hpp"
#include "decode_tables.hpp"
#include "engine.hpp"

namespace carmel_hip {
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
  const uint32_t* st_ent;    // [n_states] -> the entry whose destination the state is (kNone: no epsilon arc enters it, or cyclic)
};

// The outgoing view of the same arcs, for the backward pass of the arc posteriors (decode_posterior.hip): DecodeTables files an arc
// under its destination, this under its source.  Symbols, dropped arcs and epsilon levels are DecodeTables'; a source's level is
// strictly lower than the levels of its epsilon arcs' destinations, so the levels that hold sources are 0 .. n_levels - 1.
// Empty epsilon lists when the epsilon subgraph is cyclic (no levels: the posteriors are refused).
struct DecodeOutTables {
  const uint32_t* sym_seg;   // [n_syms + 1] -> segments
  const uint32_t* seg_src;   // [n_seg]
  const uint32_t* seg_arc;   // [n_seg + 1] -> matched arcs
  const uint32_t* m_dst;     // matched arcs, by (symbol, src, arc id)
  const double* m_w;
  const uint32_t* m_id;
  const uint32_t* lvl_ent;   // [n_levels + 1] -> entries (one source state each), by the level of the source
  const uint32_t* ent_src;
  const uint32_t* ent_arc;   // [n_ent + 1] -> epsilon arcs
  const uint32_t* e_dst;     // epsilon arcs, by (level of src, src, arc id)
  const double* e_w;
  const uint32_t* e_id;
  const uint8_t* eps_out;    // [n_states]: an epsilon arc leaves the state
};

// What the pair decoder (decode_pairs.hip) adds to DecodeTables' matched arrays: the other side's symbol of every matched arc, and
// the matched-side-epsilon arcs once more, ordered for a trellis over (matched position i, other position j, state q).  There an
// epsilon arc whose other symbol is not epsilon (0M) advances j and needs no order inside a cell; only the arcs with epsilon on
// both sides (00) do, so the levels are the longest-path levels of the 00 subgraph ALONE: they exist whenever the 00 arcs are
// acyclic, also when DecodeTables' epsilon levels do not (a 0M self-loop).  A state that only 0M arcs enter is at level 0.
struct DecodePairTables {
  const uint32_t* m_osym;   // parallel to m_src / m_w / m_id
  uint32_t n_levels;        // 1 + the highest 00 level of a state that an epsilon arc enters (0: no epsilon arcs)
  uint32_t max_seg;         // the most destination segments a matched symbol has
  const uint32_t* lvl_ent;  // [n_levels + 1] -> entries (one destination state each), by the 00 level of the state
  const uint32_t* ent_dst;
  const uint32_t* ent_arc;  // [n_ent + 1] -> epsilon arcs
  const uint32_t* e_src;    // epsilon arcs, by (00 level of dst, dst, arc id)
  const double* e_w;
  const uint32_t* e_id;
  const uint32_t* e_osym;   // 0: a 00 arc (source in the same cell); else a 0M arc (source in cell (i, j - 1))
  const uint32_t* st_ent;   // [n_states] -> the entry whose destination the state is (kNone: no such arc enters it); the pair sampler's walk
};

// The outgoing view of DecodePairTables, for the backward pass of the pair arc posteriors (decode_pairs_posterior.hip): an arc is
// filed under its source.  The matched CSR is DecodeOutTables' (it has no levels in it) with the other side's symbols beside it;
// the matched-side-epsilon arcs are filed by the 00 level of their SOURCE (DecodePairTables' levels: a 00 arc's destination is of
// strictly higher level than its source, a 0M arc leaves the cell), never by DecodeOutTables' epsilon levels, which a 0M loop
// takes away.  Empty epsilon lists when the 00 arcs have a cycle (the pair entry points refuse).
struct DecodePairOutTables {
  const uint32_t* sym_seg;  // [n_syms + 1] -> segments          (DecodeOutTables')
  const uint32_t* seg_src;  // [n_seg]
  const uint32_t* seg_arc;  // [n_seg + 1] -> matched arcs
  const uint32_t* m_dst;    // matched arcs, by (symbol, src, arc id)
  const double* m_w;
  const uint32_t* m_id;
  const uint32_t* m_osym;   // parallel to m_dst / m_w / m_id
  uint32_t n_levels;        // 1 + the highest 00 level of a state that an epsilon arc leaves (0: no epsilon arcs)
  uint32_t max_seg;         // the most source segments a matched symbol has
  const uint32_t* lvl_ent;  // [n_levels + 1] -> entries (one source state each), by the 00 level of the state
  const uint32_t* ent_src;
  const uint32_t* ent_arc;  // [n_ent + 1] -> epsilon arcs
  const uint32_t* e_dst;    // epsilon arcs, by (00 level of src, src, arc id)
  const double* e_w;
  const uint32_t* e_id;
  const uint32_t* e_osym;   // 0: a 00 arc (destination in the same cell); else a 0M arc (destination in cell (i, j + 1))
  const uint8_t* eps_out;   // [n_states]: a matched-side-epsilon arc (of weight > 0) leaves the state
};

// a chunk's lines, as every trellis kernel takes them: one workgroup of kLanes lanes per line
struct DecodeLines {
  const uint64_t* off;    // chunk-local CSR of the lines' symbols
  const uint32_t* sym;
  const uint32_t* order;  // launch order: chunk-local line index of block b
  double* rows;           // global tier: a line's two rows (nullptr in the LDS tier)
};

// what a trellis kernel that records paths leaves to the walk: K slots per (position, state), slot (i |Q| + q) K + r
struct DecodePaths {
  const uint64_t* bp_off;  // [n + 1]: each line's (len + 1) x |Q| x K slots
  uint32_t* bp_arc;        // the arc that enters the slot's path last (kNone: the path ends here)
  uint16_t* bp_rank;       // the rank of that arc's source; nullptr: every rank is 0 (the 1-best trellis, 4 bytes a slot)
  uint32_t* n_paths;       // [n]: how many of its K slots the final node of a line fills
  int* err;
  uint32_t K;
};

// The generation tables on the device (decode_generate_tables.hpp), one per mode.  Joint: st_grp is nullptr and list q is state
// q's.  Conditional: state q's groups are st_grp[q] .. st_grp[q + 1], each a list.  List g is arcs list_arc[g] .. list_arc[g + 1].
struct GenerateTables {
  const uint32_t* st_grp;    // [n_states + 1], or nullptr
  const uint32_t* list_arc;  // [n_lists + 1]
  const uint32_t* id;        // per arc of a list: its id, its destination, its cumulative value
  const uint32_t* dst;
  const double* cum;
};

// The tables of the K best paths of the whole machine on the device (decode_best_paths_tables.hpp): the existing arcs by
// destination, in arc-id order within one, and once more by source.
struct BestPathsTables {
  const uint32_t* in_off;   // [n_states + 1] -> the arcs into the state
  const uint32_t* in_src;
  const uint32_t* in_id;
  const double* in_w;
  const uint32_t* out_off;  // [n_states + 1] -> the arcs out of the state
  const uint32_t* out_dst;
};
}  // namespace carmel_hip

struct carmel_hip_decoder {
  int device = 0;
  int side = 0;
  uint32_t n_states = 0, final_state = 0;
  uint64_t n_arcs = 0;
  std::vector<uint32_t> src, dst, msym;  // msym: the matched-side symbol of every arc
  std::vector<double> logw;
  std::vector<uint32_t> osym;  // the other side's symbol of every arc
  bool eps_cyclic = false;
  // the tables on the device, and the buffers that own them: one buffer per table, in the order upload_tables filled the four
  // structs (a deque: a DevBuf frees its memory when destroyed and must not move)
  DecodeTables T;
  DecodeOutTables TO;        // the outgoing view
  DecodePairTables TP;       // the pair decoders' tables (decode_pairs.hip)
  DecodePairOutTables TPO;   // their outgoing view, for carmel_hip_decode_pairs_posterior
  std::deque<DevBuf<uint32_t> > tab_u32;
  std::deque<DevBuf<double> > tab_f64;
  std::deque<DevBuf<uint8_t> > tab_u8;
  // what the walks and the trellis launches take beside the structs: every arc's source and weight, dropped arcs too
  DevBuf<uint32_t> a_src;
  DevBuf<double> a_w;
  DevBuf<uint8_t> a_eps;    // per arc: the matched symbol is epsilon
  DevBuf<uint8_t> a_flags;  // per arc, for the pair walk: bit 0 the matched symbol is not epsilon, bit 1 the other symbol is not
  DevBuf<uint8_t> eps_in;   // [|Q|]: the state is the destination of an epsilon arc of non-zero weight (k-best: its epsilon level is >= 1)
  // the arc counts of a carmel_hip_decode_posterior or carmel_hip_decode_pairs_posterior call: zeroed once per call, accumulated
  // over all its chunks
  DevBuf<double> count;
  uint32_t pair_levels = 0;  // the highest 00 level
  std::string pair_cycle;    // empty, or the 00 cycle that makes the pair entry points refuse
  std::vector<uint32_t> paths;  // the last decode's paths (arc ids, path order)
  // the last k-best or sample call (carmel_hip_decode_kbest, carmel_hip_decode_sample, carmel_hip_decode_pairs_sample,
  // carmel_hip_decode_pairs_kbest): every path's reported weight, the CSR
  // of the paths' arcs, the arcs
  std::vector<double> kb_logw;
  std::vector<uint64_t> kb_off;
  std::vector<uint32_t> kb_arcs;
  // the generation tables (decode_generate_tables.hpp; carmel_hip_decoder_generate, decode_generate.hip): built and copied by the
  // first generate call, dropped by carmel_hip_decoder_set_weights
  bool gen_ready = false;
  carmel_hip::GenerateTables GJ, GC;  // joint: a list per state; conditional: a state's groups, a list per group
  DevBuf<uint32_t> gen_u32[7];
  DevBuf<double> gen_f64[2];
  // the tables of the whole machine's K best paths (decode_best_paths_tables.hpp; carmel_hip_decoder_best_paths,
  // decode_best_paths.hip): built and copied by the first call, dropped by carmel_hip_decoder_set_weights
  bool bp_ready = false;
  int64_t bp_cycle_arc = -1;  // an arc of weight above 1 on a cycle: the call refuses
  uint64_t bp_n_in = 0;       // the arcs that exist
  carmel_hip::BestPathsTables BP;
  DevBuf<uint32_t> bp_u32[5];
  DevBuf<double> bp_f64;
  uint32_t bp_rounds = 0;     // the last successful call's statistics
  uint64_t bp_selected = 0;
  // pruning by best-path weight (carmel_hip_decoder_prune, decode_prune.hip): the tables of the forward and the backward pass for
  // one arc threshold, built and copied by the first call with it, dropped by carmel_hip_decoder_set_weights; the last successful
  // call's distances and rounds
  bool pr_ready = false, pr_have = false;
  double pr_min_arc_logw = 0;
  int64_t pr_cycle_arc = -1;
  carmel_hip::BestPathsTables PR[2];  // forward, backward
  DevBuf<uint32_t> pr_u32[10], pr_dst;  // pr_dst: every arc's destination, beside a_src
  DevBuf<double> pr_f64[2];
  std::vector<double> pr_fwd, pr_bwd;
  uint32_t pr_rounds[2] = {0, 0};
  // the sums over all paths of the whole machine (carmel_hip_decoder_machine_sums, decode_machine_sums.hip): the tables of the
  // machine and of its reversal, built and copied by the first call, dropped by carmel_hip_decoder_set_weights; the last
  // successful call's results
  bool ms_ready = false, ms_have = false;
  carmel_hip::BestPathsTables MS[2];  // forward, backward
  DevBuf<uint32_t> ms_u32[10], ms_dst;  // ms_dst: every arc's destination, beside a_src
  DevBuf<double> ms_f64[2];
  std::vector<double> ms_alpha, ms_beta, ms_cf, ms_cb, ms_post;
  std::vector<uint32_t> ms_level;
  double ms_total = 0, ms_paths = 0;
  uint64_t ms_useful = 0;
  uint32_t ms_levels[2] = {0, 0};
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

namespace carmel_hip {
// One chunk of a call's lines, as decode_chunks hands it to its caller.  The caller launches its kernels between begin() and end()
// (which bracket them with the handle's events), queues its copies back and calls wait(): last_ms covers the kernels, not the copies.
struct DecodeChunk {
  carmel_hip_decoder* d;
  uint64_t lo, hi;        // the chunk is lines [lo, hi) of the call
  uint32_t n;             // hi - lo
  const uint64_t* h_off;  // [n + 1]: L.off on the host
  DecodeLines L;          // on the device
  const uint64_t* h_off2;  // pairs: the second lines' chunk-local CSR on the host, and (off2, sym2) on the device
  const uint64_t* off2;
  const uint32_t* sym2;
  bool lds;               // the rows are in LDS
  float ms;
  int begin();
  int end();   // checks the launches
  int wait();  // the stream has drained; adds the bracket's time
};

// <who>: bad line offsets, for the entry point `who`
int decode_check_lines(const char* who, uint64_t n_lines, const uint64_t* off);
// The chunk driver: lines go in chunks, in line order, of fewer than `cap` lines whose cost fits the budget (option
// "decode_chunk_bytes", default 1 GiB; a single line larger than it goes alone).  A line of len symbols costs a len + b bytes,
// plus its two rows of row_doubles doubles in the global tier (row_doubles > kLdsStates, or option decode_lds=0).  Every chunk's
// lines are uploaded with their launch order (longest first) and handed to `body`; d->last_ms is set if every chunk returns 0.
int decode_chunks(carmel_hip_decoder* d, uint64_t n_lines, const uint64_t* off, const uint32_t* sym, uint64_t a, uint64_t b,
                  uint64_t cap, uint64_t row_doubles, const std::function<int(DecodeChunk&)>& body);

// The same driver with the cost of a line given by its index (cost(l) bytes, whatever it is made of): chunks of fewer than `cap`
// lines whose costs fit the budget, a line that costs more goes alone; a chunk's launch order is costliest first (stable).  With
// off2 / sym2 (pairs) the second lines of the chunk are uploaded beside the first.  The driver allocates no rows: c.L.rows is
// nullptr, c.lds is `lds`.  decode_chunks above is this with cost(l) = a len + b (+ 16 row_doubles in the global tier), which
// orders by length as it always did, and with its rows.
int decode_chunks_by_cost(carmel_hip_decoder* d, uint64_t n_lines, const uint64_t* off, const uint32_t* sym, const uint64_t* off2,
                          const uint32_t* sym2, bool lds, const std::function<uint64_t(uint64_t)>& cost, uint64_t cap,
                          const std::function<int(DecodeChunk&)>& body);

// launches a path-recording trellis kernel over the n lines of a chunk
typedef void (*TrellisLaunch)(const carmel_hip_decoder* d, bool lds, uint32_t n, const DecodeLines& L, const DecodePaths& P,
                              hipStream_t s);
void launch_decode_trellis(const carmel_hip_decoder* d, bool lds, uint32_t n, const DecodeLines& L, const DecodePaths& P,
                           hipStream_t s);  // the 1-best trellis (decode.hip): K = 1, no rank array
// The path driver: per chunk the trellis `launch` with K slots a node (a rank array if `ranked`), the counting walk, the prefix
// sums and the writing walk.  -> line_paths [n_lines + 1] (line -> paths), and per path its reported weight, the CSR of its arcs
// and the arcs, in (line, rank) order.  Errors are reported in the name of the entry point `who`.
int decode_paths(carmel_hip_decoder* d, const char* who, uint32_t K, bool ranked, TrellisLaunch launch, uint64_t n_lines,
                 const uint64_t* off, const uint32_t* sym, uint64_t* line_paths, std::vector<double>& logw,
                 std::vector<uint64_t>& path_off, std::vector<uint32_t>& arcs);
// What the path driver and the sampler make of a chunk's counting walk: np [n] paths a line (its first np[l] of K slots), len
// and lw [n K] every slot's arcs and reported weight.  Appends the paths' weights to logw and their ends (from `base` on, the
// arcs already held) to path_off, sets line_paths for the chunk's lines, -> [n K + 1]: where each slot's arcs go in the chunk's
// compact path array (a slot without a path is empty).
std::vector<uint64_t> decode_collect_paths(const DecodeChunk& c, uint32_t K, const std::vector<uint32_t>& np,
                                           const std::vector<uint32_t>& len, const std::vector<double>& lw, uint64_t base,
                                           uint64_t* line_paths, std::vector<double>& logw, std::vector<uint64_t>& path_off);
}  // namespace carmel_hip
