// forest.hpp — what forest.hip (the forest kernels and their launchers) shares with the host side of forest-em's
// forests (forest_host.cpp: the handle, EM, Viterbi; forest_gibbs.cpp: the sampler's schedules): the record words of
// the streams, the kernels' argument structs, the LDS each kernel needs, one launch_forest_* per kernel family.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace carmel_hip {

static const uint32_t F_HEADER = 0x80000000u, F_VALID = 0x40000000u, F_LAST = 0x20000000u, F_AND = 0x10000000u;
static const uint32_t F_IDX = 0x0fffffffu;
#define F_NONORM 0xffffffffu
#define FOREST_GHASH 2048u
static const size_t F_LDS_LIMIT = 150 * 1024;  // dynamic LDS a forest kernel may ask for

struct FGroup {  // 32 bytes, one wavefront of forests
  uint64_t stream_base;
  uint32_t maxlen, n_lanes, lane_base, max_nodes;
  uint64_t node_base;  // of the group's rows in node-indexed arrays: 64 * (sum of max_nodes over the groups before it)
};

struct FAnd {  // one per AND header record of the inside streams, in stream order (forest_proposal_kernel)
  uint64_t pos;    // position in the stream arrays
  uint32_t group;  // lane group
  uint32_t cls;    // rec_cls of the record
  uint32_t rule;
  uint32_t forest;
};

struct ForestArgs {
  const FAnd* and_list;          // the AND header records (n_and of them)
  uint64_t n_and;
  int p_only;                    // this sweep needs the proposal probabilities only, not their logarithms (temperature 1)
  const FGroup* groups;
  const uint2* ins_stream;
  const uint2* out_stream;
  const uint32_t* lane_forest;   // forest id per lane slot
  const uint32_t* lane_nodes;    // non-reference nodes per lane slot
  const double* rule_logw;
  double* post;                  // one slot per outside-stream record (only AND headers are used)
  double* forest_logprob;        // per forest: ln inside[root]
  double* scalars;               // {sum ln p over non-zero forests, n non-zero, n zero}
  // Gibbs
  const uint32_t* p_norm;        // per rule: norm group or F_NONORM
  const double* p_prior;
  const double* snap_x;          // counts / normsums the proposal is computed from
  const double* snap_norm;
  const uint32_t* hdr_pos;       // per (node, lane): position of the node's header in the inside stream
  const uint64_t* sample_off;    // per forest
  uint32_t* sample_len;
  uint32_t* sample_rules;
  const uint32_t* old_len;       // previous sample (counterfactual removal); may alias sample_* of the other buffer
  const uint32_t* old_rules;
  double* iter_out;
  // parallel sweep, second formulation (forest_proposal / forest_sample / forest_recount kernels)
  const uint32_t* rec_cls;       // per inside-stream record (AND headers): class of its rule | class of its norm group << 16,
                                 // both dense within the forest
  double* rec_logp;              // per inside-stream record (AND headers): ln proposal probability of the rule
  double* rec_p;                 //                                          the probability itself
  uint32_t* sample_cls;          // per sample entry: the rec_cls word of its record (0xffffffff: a rule outside every norm
                                 // group), written by the recount, scanned by the next sweep's proposal kernel
  uint32_t* sample_hdr;          // per sample entry: stream position of the AND header it came from
  const uint32_t* lane_of_forest;
  double* gcol;                  // forests too large for LDS: the inside (/ outside) columns of a group in global memory,
  uint64_t gcol_stride;          //   gcol + workgroup * gcol_stride (doubles)
  uint32_t* ghash;               // FOREST_GHASH slots per forest: own-sample table of lanes that overflow LDS (may be null)
  unsigned long long* trace;     // experiment (CARMEL_HIP_FOREST_TRACE): per block {start, after table, after inside, after walk, end}
  uint64_t seed;
  double power;                  // 1 / temperature of this sweep (annealing)
  uint32_t iter, first_group, serial_forest;  // serial_forest: exact mode processes exactly this forest (lane slot)
  int counterfactual;
};

// several lanes per forest (forest_sample_multi_kernel): FM_G lanes a forest, FM_FPW forests a wavefront
#ifndef FM_G
#define FM_G 8
#endif
#define FM_FPW (64 / FM_G)
struct FMultiArgs {
  const uint16_t* tab;      // per forest, its nodes numbered by height: {n, H, n_kids, -}, lvl_off[H + 1], kid_off[n + 1],
                            // kids[n_kids] (| 0x8000: back-reference)
  const uint32_t* hdr;      // per forest, per node: {row of its header in the lane's inside stream | bit 31 = AND, rule id,
                            // class word (ForestArgs::rec_cls), norm group}: four words per node
  const uint4* slots;       // per lane slot, two words of 16 bytes: {tab offset (u16 words, a multiple of 8: the table is copied
                            // 16 bytes at a time), hdr offset (u32 words)} as two 64-bit numbers, {sample offset (64 bit),
                            // forest (0xffffffff: none), nodes | table words << 15}: everything the staging needs to address
                            // its loads, in one round trip
  uint32_t lane_lo, lane_hi;            // the lane slots of this launch (a launch class)
  uint32_t max_tab, max_n, max_front;   // LDS per forest: table words, nodes, frontier entries
  int own_proposal;                     // the kernel computes the rules' proposal probabilities itself (forest_proposal_kernel
                                        // folded in: each AND node scans the forest's previous sample for its own uses)
  uint16_t* node_cnt;                   // own_proposal, non-null: per node (in the order of hdr) how often this sweep's sample
                                        // records it -- what the counts are gathered from afterwards (forest_rule_gather_kernel);
                                        // counted in the low half of the node's header word in LDS, which the walk does not use
  double* prob;                         // own_proposal: per node (in the order of hdr, four words a node) its rule's proposal
                                        // probability, and the sample is written as NODE numbers: what the recount needs of a
                                        // sampled rule -- id, class word, norm group, probability -- then lies in the forest's
                                        // own few lines of hdr / prob instead of three interleaved record streams (round 6)
};

// forest_rule_gather_kernel's split of the rule -> nodes lists (carmel_hip_forests_create cuts the pieces)
#define FRG_COLD 8u      // a rule on at most so many nodes: one thread, its loads side by side
#define FRG_PIECE 512u   // other rules: pieces of so many nodes, a wavefront each (eight loads a lane, side by side)

// ---- dynamic LDS of the kernels, by the figures of a launch class ----
// the class's two columns a lane (inside, outside) do not fit LDS: its kernels keep them in global memory (ForestArgs::gcol)
bool forest_cols_exceed_lds(uint32_t max_nodes);
size_t forest_estimate_lds_bytes(uint32_t max_nodes);      // forest_estimate_kernel<false>: the two columns
size_t forest_estimate_ext_lds_bytes(uint32_t max_nodes);  // forest_estimate_ext_kernel: 24 bytes a node and lane
// the E-step kernel of a launch class, by its largest forest: mantissa / exponent arithmetic where 24 bytes a node and lane fit
// LDS, else the log domain with its two columns in LDS, else the log domain with the columns in global memory
enum FEstepKind { F_ESTEP_EXT, F_ESTEP_LOG, F_ESTEP_GCOL };
FEstepKind forest_estep_kind(uint32_t max_nodes);
const char* forest_estep_kind_name(FEstepKind k);  // "ext", "log", "gcol"
// forest_gibbs_kernel: the inside column (unless in global memory), own_cap hash slots and stack_lds stack words a lane
size_t forest_gibbs_lds_bytes(bool gcol, uint32_t ins_rows, uint32_t own_cap, uint32_t stack_lds);
// forest_sample_kernel: the column (EXT: 12 bytes a node, else 8) and the stack ...
size_t forest_sample_lds_bytes(uint32_t max_nodes, bool ext, uint32_t stack_lds);
// ... and its LW form, the walk's tables in LDS: 16-bit rows (2 per node + 1, the child entries, the stack)
size_t forest_sample_lw_lds_bytes(uint32_t max_nodes, bool ext, uint32_t kid_rows, uint32_t stack_lds);
// forest_sample_multi_kernel: LDS of ONE forest (a wavefront takes FM_FPW times as much)
size_t forest_multi_lds_bytes(uint32_t max_n, uint32_t max_tab, uint32_t max_front);
inline uint32_t forest_multi_workgroups(const FMultiArgs& M) { return (M.lane_hi - M.lane_lo + FM_FPW - 1) / FM_FPW; }

// ---- launchers: template dispatch, grid, dynamic LDS (raised past the default limit right before the launch) ----
// A.first_group = the class's first lane group, n_groups of them, a workgroup each; gcol: A.gcol / gcol_stride are set
hipError_t launch_forest_estimate(const ForestArgs& A, bool gcol, uint32_t n_groups, uint32_t max_nodes, hipStream_t s);
hipError_t launch_forest_estimate_ext(const ForestArgs& A, uint32_t n_groups, uint32_t max_nodes, hipStream_t s);
hipError_t launch_forest_proposal(const ForestArgs& A, hipStream_t s);  // a thread per entry of A.and_list
struct FSampleLaunch {
  bool gcol, ext, lw;  // forest_sample_kernel<GCOL, EXT, LW>
  uint32_t n_groups, max_sample, max_nodes, stack_lds, kid_rows;
};
hipError_t launch_forest_sample(const ForestArgs& A, const FSampleLaunch& L, hipStream_t s);
hipError_t launch_forest_sample_multi(const ForestArgs& A, const FMultiArgs& M, uint32_t max_sample, hipStream_t s);
hipError_t launch_forest_gibbs(const ForestArgs& A, bool gcol, uint32_t n_groups, uint32_t max_sample, uint32_t ins_rows,
                               uint32_t own_cap, uint32_t stack_lds, hipStream_t s);
hipError_t launch_forest_viterbi(const ForestArgs& A, bool gcol, uint32_t n_groups, uint32_t max_sample, uint32_t max_nodes,
                                 uint32_t stack_lds, double* best_logprob, hipStream_t s);
struct FRecount {  // forest_recount_kernel's arguments
  const uint64_t* sample_off;
  const uint32_t* sample_len;
  uint32_t* rules;
  const uint32_t* p_norm;
  double* x;
  double* normsum;
  uint32_t n_forests;
  int sweep2;                    // bit 0: second formulation; bit 1: the counts are gathered afterwards, not added here
  const uint32_t* slot_forest;   // non-null: the forests of lane slots slot0 .. slot1 (one launch class); null: all forests
  uint32_t slot0, slot1;
  const uint32_t* node_hdr;      // non-null: the sample is node numbers (FMultiArgs::prob) ...
  const double* node_prob;
  const uint4* node_slots;
};
// once per run, before its first recount: the kernel's two LDS tables take more than the default limit
hipError_t prepare_forest_recount();
hipError_t launch_forest_recount(const FRecount& R, const ForestArgs& A, hipStream_t s);
hipError_t launch_forest_rule_gather(const uint32_t* inv_off, const uint32_t* inv_node, const uint16_t* node_cnt, uint32_t* rule_cnt,
                                     uint32_t n_rules, const uint32_t* pieces, uint32_t n_pieces, uint32_t n_inv, hipStream_t s);
hipError_t launch_forest_group_sum(const uint64_t* group_off, const uint32_t* group_rule, uint64_t n_groups, const uint32_t* rule_cnt,
                                   const double* prior_norm, double* normsum, hipStream_t s);
struct FCommit {  // forest_commit_kernel's arguments
  double *new_x, *p_x, *p_s, *p_tmax;
  const uint32_t* p_norm;
  double time;
  uint64_t n;
  const double* reset_x;  // non-null: the next sweep's count buffers start from these (the priors) ...
  double* next_norm;      // ... and its norm sums from reset_norm
  const double* reset_norm;
  uint64_t n_norm;
  uint32_t* rule_cnt;     // non-null: this sweep's counts are here (forest_rule_gather_kernel), to be added to prior
  const double* prior;
};
hipError_t launch_forest_commit(const FCommit& C, hipStream_t s);
// n_groups > 0
hipError_t launch_forest_mstep(double* rule_logw, const double* counts, double prior, const uint64_t* group_off,
                               const uint32_t* group_rule, uint64_t n_groups, double add_k, int zero_zero,
                               unsigned long long* max_bits, hipStream_t s);

}  // namespace carmel_hip
