// layout.hpp — the host planner: where each BP kernel family's lanes, LDS
// slots and mailbox entries go.  Three plans, one per family:
//   RegularLayout  (bp_regular.hip)     which lane owns which column, and the
//                                       slot half of each c2v message;
//   PartitionPlan  (bp_coop.hip)        which of G workgroups owns which rows
//                                       and columns, and the cut-edge exchange;
//   IrregularPlan  (bp_irregular.hip)   which wave and round runs which
//                                       columns / rows, and the slot blocks.
// A fourth, LayeredPlan (bp_irregular_lnms.hip), is the row layers of the
// layered min-sum schedule and the passes the kernel cuts them into.
// A plan changes nothing in the arithmetic: any valid plan gives the same
// decoder output, it only moves work between lanes, so it decides speed (LDS
// bank conflicts, mailbox traffic, SIMD balance) and nothing else.
//
// Every field of the three structs goes into the plan's digest in
// tests/native/plan_check.cpp, which tests/golden/host/plan_digests.json pins:
// a field added to a struct must be added to its digest there.
#pragma once
#include <cstdint>
#include <vector>

#include "code.hpp"

namespace kml {

// ------------------------------------------------- RegularLayout (bp_regular)
// The kernel keeps one 16-byte slot per edge in LDS, in the reference's row
// traversal order (rows contiguous, so a check-row lane pair reads its row as
// consecutive slots).  The variable-node phase gathers and scatters those slots
// by column, which on gfx950 serialises on LDS banks (MI355X_MICROARCH.md §LDS:
// ds_read_b64 banks by 32-lane halves mod 64 dwords, ds_write_b128 by 8-lane
// groups mod 32 dwords).  The plan changes nothing in the arithmetic; it picks
//   * which lane owns which column (`order`, any permutation is valid: the VN
//     phase is column-independent), by simulated annealing on the bank-conflict
//     count of the VN gathers/scatters, and
//   * which half of its slot a check-to-variable message is written to
//     (`c2v_addr`): rows whose position in the CN phase has bit 2 set store it
//     in the upper 8 bytes, which makes the CN phase's 16-lane ds_write_b64
//     groups conflict-free (8 rows x 2 edges on 16 distinct bank pairs).
struct RegularLayout {
  std::vector<int32_t> order;     // position -> column (position = r*T + thread)
  std::vector<int32_t> pos;       // column -> position
  std::vector<int32_t> c2v_addr;  // aligned with col_slot: byte offset of the c2v message
  long long cost_initial = 0;     // modelled extra LDS cycles per VN phase (all waves)
  long long cost_final = 0;
};

// Positions are grouped by wave (64 consecutive positions) whatever the
// kernel's workgroup size is, so the plan does not depend on it.  Cached per
// graph (row_col, col_slot, cn_order).
void plan_regular_layout(const LdpcCode &L, RegularLayout &out);

// -------------------------------------------- PartitionPlan (bp_part_kernel)
// Partition plan for the partitioned cooperative BP kernel (bp_coop.hip,
// bp_part_kernel): a group of G workgroups decodes one codeword; member m owns
// the rows [m*MG, (m+1)*MG) and the columns [m*NG, (m+1)*NG) of the orders
// below.  Its LDS holds the 16-byte slots of its rows (slot (P - m*MG)*dc + k
// for the k-th edge of the row at plan index P) followed by one MIRROR slot per
// CUT edge of its columns (an edge whose row another member owns).  Cut edges
// are exchanged through two mailboxes in global memory, v2c (column owner ->
// row owner) and c2v (row owner -> column owner), indexed by the cut-edge
// index x, which is sorted by (row owner, row slot): each row owner's share
// is one contiguous run and the cut edges of one row are consecutive (the
// tagged exchange addresses a row's mailbox entries from its first index and
// a 6-bit mask); each column owner's share is a few runs.  The planner
// minimises the number of cut edges (balanced G-way partition of the Tanner
// graph: alternating majority assignment of columns given rows and rows given
// columns, capacity-bounded, then annealed single-node moves in four seeded
// chains: layout.cpp PartRefiner).  Any partition gives the same decoder
// output: it only moves work between lanes.
struct PartitionPlan {
  int G = 0, MG = 0, NG = 0;
  int ncut = 0;                 // cut edges (mailbox entries)
  int mirror_max = 0;           // most mirror slots of one member
  std::vector<int32_t> vn;      // N: columns in member order (member m: [m*NG, (m+1)*NG))
  std::vector<int32_t> cn;      // M: rows in member order
  std::vector<int32_t> pos;     // N: column -> index into vn
  std::vector<int32_t> vaddr;   // 3N (dv = 3): [p*dv + k] = LDS byte offset of the k-th edge of column vn[p]
                                // in its owner's LDS (a row slot or a mirror slot)
  // exchange lists, per member [ptr[m], ptr[m+1]); entry = (x << 16) | (LDS slot index)
  std::vector<int32_t> xr, xr_ptr;  // as row owner: cut edges of its rows
  std::vector<int32_t> xc, xc_ptr;  // as column owner: cut edges of its columns (-> mirror slots)
  // tagged exchange (bp_part_kernel's direct mailbox stores):
  std::vector<int32_t> vx;  // 3N: [p*dv + k] = mailbox index x of that edge when it is cut, else -1
  std::vector<int32_t> rx;  // M, plan order: (x of the row's first cut edge << 8) | mask of its cut
                            // edges by position in the row (0 when none are cut)
  long long anneal_initial = 0, anneal_final = 0;  // VN bank-conflict model cost before / after annealing
  int interior = 0;  // columns whose edges are all their member's (each member's last run of vn)
  // every member owns rows that receive cut-edge v2c messages from every other
  // member (the tagged exchanges' ordering arguments use it, bp_coop.hip)
  bool all_pairs = false;
};

// False when the code is not regular or M, N are not multiples of G.  Reads
// the refinement's schedule from the environment on every call
// (KML_PART_REFINE=0: no cut refinement; KML_PART_REFINE_ITERS: annealing
// steps per chain, default 150 M) and caches per (graph, G, schedule).
bool plan_partition(const LdpcCode &L, int G, PartitionPlan &out);

// -------------------------------------------- IrregularPlan (bp_irregular)
// Round plan of the irregular-code BP kernel (bp_irregular.hip): T threads in
// W = T/64 waves, three rounds per phase.  In rounds 0 and 1 a lane owns TWO
// columns (two half-rows) of the same degree and runs their chains
// interleaved; round 2 holds single columns (half-rows).  Every wave of a
// round runs one degree (64 columns, or 32 rows as lane pairs), except at
// most a few waves that mix the leftovers of two degrees.  Pairs are formed
// from the highest degrees up to a limit (the longest dependent chains gain
// most from a second chain; the limits keep two chains within the registers), and the waves are placed so that the modelled VALU work of
// the 4 SIMDs (wave w runs on SIMD w % 4) is balanced.  Any placement gives
// the same decoder output: it only moves work between lanes.
constexpr int kIrrThreads = 768;  // threads per workgroup of bp_irregular.hip (its plan is made for this)
constexpr int kIrrVnPairMax = 4;  // highest column degree bp_irregular.hip pairs
constexpr int kIrrCnPairMax = 8;  // highest row degree it pairs (BG2, 50 iterations: 4/8 19.7 ms,
                                  // 5/8 20.5, 7/8 21.8, 9/8 23.0 with c2v reloads against spills)

// Slot layout of the irregular kernel: the rows of a wave's round (32 lane
// pairs, one degree) form a block in which edge e of the row at pair index pi
// sits at slot pi + e * kIrrCnStride, so at every CN step a wave reads two
// contiguous 512-byte runs (conflict-free b128 reads) instead of 32 rows
// strided by their degree.
constexpr int kIrrCnStride = 32;

struct IrregularPlan {
  std::vector<int32_t> vn;        // [3*T]: column of position r*T + t, -1 = idle
  std::vector<int32_t> cn;        // [3*T/2]: row of lane pair r*T/2 + (t >> 1), -1 = idle
  std::vector<int32_t> cn_base;   // [3*T/2]: slot of edge 0 of that row, -1 = idle
  std::vector<int32_t> col_slot;  // [E]: slot of each column-ordered edge (as LdpcCode::col_slot)
  int n_slots = 0;                // slots incl. the holes of partly filled blocks
};

// False when the code's degree groups do not fit three rounds of T lanes.
bool plan_irregular(const LdpcCode &L, int T, int vn_pair_max, int cn_pair_max, IrregularPlan &out);

// ---------------------------------------- LayeredPlan (bp_irregular_lnms)
// Layer plan of the layered min-sum kernel (bp_irregular_lnms.hip).  A layer
// is a maximal run of consecutive rows with pairwise disjoint columns, found
// greedily in row order: a row that shares a column with the open layer closes
// it and opens the next (kml_code_layers; 5G BG2 K960: 12 layers of 96 rows).
// The rows of a layer touch disjoint posteriors and messages, so the kernel
// works on them in parallel and still computes the serial row-by-row sweep.
// A workgroup takes kLayRowsPerPass rows at a time (kLayLanesPerRow lanes per
// row); a layer is cut into passes of at most that many rows, and only a
// layer's last pass ends with a barrier.  Not one of the three digested plans
// above: the layers are pinned through kml_code_layers instead.
constexpr int kLayLanesPerRow = 8;                              // lanes that share a row (<= 2 edges each)
constexpr int kLayRowsPerPass = kIrrThreads / kLayLanesPerRow;  // 96

struct LayeredPlan {
  std::vector<int32_t> layer_ptr;  // [nl + 1]: layer l = rows [layer_ptr[l], layer_ptr[l + 1])
  // one word per pass, in sweep order: first row | rows << 16 | (last pass of its layer) << 24
  std::vector<int32_t> pass;
};

// Any code (rows of any degree); the kernel's own limits are the launcher's.
void plan_layered(const LdpcCode &L, LayeredPlan &out);

// Every lane's share of every pass of a plan, for the layered kernels'
// global-table instances (kernels.hpp LnmsItemsDev): two words per entry,
// entry p * kIrrThreads + t = thread t in pass p.  Lane l = t % 8 of row
// g = t / 8 of the pass takes the row's edges l and l + 8: word 0 = their
// columns v0 | v1 << 16 (0xFFFF: no such edge), word 1 = the index of edge l.
// An idle lane holds (0xFFFFFFFF, 0).  Needs E <= 65535 and N < 65535, and row
// degrees <= 16 (false otherwise: the codes the kernels refuse).
bool layered_items(const LdpcCode &L, const LayeredPlan &plan, std::vector<uint32_t> &out);

}  // namespace kml

