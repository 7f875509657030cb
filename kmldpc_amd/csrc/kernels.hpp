// kernels.hpp — launch interfaces of the gfx950 kernels (host-visible).
//
// Layouts in HBM (B = codewords in the batch, codeword index slowest):
//   y       [B][S] double2      received symbols
//   h       [B] double2         per-codeword channel (true or estimated)
//   p0      [B][cc_len] double  P(bit = 0) from the demapper (decoder input)
//   uu_bits [B][Kw] u64         reference info bits, little-endian bit order
//   cc_bits [B][Cw] u64         transmitted codeword bits
//   uu_hat  [B][K] u8           decoded info bits (optional)
// Decoder message state never leaves the chip for N <= ~9k edges: it lives in
// LDS as one 16-byte slot per edge (see bp.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "layout.hpp"  // kIrrThreads, kIrrVnPairMax, kIrrCnPairMax

namespace kml {

// Device-resident code description (uploaded once per context).
struct DevCode {
  const int32_t *row_ptr, *row_col, *col_ptr, *col_slot, *vn_order, *cn_order;
  const uint64_t *enc_info;
  int M, N, E, K, cc_len, punct, info_off, chk, Kw, dv_max, dc_max, is5g, active;
  int regular;  // every column has degree dv_max and every row dc_max
  int irr_ok;   // column degrees in [1, 9] and row degrees in [2, 10] (bp_irregular.hip)
  // Round plan of bp_irregular.hip (layout.hpp IrregularPlan); null when none fits.
  const int32_t *irr_vn, *irr_cn, *irr_cn_base, *irr_col_slot;
  int irr_slots;
  // LDS placement plan of bp_regular.hip (layout.hpp); null when the code does
  // not take that kernel.  vn_order then holds the planned column order.
  const int32_t *reg_c2v;  // aligned with col_slot: byte offset of the c2v message
  const int32_t *reg_pos;  // column -> position (index into the kernel's hard-decision bytes)
  // Partition plan of the partitioned cooperative kernel (layout.hpp
  // PartitionPlan); null / 0 when the code does not take it.
  const int32_t *pt_vn, *pt_cn, *pt_pos, *pt_vaddr, *pt_xr, *pt_xr_ptr, *pt_xc, *pt_xc_ptr;
  const int32_t *pt_vx, *pt_rx;  // tagged exchange: mailbox index per column edge, per-row (first x, cut mask)
  int pt_G, pt_ncut, pt_mirror;
  int pt_pairs;                // every member receives cut-edge messages from every other member
  int pt_xr_n[8], pt_xc_n[8];  // exchange-list lengths per member (host copy, launch checks)
};

// Counter block in device memory (uint64):
enum {
  CNT_ERR_BIT = 0,
  CNT_ERR_BLK = 1,
  CNT_TOT_BIT = 2,
  CNT_TOT_BLK = 3,
  CNT_VN_PHASES = 4,
  CNT_CN_PHASES = 5,
  CNT_CONVERGED = 6,
  CNT_REDONE = 7,  // FAST decodes redone on the exact path (an unproven quotient, exact_div.hpp)
  CNT_N = 8
};

struct BpLaunch {
  int B = 0;
  int iter_count = 0, max_iter = 0;
  // prec = 2 (below): the normalisation factor of the min-sum CN phase, in
  // (0, 1].  It sits in what was the padding ahead of p0: no field moves and
  // the struct keeps its size, so the existing kernels' code is unchanged.
  float nms_alpha = 0.75f;
  const double *p0 = nullptr;
  long long p0_stride = 0;       // doubles between codewords
  const int32_t *p0_sel = nullptr;  // optional per-codeword candidate: p0 += sel*p0_sel_stride
  long long p0_sel_stride = 0;
  uint8_t *uu_hat = nullptr;     // [B][K]
  int32_t *ret = nullptr;        // [B]  BinaryLDPCCodec::Decoder return value
  uint8_t *cc_hat = nullptr;     // [B][N]
  double *syn = nullptr;         // [B][M] syndrom_soft (written by CN phases only)
  int32_t *parity_cnt = nullptr; // [B] unsatisfied checks of the final cc_hat
  const uint64_t *ref_bits = nullptr;  // [B][Kw] for error counting
  unsigned long long *counters = nullptr;  // [CNT_N]
  int32_t *cw_err = nullptr;     // [B] error bits per codeword vs ref_bits (stop-rule prefix)
  int32_t *iters = nullptr;      // [B] CN phases run (= iter of the reference loop)
  // Entry e of the launch decodes codeword cw_idx[e] (NULL: e); every
  // per-codeword array above is indexed by the codeword, B counts entries.
  const int32_t *cw_idx = nullptr;
  const unsigned *B_dev = nullptr;  // when set, the entry count is *B_dev (<= B), read on the device
  // partitioned kernel's tagged launch: codewords it leaves to the barrier-exchange launch
  int32_t *defer_idx = nullptr;
  unsigned *defer_cnt = nullptr;
  // Cooperative global-slot kernel (bp_coop.hip): per-group sync blocks
  // (bp_coop_sync_bytes) and per-group hard-decision bytes (groups x N).
  void *gsync = nullptr;
  uint8_t *gcch = nullptr;
  double2 *gslots = nullptr;     // global slot scratch when E*16 exceeds LDS
  long long gslots_cap = 0;      // number of double2 available
  unsigned int *queue = nullptr; // 4-byte device dequeue counter (zeroed by the launcher)
  // Cooperative kernels: clear the abort word before the launch.  The caller
  // clears it only for the first launch after the last check (context.cpp sync),
  // so a timeout in an earlier launch of the same API call stays visible.
  bool reset_abort = true;
  // Fused demap (bp_regular.hip only, bp_regular_fuses_demap): when sym_y is
  // set, p0 is ignored and each codeword's P0 is computed in the kernel's
  // prologue from y[B][S] and the known channel h[B] (demap_common.hpp).
  const double2 *sym_y = nullptr;
  const double2 *sym_h = nullptr;     // h of codeword cw: sym_h[cw * sym_h_stride + (sym_h_sel ? sym_h_sel[cw] : 0)]
  int sym_h_stride = 1;
  const int32_t *sym_h_sel = nullptr;  // chosen candidate (blind path)
  const double *sym_cons = nullptr;  // the normalised constellation, 2 << bits doubles
  double sym_var = 0;
  int sym_bits = 0;
  // 0: the bit-exact fp64 kernels; 1: the single-precision kernel
  // (bp_regular_f32.hip, PEG2304-class codes only; launch_bp fails for any
  // other code, there is no fallback in either direction); 2: the normalized
  // min-sum kernel (bp_irregular_nms.hip, the codes of bp_irregular.hip only,
  // nms_alpha above; the same rule); 3: its layered schedule
  // (bp_irregular_lnms.hip, the same codes, nms_alpha, launch_bp's lnms plan);
  // 4: the layered schedule on binary16 messages (bp_irregular_lnms_h16.hip,
  // the same codes, plan and rule)
  int prec = 0;
  // Iteration profile (bp_regular.hip / bp_irregular.hip only, SYN = false,
  // ref_bits set, 1 <= iter_count <= kBpProfMaxIter): when either is set the
  // launch runs the PROF kernels, which count the info-bit errors of every
  // iteration's decisions and report, for every budget k = 1..iter_count, what
  // a decode with iter_count = k would have counted on the same codeword:
  //   cw_prof[cw * cw_prof_stride + k-1] = error bits at budget k
  //   prof[(k-1) * 3 + {0, 1, 2}]       += {error bits, codewords in error, converged} at budget k
  // Any other kernel family answers hipErrorNotSupported (launch_bp: no fallback).
  int32_t *cw_prof = nullptr;
  long long cw_prof_stride = 0;
  unsigned long long *prof = nullptr;
};
// The kernels take BpLaunch by value, so its layout is part of their code; the
// arguments that follow it (queue, fast_allowed, ...) sit behind its size.
static_assert(sizeof(BpLaunch) == 280 && offsetof(BpLaunch, p0) == 16 && offsetof(BpLaunch, prof) == 272,
              "BpLaunch layout changed: every BP kernel's kernarg offsets move with it");

constexpr int kBpProfMaxIter = 64;  // budgets of a profile launch (static LDS: perr + wprof, 1792 B)

// FAST-path mode of a BP launch: bit 0 = FAST division allowed (column degree
// <= kFastMaxColumnDegree, and not KML_NO_FAST=1: every codeword on the
// exact path); bit 1 = KML_FORCE_REDO=1 (tests: every FAST decode is treated
// as suspect and redone on the exact path, exercising the redo machinery).
int bp_fast_mode(const DevCode &c);
// Why a profile launch (BpLaunch::cw_prof / prof) with this budget cannot run
// for this code, or NULL when it can: the host-side check callers make before
// they launch anything (launch_bp repeats it).
const char *bp_profile_refusal(const DevCode &c, int iter_count);
hipError_t launch_bp_regular(const DevCode &c, const BpLaunch &a, hipStream_t s);
// Can the regular kernel compute P0 itself (BpLaunch::sym_y) for this code and modem?
bool bp_regular_fuses_demap(const DevCode &c, int bits);
// The single-precision sibling (BpLaunch::prec = 1) and whether this code takes it.
hipError_t launch_bp_regular_f32(const DevCode &c, const BpLaunch &a, hipStream_t s);
bool bp_regular_f32_supported(const DevCode &c);
hipError_t launch_bp_irregular(const DevCode &c, const BpLaunch &a, hipStream_t s);
// The normalized min-sum sibling (BpLaunch::prec = 2) and whether this code
// takes it: the codes of launch_bp_irregular whose min-sum state fits in LDS.
// (the launcher is declared with its optional arguments, below)
bool bp_irregular_nms_supported(const DevCode &c);
// The layered min-sum sibling (BpLaunch::prec = 3, bp_irregular_lnms.hip): the
// codes of launch_bp_irregular_nms.  Its layer plan (layout.hpp LayeredPlan)
// travels as a kernel argument of its own: DevCode and BpLaunch are part of the
// existing kernels' code and neither grows.
struct LnmsPlanDev {
  const int32_t *pass = nullptr;  // LayeredPlan::pass, device copy
  int npass = 0;
};
// The LLR front end of the two min-sum kernels (prec = 2 and 3 only): float
// priors in place of BpLaunch::p0, with p0's addressing (p0_stride and
// p0_sel_stride then count floats; p0_sel and cw_idx as they are), and an
// optional posterior output.  Like LnmsPlanDev it travels as a kernel argument
// of its own, and only the instances that read it take it: BpLaunch, DevCode
// and the existing instances' kernarg segments stay as they are.
struct LlrIoDev {
  const float *llr = nullptr;  // priors: L[v] = min(max(llr[v - punct], -256), 256), +0 for a punctured column
  float *post = nullptr;       // [B][N] posteriors the decisions were taken from (optional; iter_count = 0 writes none)
};
// The offset correction of the three min-sum kernels (kml_set_nms_offset): after
// c = RN(alpha * a_j) the offset instances run c = RN(c - beta), c = c > 0 ? c
// : +0 (binary16 in the h16 kernel, with beta rounded once more to binary16).
// Like LlrIoDev it travels as a kernel argument of its own, behind LlrIoDev
// where both are present, and only the offset instances take it.  oms = NULL
// (or beta = 0) launches the instances without it.
struct OmsDev {
  float beta = 0.0f;  // > 0
};
// The global-table instances of the two layered kernels (DESIGN.md "Layered
// min-sum beyond one CU's round plan"): the code tables stay in global memory
// and LDS holds the decoder state only.  The table is every lane's share of
// every pass, made once on the host (layout.hpp layered_items): entry
// p * kIrrThreads + tid = (v0 | v1 << 16, e0) of thread tid in pass p, so a pass
// costs a lane one coalesced 8-byte load with no address that depends on
// another load.  Like LlrIoDev it travels as a kernel argument of its own, the
// last one, and only the global-table instances take it.
struct LnmsItemsDev {
  const uint2 *item = nullptr;  // [npass * kIrrThreads]
};
// The optional arguments of a min-sum kernel are a pack of the types above:
// which are present picks the instance, and the kernel reads them by type.
template <class W, class... A>
constexpr bool pack_has = (std::is_same_v<W, A> || ...);
template <class W, class A0, class... A>
__device__ __forceinline__ const W &pack_get(const A0 &a0, const A &...a) {
  if constexpr (std::is_same_v<W, A0>)
    return a0;
  else
    return pack_get<W>(a...);
}
hipError_t launch_bp_irregular_nms(const DevCode &c, const BpLaunch &a, const LlrIoDev *io, const OmsDev *oms,
                                   hipStream_t s);
// Does the flooding kernel's posterior instance (N more floats of LDS) fit this code?
bool bp_irregular_nms_post_supported(const DevCode &c);
// gt: the global-table instances' table, or NULL (then only the LDS-table
// instances can run).  A launch takes the LDS-table instance when its LDS fits
// and KML_LNMS_TABLES=global is not set, the global-table instance otherwise;
// global_out (optional) says which it was.
hipError_t launch_bp_irregular_lnms(const DevCode &c, const BpLaunch &a, const LnmsPlanDev &lp, const LlrIoDev *io,
                                    const OmsDev *oms, hipStream_t s, const LnmsItemsDev *gt = nullptr,
                                    bool *global_out = nullptr);
// The "layered-only" codes: not bp_irregular_nms_supported (no round plan of
// bp_irregular_kernel, or its LDS does not fit), yet irregular with irr_ok,
// E, M <= 65535, N < 65535 (the 16-bit fields of the pass words and the
// items), and the global-table instance's LDS (the decoder state of a code
// with npass passes) within one CU.  Both layered kernels take them; the
// flooding kernel does not.
bool bp_lnms_only_supported(const DevCode &c, int npass);
// The same rule on plain numbers, for the host plan of a context without a GPU.
bool lnms_only_shape_ok(int N, int M, int E, int npass);
// KML_LNMS_TABLES=global (read once per process): every layered launch takes
// the global-table instance.
bool lnms_tables_forced_global();
// The binary16 message format of the layered kernel (BpLaunch::prec = 4,
// bp_irregular_lnms_h16.hip): the codes, the layer plan and the launch rules of
// launch_bp_irregular_lnms; two codewords a workgroup, one in each half of a
// 32-bit word.  io = NULL: P0 priors; else float priors (and posteriors out
// when io->post is set), as above.
hipError_t launch_bp_irregular_lnms_h16(const DevCode &c, const BpLaunch &a, const LnmsPlanDev &lp,
                                        const LlrIoDev *io, const OmsDev *oms, hipStream_t s,
                                        const LnmsItemsDev *gt = nullptr, bool *global_out = nullptr);
// KML_BP_KERNEL=generic (read now, and as the dispatch first read it).
bool bp_generic_forced();
// Cooperative kernel for regular codes whose slots exceed the LDS: groups of
// workgroups on one XCD share a codeword.  0 groups = not applicable.
int bp_coop_groups(const DevCode &c);
size_t bp_coop_sync_bytes(int groups);
hipError_t launch_bp_coop(const DevCode &c, const BpLaunch &a, hipStream_t s);
// Group size of the partitioned cooperative kernel (0: not used); host-side,
// decides whether upload_code builds the partition plan.
int bp_part_group_size(int N, int M, int E, int dv_max, int dc_max, int regular);
// Does a partition plan (cut edges, most mirror slots of a member, longest
// exchange list) fit the partitioned kernel's LDS, scratch and tilings?
bool part_plan_fits(int G, int N, int M, int E, int ncut, int mirror_max, int xmax);
// Name of the cooperative kernel launch_bp_coop runs for this code.
const char *bp_coop_family(const DevCode &c);
bool bp_coop_aborted(const BpLaunch &a, int groups, hipStream_t s, unsigned *why = nullptr);
// Test hook: set the abort word on the stream, as a timed-out group barrier would.
hipError_t bp_coop_raise_abort(const BpLaunch &a, int groups, hipStream_t s);
// Threads per workgroup of the regular kernel for this code shape, 0 if it does
// not apply (host-side; decides whether upload_code builds the LDS plan).
int bp_regular_threads(int N, int M, int E, int dv_max, int dc_max, int regular);
// family (optional) receives the name of the kernel that was launched.
// lnms: the layer plan, read by prec = 3 only (which fails without one).
// llr: the LLR front end (prec = 2 and 3 only; any other prec fails with it).
// oms: the offset correction (the min-sum precs only; any other prec fails with it).
// gt: the layered kernels' global-table instances (prec = 3 and 4 read it; their
// family is then "bp_irregular_lnms_gt_kernel" / "bp_irregular_lnms_h16_gt_kernel").
hipError_t launch_bp(const DevCode &c, const BpLaunch &a, hipStream_t s, const char **err,
                     const char **family = nullptr, const LnmsPlanDev *lnms = nullptr, const LlrIoDev *llr = nullptr,
                     const OmsDev *oms = nullptr, const LnmsItemsDev *gt = nullptr);
// Workspace the BP launcher needs in global-slot mode (double2 elements).
long long bp_gslots_needed(const DevCode &c);
bool bp_uses_lds(const DevCode &c);

// The FAST demappers' defer list (demap.hip): symbol indices (launch_demap,
// any cap; past it the exact pass scans for the sentinel) or codewords
// (launch_cand_metric, cap >= B), and their device-side count.
struct DemapDefer {
  int32_t *idx = nullptr;
  unsigned *cnt = nullptr;
  int cap = 0;
};
// SoftAWGNDemodulation + Modem::DeMapping with bitLin = 0.5, for `n` entries:
// entry e reads y row e / reps and channel h[e * h_stride + (h_sel ? h_sel[e] : 0)],
// writes p0 row e.  (reps = 4, h_stride = 1 demaps the 4 blind candidates.)
hipError_t launch_demap(int bits, const double *cons, const double2 *y, int S, int reps, const double2 *h,
                        int h_stride, const int32_t *h_sel, double var, int n, double *p0, const DemapDefer &d,
                        hipStream_t s);

// The max-log demapper (demap_llr.hip): launch_demap's addressing (entry e
// reads y row e / reps and channel h[e * h_stride + (h_sel ? h_sel[e] : 0)]),
// float LLRs out, llr row e of S * bits floats.  inv = (float)(1.0 / var).
hipError_t launch_demap_llr(int bits, const double *cons, const double2 *y, int S, int reps, const double2 *h,
                            int h_stride, const int32_t *h_sel, float inv, int n, float *llr, hipStream_t s);

// Hard-metric candidates for the PEG blind path (kmcodec.cc:105-119):
// for each codeword and each of its nc (1 or 4) channel estimates h4[b][j], the
// number of unsatisfied checks of rr = (P0 > 0.5).  metrics[b][4] doubles
// (entries >= nc zeroed), chosen[b] = first argmin.
hipError_t launch_cand_metric(const DevCode &c, int bits, const double *cons, const double2 *y, int S,
                              const double2 *h4, int nc, double var, int B, double *metrics, int32_t *chosen,
                              const DemapDefer &d, hipStream_t s);
// argmin over a [B][nc] parity-count table (first minimum) for the BP-based
// metrics; metrics[b][4] = |count|.
hipError_t launch_select(const int32_t *parity_cnt, int nc, int B, double *metrics, int32_t *chosen, hipStream_t s);
// Soft syndrome metric sums: L[e] = sum_j log(syn[e][j]) in row order, for
// e = list[i] (or i), i < n; skipped where iters[e] == 0.
hipError_t launch_soft_sum(const double *syn, int M, const int32_t *iters, const int32_t *list, int n, double *L,
                           hipStream_t s);
// CntErr of byte decisions (uh == NULL: all-zero decisions) against packed
// reference bits; optional per-codeword error bits.
hipError_t launch_count_packed(const uint64_t *ref, int Kw, int K, const uint8_t *uh, long long uh_stride, int B,
                               int32_t *cw_err, unsigned long long *counters, hipStream_t s);

// KMeans::Run + h_hat = clusters[0]/c[0] + 4 rotations (kmeans.hip).
struct KmState {
  double2 hat, prev, sum;  // current h_hat, previous iteration's, cumulative cluster-0 sum
  int cnt, it, done, have_prev;
};
size_t kmeans_workspace_bytes(int S, int B);
// hat_out (optional): the final hatH per codeword (clusters_ = c[k] * hatH).
hipError_t launch_kmeans(int Kc, const double *cons, const double *rot, const double2 *y, int S, int iters, int B,
                         double2 *h_hat, double2 *h4, void *ws, hipStream_t s, double2 *hat_out = nullptr);
// KMeans::clusters() / idx() from the final hatH (kmeans.cc:72-83): clusters[B][Kc], idx[B][S] (either may be null).
hipError_t launch_kmeans_state(int Kc, const double *cons, const double2 *y, int S, int B, const double2 *hat,
                               double2 *clusters, int *idx, hipStream_t s);

// GPU frame generation (counter-based Philox; statistically equivalent to the
// reference's sequential Park-Miller stream, not bit-equal).
struct FrameLaunch {
  int B = 0;
  unsigned long long seed = 0, first_cw = 0;
  double noise_scale = 0;
  uint64_t *uu_bits = nullptr;  // [B][Kw]
  uint64_t *cc_bits = nullptr;  // [B][Cw]
  double2 *y = nullptr;         // [B][S]
  double2 *h = nullptr;         // [B]
};
hipError_t launch_framegen(const DevCode &c, int bits, const double *cons, const FrameLaunch &f, hipStream_t s);

// Count mismatching bits: uu_hat bytes vs reference bits (SourceSink::CntErr).
hipError_t launch_count_bytes(const uint8_t *uu, const uint8_t *uu_hat, int K, int B, unsigned long long *counters,
                              hipStream_t s);

// Device-side self tests of the exact-math helpers (hypot, complex division).
hipError_t launch_math_probe(const double *in, int n, double *out, hipStream_t s);
hipError_t launch_log_probe(const double *in, int n, double *out, hipStream_t s);
// Device-side self test of the shared-reciprocal division (bp_common.hpp):
// in[n][3] = (n0, n1, s) -> out[n][4] = (fast q0, fast q1, IEEE q0, IEEE q1).
hipError_t launch_div_probe(const double *in, int n, double *out, hipStream_t s);

}  // namespace kml
