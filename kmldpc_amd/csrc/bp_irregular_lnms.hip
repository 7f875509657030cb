// bp_irregular_lnms.hip — the layered schedule of the normalized min-sum mode
// (KML_SCHED_LAYERED, include/kmldpc_amd.h): the sibling of
// bp_irregular_nms.hip for the same codes (5G BG2 K960 among them).  Where the
// flooding kernel runs one VN phase over all columns and one CN phase over all
// rows per iteration, this one keeps one posterior per column and walks the
// rows in index order, each row reading the posteriors the rows before it left.
// tests/bp_lnms_model.py states the arithmetic in numpy and this kernel equals
// it bit for bit.
//
// The arithmetic contract.  Every value is IEEE binary32 with denormals kept,
// no fma (-ffp-contract=off), each operation rounded once; the priors, alpha,
// the +-256 clamp and the tie rule are bp_irregular_nms.hip's:
//   * state: T[v] = L[v] (the prior; +0 for a punctured 5G column), one
//     posterior per column; c2v[e] = +0, one message per edge, row-major;
//   * decisions: hard[v] = T[v] > 0 ? 0 : 1 (a tie decides 1);
//   * loop, it = 0: when every row of hard has even parity, stop (converged);
//     when it == iter_count, stop; otherwise one sweep, it += 1, and again;
//   * sweep: rows r = 0 .. M-1 in index order; for each edge j of r (column
//     v_j): m_j = clamp(T[v_j] - c2v_j, -256, 256); then a_j = min over i != j
//     of |m_i|, s_j = XOR over i != j of the sign bits of m_i (-0 counts as
//     negative), c2v_j = RN(alpha * a_j) with its sign bit set to s_j, and
//     T[v_j] = m_j + c2v_j;
//   * ret = it + (it < max_iter), iters = it (sweeps); iter_count = 0 writes no
//     decisions.
// A budget of k uses all k sweeps: the decisions come from the posteriors the
// last sweep left.  (The flooding schedule's last CN phase is never read; this
// is a deliberate difference between the two schedules.)
// As in the sibling, magnitudes are compared as the integers their bit
// patterns are, and a_j is the row's second minimum on the edges that hold the
// minimum and the minimum elsewhere.  No division, no FAST / EXACT split, no
// redo: CNT_REDONE stays 0.
//
// What runs in parallel.  A layer (layout.hpp LayeredPlan) is a run of
// consecutive rows with pairwise disjoint columns: its rows touch disjoint T
// and c2v entries, so they run at once and give exactly the serial result.
// Mapping: one workgroup of kIrrThreads = 768 per codeword over the dequeue
// counter; kLayLanesPerRow = 8 lanes share a row, lane l takes edges l and
// l + 8 (row degrees <= 10), so a pass is 96 rows: one BG2 layer.  The
// (min1, min2, sign XOR) of a row cross its eight lanes in three DPP steps
// (quad swaps, then the half-row mirror); the sign XOR rides in min1's sign bit.
// A layer longer than a pass takes several, with no barrier between them; one
// barrier closes each layer.  The stop rule is a parity pass over sign(T) in
// the same mapping: a wave's ballot of the lanes' parities folds to one bit
// per row, and wg_any closes it.
// LDS: T (N floats), c2v (E floats), the pass words, 16 bytes of tallies, the
// column of every edge and the row pointers as u16, N decision bytes: 59.5 KB
// for BG2, so two workgroups share a CU.
//
// The global-table instances (kernels.hpp LnmsItemsDev, the pack's last type)
// keep the two code tables out of LDS: every lane's share of every pass comes
// from a table in global memory, one coalesced 8-byte load issued a pass ahead,
// and LDS holds T, c2v, the pass words, the tallies and the decision bytes only
// (160,720 B for BG2's structure at Z = 384, one workgroup a CU).  A launch
// takes them when the tables do not fit, or with KML_LNMS_TABLES=global; they
// compute the same (DESIGN.md "Layered min-sum beyond one CU's round plan").
//
// The offset instances (kml_set_nms_offset, kernels.hpp OmsDev) put two more
// operations behind the multiply: c = RN(c - beta), c = c > 0 ? c : +0, ahead of
// the sign; tests/bp_oms_model.py states them and equals this file's contract at
// beta = 0.  A context with offset 0 launches the instances without them.
#include "bp_common.hpp"
#include "bp_launch.hpp"
#include "exact_math.hpp"
#include "kernels.hpp"

namespace kml {

namespace {

constexpr int kRedBytes = 16;
constexpr unsigned kInfBits = 0x7F800000u;  // above every magnitude: |m| <= 256
constexpr unsigned kSignBit = 0x80000000u;
constexpr float kNmsClamp = 256.0f;
constexpr int kLanes = kLayLanesPerRow;
static_assert(kLanes == 8, "the row reduce below is three DPP steps over eight lanes");

__device__ __forceinline__ unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

// One step of the row reduce: (min1 | sign, min2) meets the partner's under the
// DPP control CTRL; every lane of a row ends with the row's.
template <int CTRL>
__device__ __forceinline__ void row_step(unsigned &x1, unsigned &min2) {
  const unsigned o1 = (unsigned)__builtin_amdgcn_mov_dpp((int)x1, CTRL, 0xF, 0xF, false);
  const unsigned p2 = (unsigned)__builtin_amdgcn_mov_dpp((int)min2, CTRL, 0xF, 0xF, false);
  const unsigned min1 = x1 & ~kSignBit, p1 = o1 & ~kSignBit;
  min2 = umin(umax(min1, p1), umin(min2, p2));
  x1 = umin(min1, p1) | ((x1 ^ o1) & kSignBit);
}

struct LnmsLds {
  float *post;                 // [N] T
  int *c2v;                    // [E] messages as bit patterns, row-major
  const int *pass;             // [npass] layout.hpp LayeredPlan::pass
  const unsigned short *cols;  // [E] column of each edge
  const unsigned short *rowp;  // [M + 1] row pointers
};

// A lane's share of a pass: its row's edges l and l + 8, as the columns v0 / v1
// (kNoCol: no such edge; an edge l + 8 implies an edge l) and the index e0 of
// edge l (edge l + 8 is e0 + 8).  It depends on the code only, so a kernel
// whose passes are few keeps it in registers (LnmsItem per pass).
constexpr unsigned kNoCol = 0xFFFFu;
struct LnmsItem {
  unsigned vv = ~0u;  // v0 | v1 << 16
  int e0 = 0;
};
__device__ __forceinline__ LnmsItem lnms_item(const LnmsLds &s, int first, int nrows, int g, int l) {
  LnmsItem it;
  if (g < nrows) {
    const int b = s.rowp[first + g], d = s.rowp[first + g + 1] - b;
    if (l < d) {
      it.e0 = b + l;
      it.vv = s.cols[b + l] | (l + kLanes < d ? (unsigned)s.cols[b + l + kLanes] : kNoCol) << 16;
    }
  }
  return it;
}

// The global-table instances (kernels.hpp LnmsItemsDev) read the same item,
// made on the host, with one coalesced 8-byte load, and run `f(p, item)` for
// every pass p with the next pass's load in flight across f: the load has no
// address that depends on another load, and by the time a pass needs its item
// the pass before it has hidden the L2 latency.
template <int T>
__device__ __forceinline__ LnmsItem lnms_gt_item(const uint2 *tab, int p, int tid) {
  const uint2 w = tab[p * T + tid];
  return LnmsItem{w.x, (int)w.y};
}
template <int T, class F>
__device__ __forceinline__ void lnms_gt_passes(const uint2 *tab, int npass, int tid, F f) {
  LnmsItem next = lnms_gt_item<T>(tab, 0, tid);
  for (int p = 0; p < npass; ++p) {
    const LnmsItem it = next;
    if (p + 1 < npass) next = lnms_gt_item<T>(tab, p + 1, tid);
    f(p, it);
  }
}

// One pass of a sweep, eight lanes a row.  OMS: the offset correction
// (kernels.hpp OmsDev), c = max(RN(c - beta), +0) ahead of the sign.
template <bool OMS>
__device__ __forceinline__ void lnms_pass(const LnmsLds &s, const LnmsItem &it, float alpha, float beta) {
  const int v0 = (int)(it.vv & 0xFFFFu), v1 = (int)(it.vv >> 16), e0 = it.e0, e1 = it.e0 + kLanes;
  const bool h0 = (unsigned)v0 != kNoCol, h1 = (unsigned)v1 != kNoCol;
  unsigned m0 = kInfBits, m1 = kInfBits;  // (an absent edge: above every magnitude, sign clear)
  if (h0) m0 = (unsigned)__float_as_int(fminf(fmaxf(s.post[v0] - __int_as_float(s.c2v[e0]), -kNmsClamp), kNmsClamp));
  if (h1) m1 = (unsigned)__float_as_int(fminf(fmaxf(s.post[v1] - __int_as_float(s.c2v[e1]), -kNmsClamp), kNmsClamp));
  const unsigned a0 = m0 & ~kSignBit, a1 = m1 & ~kSignBit;
  unsigned x1 = umin(a0, a1) | ((m0 ^ m1) & kSignBit), min2 = umax(a0, a1);
  // every lane runs the reduce: a row's eight lanes are active or idle together
  row_step<0xB1>(x1, min2);   // quad_perm [1,0,3,2]: lane ^ 1
  row_step<0x4E>(x1, min2);   // quad_perm [2,3,0,1]: lane ^ 2
  row_step<0x141>(x1, min2);  // row_half_mirror: lane -> 7 - lane, the other quad
  const unsigned r1 = x1 & ~kSignBit, r2 = min2, rsgn = x1 & kSignBit;
  if (h0) {
    float q = alpha * __int_as_float((int)(a0 == r1 ? r2 : r1));
    if constexpr (OMS) q = fmaxf(q - beta, 0.0f);  // (q - beta is never -0 and never NaN)
    const int cb = (int)((unsigned)__float_as_int(q) | ((m0 ^ rsgn) & kSignBit));
    s.c2v[e0] = cb;
    s.post[v0] = __int_as_float((int)m0) + __int_as_float(cb);
  }
  if (h1) {
    float q = alpha * __int_as_float((int)(a1 == r1 ? r2 : r1));
    if constexpr (OMS) q = fmaxf(q - beta, 0.0f);
    const int cb = (int)((unsigned)__float_as_int(q) | ((m1 ^ rsgn) & kSignBit));
    s.c2v[e1] = cb;
    s.post[v1] = __int_as_float((int)m1) + __int_as_float(cb);
  }
}

// A wave's ballot of its lanes' decision parities holds eight rows, one per
// byte: the rows of odd parity, one bit per byte.
__device__ __forceinline__ unsigned long long lnms_odd_rows(const LnmsLds &s, const LnmsItem &it) {
  const unsigned v0 = it.vv & 0xFFFFu, v1 = it.vv >> 16;
  int bit = 0;
  if (v0 != kNoCol) bit ^= s.post[v0] > 0.0f ? 0 : 1;
  if (v1 != kNoCol) bit ^= s.post[v1] > 0.0f ? 0 : 1;
  unsigned long long x = __ballot(bit);
  x ^= x >> 4;
  x ^= x >> 2;
  x ^= x >> 1;
  return x & 0x0101010101010101ull;
}

// Does any row of the decisions T > 0 ? 0 : 1 have odd parity?  (This thread's
// share: the caller ORs over the workgroup.)  Rows in blocks of T / 8, eight
// lanes a row as in the sweep.
template <int T>
__device__ __forceinline__ bool lnms_parity_fail(const LnmsLds &s, int M, int g, int l) {
  unsigned long long fail = 0;
  for (int first = 0; first < M; first += T / kLanes) fail |= lnms_odd_rows(s, lnms_item(s, first, M - first, g, l));
  return fail != 0;
}

// CACHED: the code has at most kCachePasses passes (BG2: 12) and every lane
// keeps its items in registers; the sweep and the parity pass then read only
// posteriors and messages from LDS.  Otherwise the items come from the LDS
// tables pass by pass.  Both compute the same.
// Six waves per SIMD = two workgroups of 12 waves per CU.
constexpr int kCachePasses = 12;

// The instances without Llr are the P0 front end (the contract above).  With
// one LlrIoDev argument the priors are the caller's floats, clamped to +-256
// (there is no log in those instances), and POST also writes T, as the loop
// left it, out with the decisions taken from it.  With an OmsDev argument (the
// last one) the sweep applies the offset correction.
template <int T, bool CACHED, bool POST = false, class... X>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(6, 6))) void bp_irregular_lnms_kernel(
    DevCode c, BpLaunch a, unsigned int *queue, LnmsPlanDev lp, X... io) {
  constexpr bool LLR = pack_has<LlrIoDev, X...>, OMS = pack_has<OmsDev, X...>;
  constexpr bool GT = pack_has<LnmsItemsDev, X...>;  // the code tables stay in global memory
  static_assert(LLR || !POST, "the posterior output belongs to the LLR instances");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int g = tid / kLanes, l = tid % kLanes;
  float *post = reinterpret_cast<float *>(smem);
  int *c2v = reinterpret_cast<int *>(smem + (size_t)c.N * 4);
  int *pass = c2v + c.E;
  int *red = pass + lp.npass;
  unsigned short *cols = reinterpret_cast<unsigned short *>(red + kRedBytes / 4);
  unsigned short *rowp = cols + c.E;
  unsigned char *cch = reinterpret_cast<unsigned char *>(rowp + c.M + 1);
  if constexpr (GT) cch = reinterpret_cast<unsigned char *>(cols);  // no tables: the decision bytes follow the tallies
  __shared__ WgVotes wflags;  // wg_any (bp_common.hpp)

  if constexpr (!GT) {
    for (int e = tid; e < c.E; e += T) cols[e] = (unsigned short)c.row_col[e];
    for (int r = tid; r <= c.M; r += T) rowp[r] = (unsigned short)c.row_ptr[r];
  }
  for (int p = tid; p < lp.npass; p += T) pass[p] = lp.pass[p];
  const LnmsLds s{post, c2v, pass, GT ? nullptr : cols, GT ? nullptr : rowp};
  const uint2 *gtab = nullptr;
  if constexpr (GT) gtab = pack_get<LnmsItemsDev>(io...).item;
  const float alpha = a.nms_alpha;
  float beta = 0.0f;
  if constexpr (OMS) beta = pack_get<OmsDev>(io...).beta;

  const int B = a.B_dev ? (int)*a.B_dev : a.B;
  for (;;) {
    __syncthreads();
    if (tid == 0) {
      red[3] = (int)atomicAdd(queue, 1u);
      red[0] = 0;
      red[1] = 0;
    }
    __syncthreads();
    const int entry = red[3];
    if (entry >= B) break;
    const int cw = a.cw_idx ? a.cw_idx[entry] : entry;
    if constexpr (LLR) {
      const float *in = pack_get<LlrIoDev>(io...).llr + (long long)cw * a.p0_stride;
      if (a.p0_sel) in += (long long)a.p0_sel[cw] * a.p0_sel_stride;
      for (int v = tid; v < c.N; v += T)  // (a punctured column: +0)
        post[v] = v >= c.punct ? fminf(fmaxf(in[v - c.punct], -kNmsClamp), kNmsClamp) : 0.0f;
    } else {
      const double *p0 = a.p0 + (long long)cw * a.p0_stride;
      if (a.p0_sel) p0 += (long long)a.p0_sel[cw] * a.p0_sel_stride;

      for (int v = tid; v < c.N; v += T) {
        float L = 0.0f;  // a punctured column
        if (v >= c.punct) {
          const double q = fmin(fmax(p0[v - c.punct], kSmallestProb), 1.0 - kSmallestProb);
          L = (float)(kml_log(q) - kml_log(1.0 - q));
        }
        post[v] = L;
      }
    }
    for (int e = tid; e < c.E; e += T) c2v[e] = 0;  // messages start at +0
    // (filled per codeword, after the priors: held across kml_log they would spill)
    LnmsItem item[CACHED ? kCachePasses : 1];
    unsigned last = 0;  // bit p: pass p closes its layer
    if constexpr (CACHED) {
#pragma unroll
      for (int p = 0; p < kCachePasses; ++p)
        if (p < lp.npass) {
          const int w = __builtin_amdgcn_readfirstlane(pass[p]);
          if constexpr (GT)
            item[p] = lnms_gt_item<T>(gtab, p, tid);
          else
            item[p] = lnms_item(s, w & 0xFFFF, (w >> 16) & 0xFF, g, l);
          last |= (unsigned)(w >> 24) << p;
        }
    }
    __syncthreads();

    int iter = 0;
    bool conv = false;
    for (;;) {
      // (wg_any's barrier also keeps the next sweep's writes behind this pass's reads)
      bool fail;
      if constexpr (CACHED) {  // the passes hold every row once
        unsigned long long odd = 0;
#pragma unroll
        for (int p = 0; p < kCachePasses; ++p)
          if (p < lp.npass) odd |= lnms_odd_rows(s, item[p]);
        fail = odd != 0;
      } else if constexpr (GT) {  // ... and so do the table's
        unsigned long long odd = 0;
        lnms_gt_passes<T>(gtab, lp.npass, tid, [&](int, const LnmsItem &it) { odd |= lnms_odd_rows(s, it); });
        fail = odd != 0;
      } else {
        fail = lnms_parity_fail<T>(s, c.M, g, l);
      }
      if (!wg_any<T / 64>(fail, wflags)) {
        conv = true;
        break;
      }
      if (iter == a.iter_count) break;
      if constexpr (CACHED) {
#pragma unroll
        for (int p = 0; p < kCachePasses; ++p)
          if (p < lp.npass) {
            lnms_pass<OMS>(s, item[p], alpha, beta);
            if (last >> p & 1) __syncthreads();  // the layer is complete: the next one reads its posteriors
          }
      } else if constexpr (GT) {
        lnms_gt_passes<T>(gtab, lp.npass, tid, [&](int p, const LnmsItem &it) {
          const int w = __builtin_amdgcn_readfirstlane(pass[p]);
          lnms_pass<OMS>(s, it, alpha, beta);
          if (w >> 24) __syncthreads();
        });
      } else {
        for (int p = 0; p < lp.npass; ++p) {
          const int w = __builtin_amdgcn_readfirstlane(pass[p]);
          lnms_pass<OMS>(s, lnms_item(s, w & 0xFFFF, (w >> 16) & 0xFF, g, l), alpha, beta);
          if (w >> 24) __syncthreads();
        }
      }
      ++iter;
    }

    if (a.iter_count > 0) {
      for (int v = tid; v < c.N; v += T) cch[v] = post[v] > 0.0f ? 0 : 1;
      __syncthreads();
      if (a.uu_hat) {
        uint8_t *u = a.uu_hat + (long long)cw * c.K;
        for (int i = tid; i < c.K; i += T) u[i] = cch[i + c.info_off];
      }
      if (a.cc_hat) {
        uint8_t *o = a.cc_hat + (long long)cw * c.N;
        for (int v = tid; v < c.N; v += T) o[v] = cch[v];
      }
      if constexpr (POST) {  // the posteriors hard was taken from
        float *o = pack_get<LlrIoDev>(io...).post + (long long)cw * c.N;
        for (int v = tid; v < c.N; v += T) o[v] = post[v];
      }
      if (a.parity_cnt) {  // ParityCheck(cc_hat) (:281-300)
        int cnt = 0;
        for (int r = tid; r < c.M; r += T) {
          int p = 0;
          for (int e = c.row_ptr[r]; e < c.row_ptr[r + 1]; ++e) p ^= cch[c.row_col[e]];
          cnt += p;
        }
        if (cnt) atomicAdd(&red[0], cnt);
      }
      if (a.ref_bits) {
        const int errs =
            count_info_errors<T>(cch, nullptr, c.info_off, c.K, c.Kw, a.ref_bits + (long long)cw * c.Kw, tid);
        if (errs) atomicAdd(&red[1], errs);
      }
    }
    __syncthreads();
    if (tid == 0) {
      if (a.ret) a.ret[cw] = iter + (iter < a.max_iter);
      if (a.parity_cnt) a.parity_cnt[cw] = red[0];
      if (a.cw_err && a.ref_bits) a.cw_err[cw] = a.iter_count > 0 ? red[1] : 0;
      if (a.iters) a.iters[cw] = iter;
      if (a.counters) {
        const unsigned long long vn = conv ? (unsigned long long)iter + 1 : (unsigned long long)iter;
        atomicAdd(&a.counters[CNT_VN_PHASES], vn);
        atomicAdd(&a.counters[CNT_CN_PHASES], (unsigned long long)iter);
        if (conv) atomicAdd(&a.counters[CNT_CONVERGED], 1ull);
        if (a.ref_bits && a.iter_count > 0) {
          const int errs = red[1];
          atomicAdd(&a.counters[CNT_ERR_BIT], (unsigned long long)errs);
          atomicAdd(&a.counters[CNT_ERR_BLK], errs > 0 ? 1ull : 0ull);
          atomicAdd(&a.counters[CNT_TOT_BIT], (unsigned long long)c.K);
          atomicAdd(&a.counters[CNT_TOT_BLK], 1ull);
        }
      }
    }
  }
}

size_t lnms_lds_bytes(const DevCode &c, int npass) {
  return (size_t)c.N * 4 + (size_t)c.E * 4 + (size_t)npass * 4 + kRedBytes + (size_t)c.E * 2 +
         ((size_t)c.M + 1) * 2 + (size_t)c.N;
}

// The global-table instances: the same without the two tables.
size_t lnms_gt_lds_bytes(int N, int E, int npass) {
  return (size_t)N * 4 + (size_t)E * 4 + (size_t)npass * 4 + kRedBytes + (size_t)N;
}

}  // namespace

bool lnms_only_shape_ok(int N, int M, int E, int npass) {
  return npass >= 1 && E <= 65535 && M <= 65535 && N < (int)kNoCol &&
         lnms_gt_lds_bytes(N, E, npass) + sizeof(WgVotes) <= kLdsLimit;
}

bool bp_lnms_only_supported(const DevCode &c, int npass) {
  return !bp_irregular_nms_supported(c) && !c.regular && c.irr_ok && c.dc_max <= 2 * kLanes &&
         lnms_only_shape_ok(c.N, c.M, c.E, npass);
}

namespace {
// What both front ends check, and the launch shape they share: the dynamic LDS
// and the workgroups per CU (0: the code or the launch is not this kernel's).
// global: the global-table instance (the caller has its table), taken when the
// LDS-table instance does not fit or KML_LNMS_TABLES=global asks for it.
int lnms_launch_shape(const DevCode &c, const BpLaunch &a, const LnmsPlanDev &lp, bool have_gt, size_t &lds,
                      bool &global) {
  if (!lp.pass || lp.npass < 1) return 0;
  if (!bp_irregular_nms_supported(c) && !bp_lnms_only_supported(c, lp.npass)) return 0;
  if (a.syn || a.cw_prof || a.prof) return 0;  // no syndrom_soft, no profile (launch_bp says why)
  // row degrees <= 2 * kLanes by irr_ok; the 16-bit fields hold E, N and M
  if (c.dc_max > 2 * kLanes || c.E > 65535 || c.N >= (int)kNoCol || c.M > 65535) return 0;
  lds = lnms_lds_bytes(c, lp.npass);
  global = lnms_tables_forced_global() || lds + sizeof(WgVotes) > kLdsLimit;
  if (global) {
    if (!have_gt) return 0;
    lds = lnms_gt_lds_bytes(c.N, c.E, lp.npass);
  }
  if (lds + sizeof(WgVotes) > kLdsLimit) return 0;
  // two workgroups per CU where the LDS holds both (no scratch: DESIGN.md)
  return 2 * (lds + sizeof(WgVotes) + 1024) <= kLdsLimit ? 2 : 1;
}
}  // namespace

// io = NULL: P0 priors; else float priors (io->llr), and the posterior instances
// when io->post is set.  oms: the offset instances (beta > 0), else the plain ones.
hipError_t launch_bp_irregular_lnms(const DevCode &c, const BpLaunch &a, const LnmsPlanDev &lp, const LlrIoDev *io,
                                    const OmsDev *oms, hipStream_t s, const LnmsItemsDev *gt, bool *global_out) {
  constexpr int T = kIrrThreads;
  static_assert(T / kLanes == kLayRowsPerPass, "the plan's passes are this kernel's");
  size_t lds = 0;
  bool global = false;
  const int per_cu = lnms_launch_shape(c, a, lp, gt && gt->item, lds, global);
  if (!per_cu || (io && !io->llr)) return hipErrorNotSupported;
  if (global_out) *global_out = global;
  if (oms && !(oms->beta > 0.0f)) oms = nullptr;
  auto go = [&](auto kern, const auto &...x) {
    return launch_persistent(kern, T, lds, per_cu, kNoGridCap, false, a, s, c, a, a.queue, lp, x...);
  };
  // g: nothing (the LDS-table instances), or the global-table instances' LnmsItemsDev, the pack's last
  auto pick = [&](auto cached, const auto &...g) {
    constexpr bool C = decltype(cached)::value;
    if (!io)
      return oms ? go(bp_irregular_lnms_kernel<T, C, false, OmsDev, std::decay_t<decltype(g)>...>, *oms, g...)
                 : go(bp_irregular_lnms_kernel<T, C, false, std::decay_t<decltype(g)>...>, g...);
    if (io->post)
      return oms ? go(bp_irregular_lnms_kernel<T, C, true, LlrIoDev, OmsDev, std::decay_t<decltype(g)>...>, *io, *oms, g...)
                 : go(bp_irregular_lnms_kernel<T, C, true, LlrIoDev, std::decay_t<decltype(g)>...>, *io, g...);
    return oms ? go(bp_irregular_lnms_kernel<T, C, false, LlrIoDev, OmsDev, std::decay_t<decltype(g)>...>, *io, *oms, g...)
               : go(bp_irregular_lnms_kernel<T, C, false, LlrIoDev, std::decay_t<decltype(g)>...>, *io, g...);
  };
  if (global) return lp.npass <= kCachePasses ? pick(std::true_type{}, *gt) : pick(std::false_type{}, *gt);
  return lp.npass <= kCachePasses ? pick(std::true_type{}) : pick(std::false_type{});
}

}  // namespace kml
