// bp_irregular_lnms_h16.hip — the binary16 message format of the layered
// min-sum decoder (KML_MSG_F16, include/kmldpc_amd.h): the sibling of
// bp_irregular_lnms.hip for the same codes, the same layer plan and the same
// mapping, with every value of the decoder state an IEEE binary16 and every
// 32-bit word holding the same value of TWO codewords.  tests/bp_h16_model.py
// states the arithmetic in numpy and this kernel equals it bit for bit.
//
// The arithmetic contract is bp_irregular_lnms.hip's with binary16 in place of
// binary32 (denormals kept: the code object's float_denorm_mode_16_64 is 3; no
// fma; each operation rounded once to nearest-even):
//   * prior: the float L of that contract (P0: (float)(log q - log(1 - q));
//     LLR: min(max(x, -256.0f), 256.0f)), rounded once to binary16; +0 for a
//     punctured column;  alpha: a16 = RN16((float)alpha);
//   * sweep, per edge j of a row: m_j = clamp(T[v_j] - c2v_j, -256, 256); a_j =
//     min over i != j of |m_i| (compared as the integers their 15-bit patterns
//     are), s_j = XOR over i != j of the sign bits; c2v_j = RN16(a16 * a_j) with
//     its sign bit set to s_j; T[v_j] = m_j + c2v_j — one packed instruction each;
//   * decisions T > 0 ? 0 : 1, the stop rule, ret, iters and the counters are
//     the f32 kernel's; the posterior output is T widened to float (exact).
//
// Two codewords a word.  A workgroup takes two queue entries at a time: entry
// 2q sits in the low halves, entry 2q + 1 in the high halves of T[N] and
// c2v[E] (4 bytes per entry, as in the f32 kernel).  A half's arithmetic never
// reads the other half: packed f16 / u16 instructions and 32-bit bit operations
// under the mask 0x80008000 only, so a codeword's result does not depend on its
// partner.  The row reduce carries (min1 | sign, min2) of both halves through
// the f32 kernel's three DPP steps; a_j = min1 + min2 - min(|m_j|, min2) picks
// the second minimum on the edges that hold the minimum without a per-half
// select (no carry crosses: min1 + min2 <= 2 * 0x7C00 < 2^16).
//
// Two stopping times.  The parity pass votes per half (wg_any2).  At the loop
// top where a half first passes, or where the budget ends, that half is
// RECORDED: the whole epilogue of the f32 kernel runs for it there and then
// (decisions, outputs, parity count, error count, ret, iters, counters, all
// from its own T and its own sweep count).  The loop goes on until both halves
// are recorded; a recorded half's lanes keep computing (the clamp keeps every
// value finite, |T| <= 512) and nothing of it is written out again.  Recording
// on the spot needs no second set of decision bytes and no copy of T in LDS:
// the footprint is the f32 kernel's, 59.5 KB for BG2, two workgroups a CU.
// An odd batch leaves the last pair with one live half; the dead one starts
// recorded, with priors +0, writes nothing and counts nothing.
//
// The offset instances (kml_set_nms_offset, kernels.hpp OmsDev) put two more
// operations behind the multiply: c = RN16(c - b16), b16 = RN16(beta), c = c > 0 ? c : +0, ahead of
// the sign; tests/bp_oms_model.py states them and equals this file's contract at
// beta = 0.  A context with offset 0 launches the instances without them.
#include "bp_common.hpp"
#include "bp_launch.hpp"
#include "exact_math.hpp"
#include "kernels.hpp"

namespace kml {

namespace {

typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef unsigned short us2 __attribute__((ext_vector_type(2)));

constexpr int kRedBytes = 16;
constexpr unsigned kInf2 = 0x7C007C00u;   // above every magnitude: |m| <= 256 = 0x5C00
constexpr unsigned kSign2 = 0x80008000u;
constexpr float kNmsClamp = 256.0f;
constexpr int kLanes = kLayLanesPerRow;
static_assert(kLanes == 8, "the row reduce below is three DPP steps over eight lanes");

__device__ __forceinline__ h2 as_h2(unsigned x) { return __builtin_bit_cast(h2, x); }
__device__ __forceinline__ unsigned as_u(h2 x) { return __builtin_bit_cast(unsigned, x); }
__device__ __forceinline__ unsigned pk_min(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
__device__ __forceinline__ unsigned pk_max(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}
__device__ __forceinline__ unsigned pk_add(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, (us2)(__builtin_bit_cast(us2, a) + __builtin_bit_cast(us2, b)));
}
__device__ __forceinline__ unsigned pk_sub(unsigned a, unsigned b) {
  return __builtin_bit_cast(unsigned, (us2)(__builtin_bit_cast(us2, a) - __builtin_bit_cast(us2, b)));
}
// m = clamp(t - c, -256, 256), both halves
__device__ __forceinline__ unsigned pk_msg(unsigned t, unsigned c) {
  const h2 lo = {(_Float16)-kNmsClamp, (_Float16)-kNmsClamp}, hi = {(_Float16)kNmsClamp, (_Float16)kNmsClamp};
  return as_u(__builtin_elementwise_min(__builtin_elementwise_max(as_h2(t) - as_h2(c), lo), hi));
}
// the decision of half H of a posterior word: T > 0 ? 0 : 1 (no NaN is ever stored)
template <int H>
__device__ __forceinline__ int hard_of(unsigned t) {
  return (H ? (int)t >> 16 : (int)(short)(t & 0xFFFFu)) > 0 ? 0 : 1;
}
template <int H>
__device__ __forceinline__ float half_of(unsigned t) {
  return (float)(H ? as_h2(t).y : as_h2(t).x);
}

// One step of the row reduce: (min1 | sign, min2) of both halves meet the
// partner lane's under the DPP control CTRL.
template <int CTRL>
__device__ __forceinline__ void row_step(unsigned &x1, unsigned &min2) {
  const unsigned o1 = (unsigned)__builtin_amdgcn_mov_dpp((int)x1, CTRL, 0xF, 0xF, false);
  const unsigned p2 = (unsigned)__builtin_amdgcn_mov_dpp((int)min2, CTRL, 0xF, 0xF, false);
  const unsigned min1 = x1 & ~kSign2, p1 = o1 & ~kSign2;
  min2 = pk_min(pk_max(min1, p1), pk_min(min2, p2));
  x1 = pk_min(min1, p1) | ((x1 ^ o1) & kSign2);
}

struct LnmsLds {
  unsigned *post;              // [N] T, two halves a word
  unsigned *c2v;               // [E] messages, row-major, two halves a word
  const int *pass;             // [npass] layout.hpp LayeredPlan::pass
  const unsigned short *cols;  // [E] column of each edge
  const unsigned short *rowp;  // [M + 1] row pointers
};

// A lane's share of a pass, as in bp_irregular_lnms.hip: its row's edges l and
// l + 8 as the columns v0 / v1 (kNoCol: no such edge) and the index e0 of edge l.
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

// The global-table instances' item and pass loop, as in bp_irregular_lnms.hip:
// one coalesced 8-byte load per lane and pass, the next pass's in flight
// across f(p, item).
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

// c2v magnitudes of both halves: RN16(alpha * a), and with OMS the offset
// correction (kernels.hpp OmsDev) in binary16: a packed subtract, then a packed
// max with +0 (its operand is never -0: x - x is +0 in round-to-nearest).
template <bool OMS>
__device__ __forceinline__ unsigned pk_c2v(h2 alpha, h2 beta, unsigned a) {
  h2 q = alpha * as_h2(a);
  if constexpr (OMS) {
    const h2 zero = {(_Float16)0.0f, (_Float16)0.0f};
    q = __builtin_elementwise_max(q - beta, zero);
  }
  return as_u(q);
}

// One pass of a sweep, eight lanes a row, two codewords a lane.
template <bool OMS>
__device__ __forceinline__ void lnms_pass(const LnmsLds &s, const LnmsItem &it, h2 alpha, h2 beta) {
  const int v0 = (int)(it.vv & 0xFFFFu), v1 = (int)(it.vv >> 16), e0 = it.e0, e1 = it.e0 + kLanes;
  const bool h0 = (unsigned)v0 != kNoCol, h1 = (unsigned)v1 != kNoCol;
  unsigned m0 = kInf2, m1 = kInf2;  // (an absent edge: above every magnitude, signs clear)
  if (h0) m0 = pk_msg(s.post[v0], s.c2v[e0]);
  if (h1) m1 = pk_msg(s.post[v1], s.c2v[e1]);
  const unsigned a0 = m0 & ~kSign2, a1 = m1 & ~kSign2;
  unsigned x1 = pk_min(a0, a1) | ((m0 ^ m1) & kSign2), min2 = pk_max(a0, a1);
  // every lane runs the reduce: a row's eight lanes are active or idle together
  row_step<0xB1>(x1, min2);   // quad_perm [1,0,3,2]: lane ^ 1
  row_step<0x4E>(x1, min2);   // quad_perm [2,3,0,1]: lane ^ 2
  row_step<0x141>(x1, min2);  // row_half_mirror: lane -> 7 - lane, the other quad
  const unsigned r2 = min2, rsgn = x1 & kSign2, rsum = pk_add(x1 & ~kSign2, r2);
  if (h0) {
    const unsigned q = pk_c2v<OMS>(alpha, beta, pk_sub(rsum, pk_min(a0, r2)));  // min2 where a0 holds min1, min1 elsewhere
    const unsigned cb = q | ((m0 ^ rsgn) & kSign2);
    s.c2v[e0] = cb;
    s.post[v0] = as_u(as_h2(m0) + as_h2(cb));
  }
  if (h1) {
    const unsigned q = pk_c2v<OMS>(alpha, beta, pk_sub(rsum, pk_min(a1, r2)));
    const unsigned cb = q | ((m1 ^ rsgn) & kSign2);
    s.c2v[e1] = cb;
    s.post[v1] = as_u(as_h2(m1) + as_h2(cb));
  }
}

// The parity pass, both halves at once.  dec2 puts a word's two decisions
// (T > 0 ? 0 : 1) into bits 15 and 31: the saturating t - 1 of a 16-bit pattern
// read as a signed integer is negative exactly where t <= 0, and a half is
// positive exactly where its pattern is (-0 = 0x8000 saturates, stays negative).
// A lane XORs its edges' words, three DPP steps XOR the row's eight lanes, and
// the rows of the passes are ORed: bits 15 / 31 of the result say whether a row
// of half 0 / 1 seen by this lane has odd parity.
typedef short s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned dec2(unsigned t) {
  const s2 one = {1, 1};
  return __builtin_bit_cast(unsigned, __builtin_elementwise_sub_sat(__builtin_bit_cast(s2, t), one));
}
template <int CTRL>
__device__ __forceinline__ unsigned xor_step(unsigned x) {
  return x ^ (unsigned)__builtin_amdgcn_mov_dpp((int)x, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ unsigned lnms_odd_rows(const LnmsLds &s, const LnmsItem &it) {
  const unsigned v0 = it.vv & 0xFFFFu, v1 = it.vv >> 16;
  unsigned x = 0;
  if (v0 != kNoCol) x = dec2(s.post[v0]);
  if (v1 != kNoCol) x ^= dec2(s.post[v1]);
  x = xor_step<0xB1>(x);
  x = xor_step<0x4E>(x);
  return xor_step<0x141>(x);
}

constexpr int kCachePasses = 12;  // as in bp_irregular_lnms.hip: BG2's passes live in registers

// What a recorded half reports (the f32 kernel's epilogue, from half H of T).
template <int T, int H, bool POST, class... X>
__device__ __forceinline__ void lnms_record(const DevCode &c, const BpLaunch &a, const LnmsLds &s, unsigned char *cch,
                                            int *red, int cw, int iter, bool conv, int tid, const X &...io) {
  if (a.iter_count > 0) {
    for (int v = tid; v < c.N; v += T) cch[v] = (unsigned char)hard_of<H>(s.post[v]);
    __syncthreads();
    if (a.uu_hat) {
      uint8_t *u = a.uu_hat + (long long)cw * c.K;
      for (int i = tid; i < c.K; i += T) u[i] = cch[i + c.info_off];
    }
    if (a.cc_hat) {
      uint8_t *o = a.cc_hat + (long long)cw * c.N;
      for (int v = tid; v < c.N; v += T) o[v] = cch[v];
    }
    if constexpr (POST) {  // the posteriors hard was taken from, widened
      float *o = pack_get<LlrIoDev>(io...).post + (long long)cw * c.N;
      for (int v = tid; v < c.N; v += T) o[v] = half_of<H>(s.post[v]);
    }
    if (a.parity_cnt) {
      int cnt = 0;
      for (int r = tid; r < c.M; r += T) {
        int p = 0;
        if constexpr (pack_has<LnmsItemsDev, X...>) {  // no tables in LDS: the graph as uploaded
          for (int e = c.row_ptr[r]; e < c.row_ptr[r + 1]; ++e) p ^= cch[c.row_col[e]];
        } else {
          for (int e = s.rowp[r]; e < s.rowp[r + 1]; ++e) p ^= cch[s.cols[e]];
        }
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
    red[0] = 0;  // for the partner's record
    red[1] = 0;
  }
  __syncthreads();  // cch and the tallies are free again; the next sweep may write T
}

// The float prior of column v >= punct of one codeword, before the rounding to half.
template <bool LLR, class... X>
__device__ __forceinline__ const void *prior_row(const BpLaunch &a, int cw, const X &...io) {
  if constexpr (LLR) {
    const float *in = pack_get<LlrIoDev>(io...).llr + (long long)cw * a.p0_stride;
    if (a.p0_sel) in += (long long)a.p0_sel[cw] * a.p0_sel_stride;
    return in;
  } else {
    const double *p0 = a.p0 + (long long)cw * a.p0_stride;
    if (a.p0_sel) p0 += (long long)a.p0_sel[cw] * a.p0_sel_stride;
    return p0;
  }
}
template <bool LLR>
__device__ __forceinline__ _Float16 prior_of(const void *row, int i) {
  if constexpr (LLR) {
    return (_Float16)fminf(fmaxf(static_cast<const float *>(row)[i], -kNmsClamp), kNmsClamp);
  } else {
    const double q = fmin(fmax(static_cast<const double *>(row)[i], kSmallestProb), 1.0 - kSmallestProb);
    return (_Float16)(float)(kml_log(q) - kml_log(1.0 - q));  // to float first, then to half
  }
}

// The instances are bp_irregular_lnms_kernel's: P0 priors without Llr, float
// priors with one LlrIoDev argument, POST also writes the recorded T; CACHED
// keeps the passes' items in registers (at most kCachePasses passes); with an
// OmsDev argument (the last one) the sweep applies the offset correction.
// Six waves per SIMD = two workgroups of 12 waves per CU.
template <int T, bool CACHED, bool POST = false, class... X>
__global__ __launch_bounds__(T) __attribute__((amdgpu_waves_per_eu(6, 6))) void bp_irregular_lnms_h16_kernel(
    DevCode c, BpLaunch a, unsigned int *queue, LnmsPlanDev lp, X... io) {
  constexpr bool LLR = pack_has<LlrIoDev, X...>, OMS = pack_has<OmsDev, X...>;
  constexpr bool GT = pack_has<LnmsItemsDev, X...>;  // the code tables stay in global memory
  static_assert(LLR || !POST, "the posterior output belongs to the LLR instances");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int g = tid / kLanes, l = tid % kLanes;
  unsigned *post = reinterpret_cast<unsigned *>(smem);
  unsigned *c2v = post + c.N;
  int *pass = reinterpret_cast<int *>(c2v + c.E);
  int *red = pass + lp.npass;
  unsigned short *cols = reinterpret_cast<unsigned short *>(red + kRedBytes / 4);
  unsigned short *rowp = cols + c.E;
  unsigned char *cch = reinterpret_cast<unsigned char *>(rowp + c.M + 1);
  if constexpr (GT) cch = reinterpret_cast<unsigned char *>(cols);  // no tables: the decision bytes follow the tallies
  __shared__ WgVotes wflags;  // wg_any2 (bp_common.hpp)

  if constexpr (!GT) {
    for (int e = tid; e < c.E; e += T) cols[e] = (unsigned short)c.row_col[e];
    for (int r = tid; r <= c.M; r += T) rowp[r] = (unsigned short)c.row_ptr[r];
  }
  for (int p = tid; p < lp.npass; p += T) pass[p] = lp.pass[p];
  const LnmsLds s{post, c2v, pass, GT ? nullptr : cols, GT ? nullptr : rowp};
  const uint2 *gtab = nullptr;
  if constexpr (GT) gtab = pack_get<LnmsItemsDev>(io...).item;
  const _Float16 a16 = (_Float16)a.nms_alpha;
  const h2 alpha = {a16, a16};
  h2 beta = {(_Float16)0.0f, (_Float16)0.0f};
  if constexpr (OMS) {
    const _Float16 b16 = (_Float16)pack_get<OmsDev>(io...).beta;  // RN16
    beta = h2{b16, b16};
  }

  const int B = a.B_dev ? (int)*a.B_dev : a.B;
  for (;;) {
    __syncthreads();
    if (tid == 0) {
      red[3] = (int)atomicAdd(queue, 2u);
      red[0] = 0;
      red[1] = 0;
    }
    __syncthreads();
    const int entry = red[3];
    if (entry >= B) break;
    const bool pair = entry + 1 < B;  // (an odd batch: the last pair's high half is dead)
    const int cw0 = a.cw_idx ? a.cw_idx[entry] : entry;
    const int cw1 = pair ? (a.cw_idx ? a.cw_idx[entry + 1] : entry + 1) : cw0;
    {
      const void *r0 = prior_row<LLR>(a, cw0, io...), *r1 = prior_row<LLR>(a, cw1, io...);
      for (int v = tid; v < c.N; v += T) {
        h2 L = {(_Float16)0.0f, (_Float16)0.0f};  // a punctured column, and the dead half
        if (v >= c.punct) {
          L.x = prior_of<LLR>(r0, v - c.punct);
          if (pair) L.y = prior_of<LLR>(r1, v - c.punct);
        }
        post[v] = as_u(L);
      }
    }
    for (int e = tid; e < c.E; e += T) c2v[e] = 0;  // messages start at +0
    // (filled per pair, after the priors: held across kml_log they would spill)
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
    int done = pair ? 0 : 2;  // bit H: half H is recorded
    for (;;) {
      // (wg_any2's barrier also keeps the next sweep's writes behind this pass's reads)
      unsigned odd = 0;
      if constexpr (CACHED) {  // the passes hold every row once
#pragma unroll
        for (int p = 0; p < kCachePasses; ++p)
          if (p < lp.npass) odd |= lnms_odd_rows(s, item[p]);
      } else if constexpr (GT) {  // ... and so do the table's
        lnms_gt_passes<T>(gtab, lp.npass, tid, [&](int, const LnmsItem &it) { odd |= lnms_odd_rows(s, it); });
      } else {
        for (int first = 0; first < c.M; first += T / kLanes)
          odd |= lnms_odd_rows(s, lnms_item(s, first, c.M - first, g, l));
      }
      const int fail = wg_any2<T / 64>((odd & 0x8000u) != 0, (odd & 0x80000000u) != 0, wflags);
      const int fin = ~done & (iter == a.iter_count ? 3 : ~fail & 3);  // the halves that stop here
      if (fin & 1) lnms_record<T, 0, POST>(c, a, s, cch, red, cw0, iter, !(fail & 1), tid, io...);
      if (fin & 2) lnms_record<T, 1, POST>(c, a, s, cch, red, cw1, iter, !(fail & 2), tid, io...);
      done |= fin;
      if (done == 3) break;
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
  }
}

size_t lnms_h16_lds_bytes(const DevCode &c, int npass) {
  return (size_t)c.N * 4 + (size_t)c.E * 4 + (size_t)npass * 4 + kRedBytes + (size_t)c.E * 2 +
         ((size_t)c.M + 1) * 2 + (size_t)c.N;
}

// The code and launch rules of bp_irregular_lnms.hip's lnms_launch_shape, on
// this kernel's LDS (the same bytes): 0 = not this kernel's, else workgroups per CU.
// global: the global-table instance, as in bp_irregular_lnms.hip (its LDS is
// the decoder state: no tables).
int lnms_h16_launch_shape(const DevCode &c, const BpLaunch &a, const LnmsPlanDev &lp, bool have_gt, size_t &lds,
                          bool &global) {
  if (!lp.pass || lp.npass < 1) return 0;
  if (!bp_irregular_nms_supported(c) && !bp_lnms_only_supported(c, lp.npass)) return 0;
  if (a.syn || a.cw_prof || a.prof) return 0;
  if (c.dc_max > 2 * kLanes || c.E > 65535 || c.N >= (int)kNoCol || c.M > 65535) return 0;
  lds = lnms_h16_lds_bytes(c, lp.npass);
  global = lnms_tables_forced_global() || lds + sizeof(WgVotes) > kLdsLimit;
  if (global) {
    if (!have_gt) return 0;
    lds = (size_t)c.N * 4 + (size_t)c.E * 4 + (size_t)lp.npass * 4 + kRedBytes + (size_t)c.N;
  }
  if (lds + sizeof(WgVotes) > kLdsLimit) return 0;
  return 2 * (lds + sizeof(WgVotes) + 1024) <= kLdsLimit ? 2 : 1;
}

}  // namespace

hipError_t launch_bp_irregular_lnms_h16(const DevCode &c, const BpLaunch &a, const LnmsPlanDev &lp,
                                        const LlrIoDev *io, const OmsDev *oms, hipStream_t s,
                                        const LnmsItemsDev *gt, bool *global_out) {
  constexpr int T = kIrrThreads;
  static_assert(T / kLanes == kLayRowsPerPass, "the plan's passes are this kernel's");
  size_t lds = 0;
  bool global = false;
  const int per_cu = lnms_h16_launch_shape(c, a, lp, gt && gt->item, lds, global);
  if (!per_cu || (io && !io->llr)) return hipErrorNotSupported;
  if (global_out) *global_out = global;
  if (oms && !(oms->beta > 0.0f)) oms = nullptr;
  const long long pairs = ((long long)a.B + 1) / 2;  // a workgroup takes two entries at a time
  auto go = [&](auto kern, const auto &...x) {
    return launch_persistent(kern, T, lds, per_cu, pairs, false, a, s, c, a, a.queue, lp, x...);
  };
  // g: nothing (the LDS-table instances), or the global-table instances' LnmsItemsDev, the pack's last
  auto pick = [&](auto cached, const auto &...g) {
    constexpr bool C = decltype(cached)::value;
    if (!io)
      return oms ? go(bp_irregular_lnms_h16_kernel<T, C, false, OmsDev, std::decay_t<decltype(g)>...>, *oms, g...)
                 : go(bp_irregular_lnms_h16_kernel<T, C, false, std::decay_t<decltype(g)>...>, g...);
    if (io->post)
      return oms ? go(bp_irregular_lnms_h16_kernel<T, C, true, LlrIoDev, OmsDev, std::decay_t<decltype(g)>...>, *io, *oms,
                      g...)
                 : go(bp_irregular_lnms_h16_kernel<T, C, true, LlrIoDev, std::decay_t<decltype(g)>...>, *io, g...);
    return oms ? go(bp_irregular_lnms_h16_kernel<T, C, false, LlrIoDev, OmsDev, std::decay_t<decltype(g)>...>, *io, *oms,
                    g...)
               : go(bp_irregular_lnms_h16_kernel<T, C, false, LlrIoDev, std::decay_t<decltype(g)>...>, *io, g...);
  };
  if (global) return lp.npass <= kCachePasses ? pick(std::true_type{}, *gt) : pick(std::false_type{}, *gt);
  return lp.npass <= kCachePasses ? pick(std::true_type{}) : pick(std::false_type{});
}

}  // namespace kml
