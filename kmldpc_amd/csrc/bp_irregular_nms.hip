// bp_irregular_nms.hip — normalized min-sum sibling of bp_irregular.hip: the
// KML_ALG_NMS mode of a context (include/kmldpc_amd.h), for the codes that take
// bp_irregular_kernel (5G BG2 K960: 7,392 edges, column degrees up to 9, row
// degrees up to 10).  A different decoder from the reference's sum-product:
// its results are not the reference's.  What is fixed is its arithmetic, which
// tests/bp_nms_model.py states in numpy and this kernel equals bit for bit.
//
// The arithmetic contract.  Every value is IEEE binary32 with denormals kept,
// no fma (-ffp-contract=off), each operation rounded once:
//   * prior: q = min(max(P0, 1e-12), 1 - 1e-12) in fp64 (the reference's
//     ProbClip constants), L = (float)(kml_log(q) - kml_log(1 - q)), the
//     subtraction in fp64; a punctured 5G column has L = +0; messages start
//     at +0 (the reference's 0.5);
//   * VN phase, column v, edges in column order: t = L; t = t + c2v_k for
//     every k; T = t; decision T > 0 ? 0 : 1 (a tie decides 1, as the
//     reference's alpha0 > alpha1 ? 0 : 1); v2c_k = clamp(T - c2v_k, -256, 256);
//   * stop rule and return value as in bp_irregular.hip: after the VN phase,
//     when every row's decisions have even parity, stop before the CN phase;
//     ret = iter + (iter < max_iter); iter_count = 0 writes no decisions;
//   * CN phase, row with incoming m_j: a_j = min over i != j of |m_i|, s_j =
//     XOR over i != j of the sign bits of m_i (-0 counts as negative), c2v_j =
//     RN(alpha * a_j) with its sign bit set to s_j.
// The CN phase is order-independent and exact apart from the one multiply:
// magnitudes are compared as the integers their bit patterns are (the order of
// non-negative floats, denormals included), a_j is the row's second minimum on
// the edges that hold the minimum and the minimum elsewhere (with the minimum
// held twice the two are equal).  There is no division, so no FAST / EXACT
// split, no defer list and no redo: CNT_REDONE stays 0.
//
// Mapping: bp_irregular.hip's, on the same host plan (layout.hpp
// IrregularPlan, kIrrCnStride): one persistent workgroup of kIrrThreads per
// CU over the dequeue counter; thread t has up to three columns and three
// half-rows (the plan's rounds; the items of a paired round simply run one
// after the other: there is no dependent divide chain to hide); a row is split
// over a lane pair, the even lane takes edges [0, (D+1)/2), the odd lane the
// rest, and the halves' (min1, min2, sign, parity) cross in two DPP swaps (sign
// and parity ride in the sign bits of the two magnitudes).
// Slots are 8 bytes per edge: .x the message (c2v after a CN phase, v2c after a
// VN phase), .y the column's decision bit, which the CN chains XOR from the
// words they load anyway (an LLR's sign is data, so the decision cannot ride in
// it as it does in the fp64 kernels); the CN phase closes with wg_any.
// LDS: irr_slots * 8 + cc_len * 4 (float priors) + 16 + E * 2 (u16 slot table)
// + N decision bytes: about 85 KB for BG2, one workgroup per CU.
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
constexpr unsigned kInfBits = 0x7F800000u;   // above every magnitude: |v2c| <= 256
constexpr unsigned kSignBit = 0x80000000u;
constexpr float kNmsClamp = 256.0f;

__device__ __forceinline__ unsigned swap_pair_u(unsigned x) {
  return (unsigned)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xF, 0xF, false);
}
__device__ __forceinline__ unsigned umin(unsigned a, unsigned b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

// One column of degree D: cs = its D slot indices in column order, L its prior.
// POST: T also goes to *tp (the posterior instance's LDS array).
template <int D, bool POST>
__device__ __forceinline__ void nms_vn_col(int2 *slots, const unsigned short *cs, float L, unsigned char *hard,
                                           float *tp) {
  int s[D];
  float c[D];
#pragma unroll
  for (int k = 0; k < D; ++k) s[k] = cs[k];
#pragma unroll
  for (int k = 0; k < D; ++k) c[k] = __int_as_float(slots[s[k]].x);
  float t = L;
#pragma unroll
  for (int k = 0; k < D; ++k) t = t + c[k];
  const int hb = t > 0.0f ? 0 : 1;
  *hard = (unsigned char)hb;
  if constexpr (POST) *tp = t;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const float q = fminf(fmaxf(t - c[k], -kNmsClamp), kNmsClamp);
    slots[s[k]] = make_int2(__float_as_int(q), hb);
  }
}

// Degree dispatch.  d is in 1..9 (columns) and 2..10 (rows): irr_ok and the
// maxima checked by bp_irregular_nms_supported; the default cases are 9 and 10.
template <bool POST>
__device__ __forceinline__ void nms_vn_any(int d, int2 *slots, const unsigned short *cs, float L,
                                           unsigned char *hard, float *tp) {
  switch (d) {
    case 1: nms_vn_col<1, POST>(slots, cs, L, hard, tp); break;
    case 2: nms_vn_col<2, POST>(slots, cs, L, hard, tp); break;
    case 3: nms_vn_col<3, POST>(slots, cs, L, hard, tp); break;
    case 4: nms_vn_col<4, POST>(slots, cs, L, hard, tp); break;
    case 5: nms_vn_col<5, POST>(slots, cs, L, hard, tp); break;
    case 6: nms_vn_col<6, POST>(slots, cs, L, hard, tp); break;
    case 7: nms_vn_col<7, POST>(slots, cs, L, hard, tp); break;
    case 8: nms_vn_col<8, POST>(slots, cs, L, hard, tp); break;
    default: nms_vn_col<9, POST>(slots, cs, L, hard, tp); break;
  }
}

// A lane's half of a row of degree D (both lanes of the pair run it): the even
// lane holds edges [0, S), the odd lane [S, D), S = (D + 1) / 2; base = the slot
// of edge 0, the row's edges kIrrCnStride apart.  Returns the row's parity (the
// XOR of its columns' decisions), the same on both lanes.
// OMS: the offset correction (kernels.hpp OmsDev), c = max(RN(c - beta), +0).
template <int D, bool OMS>
__device__ __forceinline__ unsigned nms_cn_half(int2 *slots, int base, int odd, float alpha, float beta) {
  constexpr int S = (D + 1) / 2;
  const int first = odd ? S : 0;
  const int own = odd ? D - S : S;
  unsigned m[S];
  unsigned min1 = kInfBits, min2 = kInfBits, sgn = 0, par = 0;
#pragma unroll
  for (int j = 0; j < S; ++j) {
    m[j] = kInfBits;  // (an absent edge: above every magnitude, sign clear)
    if (j < own) {
      const int2 w = slots[base + (first + j) * kIrrCnStride];
      m[j] = (unsigned)w.x;
      par ^= (unsigned)w.y;
      sgn ^= m[j];
      const unsigned a = m[j] & ~kSignBit;
      min2 = umin(min2, umax(min1, a));
      min1 = umin(min1, a);
    }
  }
  // the partner's half: its sign XOR rides in min1's sign bit, its parity in min2's
  const unsigned o1 = swap_pair_u(min1 | (sgn & kSignBit));
  const unsigned o2 = swap_pair_u(min2 | (par << 31));
  const unsigned p1 = o1 & ~kSignBit, p2 = o2 & ~kSignBit;
  const unsigned rsgn = (sgn ^ o1) & kSignBit;
  const unsigned rpar = (par ^ (o2 >> 31)) & 1u;
  const unsigned r1 = umin(min1, p1);
  const unsigned r2 = umin(umax(min1, p1), umin(min2, p2));
#pragma unroll
  for (int j = 0; j < S; ++j) {
    if (j < own) {
      const unsigned a = (m[j] & ~kSignBit) == r1 ? r2 : r1;
      float q = alpha * __int_as_float((int)a);
      if constexpr (OMS) q = fmaxf(q - beta, 0.0f);  // (q - beta is never -0 and never NaN)
      slots[base + (first + j) * kIrrCnStride].x = (int)((unsigned)__float_as_int(q) | ((m[j] ^ rsgn) & kSignBit));
    }
  }
  return rpar;
}

template <bool OMS>
__device__ __forceinline__ unsigned nms_cn_any(int d, int2 *slots, int base, int odd, float alpha, float beta) {
  switch (d) {
    case 2: return nms_cn_half<2, OMS>(slots, base, odd, alpha, beta);
    case 3: return nms_cn_half<3, OMS>(slots, base, odd, alpha, beta);
    case 4: return nms_cn_half<4, OMS>(slots, base, odd, alpha, beta);
    case 5: return nms_cn_half<5, OMS>(slots, base, odd, alpha, beta);
    case 6: return nms_cn_half<6, OMS>(slots, base, odd, alpha, beta);
    case 7: return nms_cn_half<7, OMS>(slots, base, odd, alpha, beta);
    case 8: return nms_cn_half<8, OMS>(slots, base, odd, alpha, beta);
    case 9: return nms_cn_half<9, OMS>(slots, base, odd, alpha, beta);
    default: return nms_cn_half<10, OMS>(slots, base, odd, alpha, beta);
  }
}

__host__ __device__ inline size_t nms_lds_bytes(const DevCode &c) {
  return (size_t)c.irr_slots * 8 + (size_t)c.cc_len * 4 + (size_t)c.E * 2 + kRedBytes + (size_t)c.N;
}
// ... and with the posterior instance's N floats behind it
size_t nms_post_lds_bytes(const DevCode &c) { return ((nms_lds_bytes(c) + 3) & ~(size_t)3) + (size_t)c.N * 4; }

// The iterations of one codeword (bp_irregular.hip decode_irr without its
// FAST / SYN / PROF parts).  Each lane's plan is packed into one word per
// round (slot base | degree << 14 | column or row << 18; ~0 = no item).
template <int T, bool POST, bool OMS>
__device__ __forceinline__ void decode_nms(const DevCode &c, const BpLaunch &a, int2 *slots,
                                           const unsigned short *cslot, const float *pri, unsigned char *cch,
                                           float *tpost, int odd, const int (&vcol)[3], const int (&crow)[3],
                                           int &iter_out, bool &conv_out, float beta) {
  unsigned vpk[3], cpk[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    vpk[r] = ~0u;
    cpk[r] = ~0u;
    if (vcol[r] >= 0) {
      const int b = c.col_ptr[vcol[r]];
      vpk[r] = (unsigned)b | (unsigned)(c.col_ptr[vcol[r] + 1] - b) << 14 | (unsigned)vcol[r] << 18;
    }
    if (crow[r] >= 0) {
      const int b = c.irr_cn_base[r * (T / 2) + (threadIdx.x >> 1)];
      const int d = c.row_ptr[crow[r] + 1] - c.row_ptr[crow[r]];
      cpk[r] = (unsigned)b | (unsigned)d << 14 | (unsigned)crow[r] << 18;
    }
  }
  auto pbase = [](unsigned w) { return (int)(w & 0x3FFFu); };
  auto pdeg = [](unsigned w) { return (int)((w >> 14) & 15u); };
  auto pitem = [](unsigned w) { return (int)(w >> 18); };
  __shared__ WgVotes wflags;  // wg_any (bp_common.hpp)
  const float alpha = a.nms_alpha;
  int iter = 0;
  bool conv = false;
  for (; iter < a.iter_count; ++iter) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if (vpk[r] != ~0u) {
        const int v = pitem(vpk[r]);
        const float L = v >= c.punct ? pri[v - c.punct] : 0.0f;
        nms_vn_any<POST>(pdeg(vpk[r]), slots, cslot + pbase(vpk[r]), L, &cch[v], POST ? &tpost[v] : nullptr);
      }
    __syncthreads();
    // The early-stop parity of each row comes out of the CN pass (the decisions
    // ride in the slots' .y words the halves load); the OR over the workgroup
    // is the CN phase's closing barrier (speculative CN, as in bp_irregular.hip).
    unsigned fail = 0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
      if (cpk[r] != ~0u)  // both lanes of a pair agree
        fail |= nms_cn_any<OMS>(pdeg(cpk[r]), slots, pbase(cpk[r]), odd, alpha, beta);
    if (!wg_any<T / 64>(fail != 0, wflags)) {
      conv = true;
      break;
    }
  }
  iter_out = iter;
  conv_out = conv;
}

// The instance without Llr is the P0 front end (the contract above).  With one
// LlrIoDev argument the priors are the caller's floats, clamped to +-256 (there
// is no log in that instance), and POST also keeps the T of every VN phase in N
// more floats of LDS and writes the last one out with the decisions.  With an
// OmsDev argument (the last one) the CN phase applies the offset correction.
template <int T, bool POST = false, class... X>
__global__ __launch_bounds__(T) void bp_irregular_nms_kernel(DevCode c, BpLaunch a, unsigned int *queue, X... io) {
  constexpr bool LLR = pack_has<LlrIoDev, X...>, OMS = pack_has<OmsDev, X...>;
  static_assert(LLR || !POST, "the posterior output belongs to the LLR instances");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  const int odd = tid & 1;
  int2 *slots = reinterpret_cast<int2 *>(smem);
  const size_t sb = (size_t)c.irr_slots * 8;  // slot blocks (layout.hpp kIrrCnStride)
  float *pri = reinterpret_cast<float *>(smem + sb);
  int *red = reinterpret_cast<int *>(smem + sb + (size_t)c.cc_len * 4);
  unsigned short *cslot = reinterpret_cast<unsigned short *>(smem + sb + (size_t)c.cc_len * 4 + kRedBytes);
  unsigned char *cch = smem + sb + (size_t)c.cc_len * 4 + kRedBytes + (size_t)c.E * 2;
  float *tpost = nullptr;  // POST: [N], behind the decision bytes
  if constexpr (POST) tpost = reinterpret_cast<float *>(smem + ((nms_lds_bytes(c) + 3) & ~(size_t)3));

  for (int e = tid; e < c.E; e += T) cslot[e] = (unsigned short)c.irr_col_slot[e];
  int vcol[3], crow[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    vcol[r] = c.irr_vn[r * T + tid];
    crow[r] = c.irr_cn[r * (T / 2) + (tid >> 1)];
  }

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
      const float *l = pack_get<LlrIoDev>(io...).llr + (long long)cw * a.p0_stride;
      if (a.p0_sel) l += (long long)a.p0_sel[cw] * a.p0_sel_stride;
      for (int i = tid; i < c.cc_len; i += T) pri[i] = fminf(fmaxf(l[i], -kNmsClamp), kNmsClamp);
    } else {
      const double *p0 = a.p0 + (long long)cw * a.p0_stride;
      if (a.p0_sel) p0 += (long long)a.p0_sel[cw] * a.p0_sel_stride;

      for (int i = tid; i < c.cc_len; i += T) {
        const double q = fmin(fmax(p0[i], kSmallestProb), 1.0 - kSmallestProb);
        pri[i] = (float)(kml_log(q) - kml_log(1.0 - q));
      }
    }
    for (int e = tid; e < c.irr_slots; e += T) slots[e] = make_int2(0, 0);  // messages start at +0
    __syncthreads();  // the first VN phase reads priors and slots other threads wrote

    int iter = 0;
    bool conv = false;
    float beta = 0.0f;
    if constexpr (OMS) beta = pack_get<OmsDev>(io...).beta;
    decode_nms<T, POST, OMS>(c, a, slots, cslot, pri, cch, tpost, odd, vcol, crow, iter, conv, beta);

    if (a.iter_count > 0) {
      if (a.uu_hat) {
        uint8_t *u = a.uu_hat + (long long)cw * c.K;
        for (int i = tid; i < c.K; i += T) u[i] = cch[i + c.info_off];
      }
      if (a.cc_hat) {
        uint8_t *o = a.cc_hat + (long long)cw * c.N;
        for (int v = tid; v < c.N; v += T) o[v] = cch[v];
      }
      if constexpr (POST) {  // the T of the VN phase these decisions came from
        float *o = pack_get<LlrIoDev>(io...).post + (long long)cw * c.N;
        for (int v = tid; v < c.N; v += T) o[v] = tpost[v];
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

}  // namespace

// The codes of launch_bp_irregular (bp_irregular.hip): irr_ok, a round plan,
// slot indices that fit the packed plan words, and the LDS of this kernel.
bool bp_irregular_nms_supported(const DevCode &c) {
  // (the fp64 sibling's LDS, 16 bytes per slot and 8 per prior, decides whether
  // the code takes bp_irregular_kernel at all)
  const size_t sibling = (size_t)c.irr_slots * 16 + (size_t)c.E * 2 + (size_t)c.cc_len * 8 + kRedBytes + (size_t)c.N;
  // nms_vn_any / nms_cn_any have instances for column degrees 1..9 and row
  // degrees 2..10 and send anything else to the largest: irr_ok says every
  // degree is inside, the maxima are checked here once more
  return c.irr_ok && c.dv_max >= 1 && c.dv_max <= 9 && c.dc_max >= 2 && c.dc_max <= 10 && c.irr_vn && c.irr_cn &&
         c.irr_cn_base && c.irr_col_slot && c.irr_slots <= 16383 && sibling <= kLdsLimit &&
         nms_lds_bytes(c) <= kLdsLimit;
}

bool bp_irregular_nms_post_supported(const DevCode &c) {
  return bp_irregular_nms_supported(c) && nms_post_lds_bytes(c) <= kLdsLimit;
}

// io = NULL: P0 priors; else float priors (io->llr), and the posterior instance
// when io->post is set.  oms: the offset instances (beta > 0), else the plain ones.
hipError_t launch_bp_irregular_nms(const DevCode &c, const BpLaunch &a, const LlrIoDev *io, const OmsDev *oms,
                                   hipStream_t s) {
  constexpr int T = kIrrThreads;
  if (!bp_irregular_nms_supported(c) || (io && !io->llr)) return hipErrorNotSupported;
  if (a.syn || a.cw_prof || a.prof) return hipErrorNotSupported;  // no syndrom_soft, no profile (launch_bp says why)
  if (oms && !(oms->beta > 0.0f)) oms = nullptr;
  const bool post = io && io->post;
  if (post && !bp_irregular_nms_post_supported(c)) return hipErrorNotSupported;
  const size_t lds = post ? nms_post_lds_bytes(c) : nms_lds_bytes(c);
  auto go = [&](auto kern, const auto &...x) {
    return launch_persistent(kern, T, lds, 1, kNoGridCap, false, a, s, c, a, a.queue, x...);
  };
  if (!io) return oms ? go(bp_irregular_nms_kernel<T, false, OmsDev>, *oms) : go(bp_irregular_nms_kernel<T>);
  if (post)
    return oms ? go(bp_irregular_nms_kernel<T, true, LlrIoDev, OmsDev>, *io, *oms)
               : go(bp_irregular_nms_kernel<T, true, LlrIoDev>, *io);
  return oms ? go(bp_irregular_nms_kernel<T, false, LlrIoDev, OmsDev>, *io, *oms)
             : go(bp_irregular_nms_kernel<T, false, LlrIoDev>, *io);
}

}  // namespace kml
