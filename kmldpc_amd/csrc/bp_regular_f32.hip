// bp_regular_f32.hip — single-precision sibling of bp_regular.hip for the
// PEG2304-class shape (dv 3, dc 6, N = 2304, 2M = 2304): the opt-in
// KML_PREC_F32 mode of a context (include/kmldpc_amd.h).
//
// NOT bit-exact with the reference.  Same schedule as
// lab::BinaryLDPCCodec::Decoder (lib/lab/src/binaryldpccodec.cc:165-278) —
// VN forward / backward chains in column order with the hard decision
// alpha0 > alpha1 ? 0 : 1, early stop on an all-zero syndrome before the CN
// phase, CN forward / backward trellis with the clip of c2v0 and
// c2v1 = 1 - c2v0, syndrom_soft from the row head, return value
// iter + (iter < max_iter) — with every message and chain value a float.
// The arithmetic contract (tests/test_bp_f32_model.py is its numpy form):
//   * the prior pair is formed in fp64, (P0, 1 - P0), and each member rounded
//     to float: the small member keeps its own 24 bits;
//   * a normalisation (n0, n1) / (n0 + n1) is r = v_rcp_f32(n0 + n1) (1 ulp)
//     and two multiplies; -ffp-contract=off, no fma;
//   * the clip constants are (float)1e-12 and (float)(1 - 1e-12) = 1.0f;
//   * identities that are exact in float are applied as such: x * 1.0f = x,
//     and the column's first backward step (c0, 1 - c0) / (c0 + (1 - c0)),
//     whose sum rounds to exactly 1 (bp_common.hpp, the same argument at
//     24 bits).
// None of the fp64 path's proof / defer / redo machinery applies to the
// decoder: CNT_REDONE stays 0.  The fused QPSK prologue computes P0 in fp64
// exactly as bp_regular_kernel does (demap_common.hpp; a codeword with a symbol
// the FAST demap cannot prove goes to a second launch that demaps with div_rn),
// so fused and separate decodes agree bit for bit within this mode.
//
// Mapping: as bp_regular.hip (one workgroup of 768 threads per codeword,
// persistent over the dequeue counter, lane pairs share a check row), with the
// message slots 8 bytes per edge — {q0, q1 | decision in the sign bit} for
// v2c, the c2v float in the lower or upper word — at half the byte offsets of
// the host plan (layout.hpp).  A codeword's LDS is 60 KB (the fused demap's
// priors alias the slot area, which is first written after the barrier that
// follows the prior loads).  One workgroup per CU, like bp_regular.hip: two
// would fit the LDS, but need 80 registers per lane, and the build bounded to
// 80 spilled to scratch and measured slower ("Single-precision
// mode").
#include <cstdlib>

#include "bp_common.hpp"
#include "bp_launch.hpp"
#include "demap_common.hpp"
#include "kernels.hpp"

namespace kml {

namespace {

constexpr int kRedBytes = 16;
constexpr int kF32MaxKw = 64;  // K <= N <= 2304: 36 words

typedef float flt2 __attribute__((ext_vector_type(2)));  // 8-byte LDS slot (ds_write_b64)

constexpr float kClipLo = 1.0e-12f;
constexpr float kClipHi = (float)(1.0 - 1.0e-12);  // 1.0f

__device__ __forceinline__ float swap_pair_f(float x) {  // adjacent lane (quad_perm [1,0,3,2])
  return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0xB1, 0xF, 0xF, false));
}
__device__ __forceinline__ int swap_pair_i32(int x) { return __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, false); }
// x (>= +0 or NaN) with its sign bit set to bit
__device__ __forceinline__ float with_sign_f(float x, int bit) {
  return __int_as_float((__float_as_int(x) & 0x7FFFFFFF) | (bit << 31));
}
// (n0, n1) / (n0 + n1): one hardware reciprocal, one packed multiply
__device__ __forceinline__ flt2 norm2(flt2 n) {
  const float r = __builtin_amdgcn_rcpf(n.x + n.y);
  return n * flt2{r, r};
}

// Dynamic LDS: E slots of 8 B (the fused demap's N priors, 8 B each, alias
// them: N <= E), the reduction words, N hard-decision bytes, then the info
// bits' positions (u16, K entries).
constexpr size_t f32_ipos_offset(int E, int N) { return ((size_t)E * 8 + kRedBytes + (size_t)N + 1) & ~(size_t)1; }
constexpr size_t f32_lds_bytes(int E, int N, int K) { return f32_ipos_offset(E, N) + (size_t)K * 2; }

// EXACT selects the fused demap's form only (DMB > 0): false = FAST demap,
// a codeword with an unproven symbol is appended to the defer list and decoded
// by the EXACT launch.  The decoder itself is the same code in both.
template <int T, int RV, int RC, int DV, int DC, bool SYN, int DMB, bool EXACT>
__global__ __launch_bounds__(T) void bp_regular_f32_kernel(DevCode c, BpLaunch a, unsigned int *queue) {
  static_assert(DC % 2 == 0, "the lane-pair split assumes an even row degree");
  constexpr int H = DC / 2;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ WgVotes wflags;  // wg_any (bp_common.hpp)
  __shared__ WgVotes pflags;  // wg_all of the fused demap's proof
  __shared__ double dcons[DMB > 0 ? (2 << DMB) : 2];
  __shared__ uint64_t detab[DMB > 0 ? 256 : 1];
  __shared__ uint64_t refw[kF32MaxKw];                    // this codeword's reference bits
  __shared__ unsigned long long wcnt[CNT_CONVERGED + 1];  // the workgroup's counters
  flt2 *p0s = reinterpret_cast<flt2 *>(smem);             // fused demap: (P0, 1 - P0) by bit, over the slots
  if constexpr (DMB > 0) {
    for (int k = threadIdx.x; k < (2 << DMB); k += T) dcons[k] = a.sym_cons[k];
    stage_exp_table(detab);
  }
  const int tid = threadIdx.x;
  const int odd = tid & 1;
  int *red = reinterpret_cast<int *>(smem + (size_t)c.E * 8);
  unsigned char *cch = smem + (size_t)c.E * 8 + kRedBytes;
  const unsigned smem_a = lds_addr(smem), hd = lds_addr(cch) + tid;
  unsigned short *ipos = reinterpret_cast<unsigned short *>(smem + f32_ipos_offset(c.E, c.N));
  for (int i = tid; i < c.K; i += T) ipos[i] = (unsigned short)c.reg_pos[c.info_off + i];
  // What a codeword needs once (its columns, its rows' numbers) is read again
  // from the plan in global memory where it is used, not held in registers
  // across the iterations.
  unsigned vaddr[RV][DV];
#pragma unroll
  for (int r = 0; r < RV; ++r) {
    const int v = c.vn_order[r * T + tid];
    const int b = c.col_ptr[v];
#pragma unroll
    for (int k = 0; k < DV; ++k) {
      vaddr[r][k] = smem_a + ((unsigned)c.reg_c2v[b + k] >> 1);  // the plan's offsets are for 16-byte slots
      asm volatile("" : "+v"(vaddr[r][k]));
    }
  }
  const int chalf = ((tid >> 3) & 1) * 4;  // bit 2 of the CN position (tid >> 1)
  unsigned rb[RC], rb2[RC], wb[RC];
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    rb[r] = smem_a + (unsigned)((r * (T / 2) + (tid >> 1)) * DC + odd) * 8;
    rb2[r] = rb[r] + 8 - 16 * odd;
    wb[r] = rb[r] + chalf;
    asm volatile("" : "+v"(rb[r]), "+v"(rb2[r]), "+v"(wb[r]));
  }

  const int B = a.B_dev ? (int)*a.B_dev : a.B;
  const bool cnt_lds = a.counters != nullptr;
  const bool ref_pre = a.ref_bits && a.iter_count > 0;  // (c.Kw <= kF32MaxKw: host check)
  if (cnt_lds && tid <= CNT_CONVERGED) wcnt[tid] = 0;   // ordered by the loop's first barrier
  if (tid == 0) {  // the first entry; then each codeword's epilogue takes the next
    red[3] = (int)atomicAdd(queue, 1u);
    red[0] = 0;
    red[1] = 0;
  }
  for (;;) {
    __syncthreads();
    const int entry = red[3];
    if (entry >= B) break;
    const int cw = a.cw_idx ? a.cw_idx[entry] : entry;
    if (ref_pre && tid < 2 * c.Kw)  // one dword per lane (the first waves), in flight through the prologue
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const unsigned *>(a.ref_bits + (long long)cw * c.Kw) + tid,
                                       (__attribute__((address_space(3))) void *)(reinterpret_cast<unsigned *>(refw) +
                                                                                  (tid & ~63)),
                                       4, 0, 0);
    flt2 pv[RV];
    bool dok = true;
    if constexpr (DMB > 0) {  // ModemLinearSystem::DeMapping of this codeword in fp64, rounded into LDS
      const int S = c.cc_len / DMB;
      const double2 hh = a.sym_h[(long long)cw * a.sym_h_stride + (a.sym_h_sel ? a.sym_h_sel[cw] : 0)];
      const double2 *yy = a.sym_y + (long long)cw * S;
      for (int j = tid; j < S; j += T) {
        const double2 v = yy[j];
        double out[DMB];
        if constexpr (EXACT)
          demap_symbol_t<DMB, false, lds_cons, false>((lds_cons)dcons, (lds_exptab)detab, v.x, v.y, hh.x, hh.y,
                                                          a.sym_var, out);
        else
          dok &= demap_symbol_t<DMB, true, lds_cons, false>((lds_cons)dcons, (lds_exptab)detab, v.x, v.y, hh.x,
                                                              hh.y, a.sym_var, out);
#pragma unroll
        for (int b = 0; b < DMB; ++b) p0s[j * DMB + b] = flt2{(float)out[b], (float)(1.0 - out[b])};
      }
      __syncthreads();
#pragma unroll
      for (int r = 0; r < RV; ++r) {
        const int v = c.vn_order[r * T + tid];
        pv[r] = (v >= c.punct) ? p0s[v - c.punct] : flt2{0.5f, 0.5f};
      }
    } else {
      const double *p0 = a.p0 + (long long)cw * a.p0_stride;
      if (a.p0_sel) p0 += (long long)a.p0_sel[cw] * a.p0_sel_stride;
#pragma unroll
      for (int r = 0; r < RV; ++r) {
        const int v = c.vn_order[r * T + tid];
        const double q = (v >= c.punct) ? p0[v - c.punct] : 0.5;
        pv[r] = flt2{(float)q, (float)(1.0 - q)};
      }
    }
    // the LDS writes land before wave 0 passes the next barrier (the barriers wait lgkmcnt only)
    if (ref_pre) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // every prior is in registers before the first slot store (p0s aliases the slots)
    bool defer = false;
    if constexpr (DMB > 0 && !EXACT)
      defer = !wg_all<T / 64>(dok, pflags);
    else if constexpr (DMB > 0)
      __syncthreads();
    if (defer) {  // (DMB > 0, FAST demap) the EXACT launch demaps and decodes this codeword
      if (tid == 0) {
        a.defer_idx[atomicAdd(a.defer_cnt, 1u)] = cw;
        red[3] = (int)atomicAdd(queue, 1u);  // (every thread has read red[3])
      }
      continue;
    }

    int iter = 0;
    bool conv = false;
    for (; iter < a.iter_count; ++iter) {
      // ---------------------------------------------------------- VN phase
      __builtin_amdgcn_s_setprio(3);
      {
        // InitMsg: every c2v is 0.5 before the first CN phase
        float c0s[RV][DV];
#pragma unroll
        for (int r = 0; r < RV; ++r)
#pragma unroll
          for (int k = 0; k < DV; ++k) c0s[r][k] = iter == 0 ? 0.5f : lds_ld<float>(vaddr[r][k]);
#pragma unroll
        for (int r = 0; r < RV; ++r) {
          flt2 al[DV], al_cur = pv[r];
          int hb = 0;
#pragma unroll
          for (int k = 0; k < DV; ++k) {
            al[k] = al_cur;
            const float c0 = c0s[r][k];
            const flt2 q = norm2(al_cur * flt2{c0, 1.0f - c0});
            if (k + 1 < DV)
              al_cur = q;
            else {  // the posterior only feeds the hard decision
              hb = (q.x > q.y) ? 0 : 1;
              lds_st<unsigned char>(hd + r * T, (unsigned char)hb);
            }
          }
          flt2 be = {1.0f, 1.0f};
#pragma unroll
          for (int k = DV - 1; k >= 0; --k) {
            const flt2 t = k == DV - 1 ? al[k] : al[k] * be;  // beta = (1, 1): x * 1 = x
            const flt2 q = norm2(t);
            lds_st<flt2>(vaddr[r][k] & ~7u, flt2{q.x, with_sign_f(q.y, hb)});
            if (k > 0) {
              const float c0 = c0s[r][k];
              const flt2 cc = {c0, 1.0f - c0};
              be = k == DV - 1 ? cc : norm2(be * cc);  // c0 + (1 - c0) rounds to exactly 1
            }
          }
          if (r == RV / 2) __builtin_amdgcn_s_setprio(1);
        }
        __builtin_amdgcn_s_setprio(0);
      }
      __syncthreads();

      // ---------------------------------------------------------- CN phase
      // (speculative: the parity check of the decisions rides on its loads, and
      // a converged codeword discards it — bp_regular.hip)
      unsigned par[RC];
      float syn0[RC];
      {
        flt2 x[RC][H];  // lower-half chain states, kept for the swap
        flt2 s[RC];     // current chain state
#pragma unroll
        for (int r = 0; r < RC; ++r) {
          s[r] = flt2{1.0f, 0.0f};
          par[r] = 0;
        }
        __builtin_amdgcn_s_setprio(2);
#pragma unroll
        for (int st = 0; st < DC; ++st) {
          if (st == 2) __builtin_amdgcn_s_setprio(1);
          if (st == 4) __builtin_amdgcn_s_setprio(0);
          const bool advance = SYN || st + 1 < DC;
          flt2 m[RC];
          if (advance) {
#pragma unroll
            for (int r = 0; r < RC; ++r) {
              // edge (odd ? DC-1-st : st): physical slot 2st+odd of the row while
              // st < H, 2(DC-1-st)+1-odd after (layout.cpp)
              const flt2 v = st < H ? lds_ld<flt2>(rb[r] + st * 16) : lds_ld<flt2>(rb2[r] + (DC - 1 - st) * 16);
              if (st < H) par[r] ^= (unsigned)__float_as_int(v.y);
              m[r] = flt2{v.x, fabsf(v.y)};  // clear the decision bit
            }
          }
          if (st < H) {
#pragma unroll
            for (int r = 0; r < RC; ++r)
              if (st > 0) x[r][st] = s[r];  // (x[.][0] is the boundary (1, 0), applied as such below)
          } else {
            // c2v of edge (odd ? st : DC-1-st) from (own state at DC-1-st, partner state at st)
#pragma unroll
            for (int r = 0; r < RC; ++r) {
              const flt2 y = {swap_pair_f(s[r].x), swap_pair_f(s[r].y)};
              float t0, ts;
              if (st == DC - 1) {  // own state is the boundary (1, 0): o y = y exactly
                t0 = y.x;
                ts = y.x + y.y;
              } else {
                const flt2 o = x[r][DC - 1 - st];
                const flt2 p = o * y;                // (o0 y0, o1 y1)
                const flt2 pc = o * flt2{y.y, y.x};  // (o0 y1, o1 y0)
                t0 = p.x + p.y;
                ts = t0 + (pc.x + pc.y);
              }
              float q = t0 * __builtin_amdgcn_rcpf(ts);
              q = q > kClipHi ? kClipHi : q;  // ProbClip (binaryldpccodec.cc:260-263)
              q = q < kClipLo ? kClipLo : q;
              lds_st<float>(wb[r] + (DC - 1 - st) * 16, q);
            }
          }
          if (advance) {
#pragma unroll
            for (int r = 0; r < RC; ++r) {
              if (st == 0) {  // state (1, 0): n = m, its sum not exactly 1
                s[r] = norm2(m[r]);
              } else {
                const flt2 sa = {s[r].x, s[r].x}, sb = {s[r].y, s[r].y};
                // (s0 m0 + s1 m1, s0 m1 + s1 m0)
                s[r] = norm2(sa * m[r] + sb * flt2{m[r].y, m[r].x});
              }
            }
          }
        }
#pragma unroll
        for (int r = 0; r < RC; ++r) syn0[r] = s[r].x;
      }
      // the pair's halves of all RC rows in one word, one swap for the lot (bp_regular.hip)
      unsigned pw = par[0] >> 31;
#pragma unroll
      for (int r = 1; r < RC; ++r) pw = __builtin_amdgcn_alignbit(pw, par[r], 31);
      const bool fail = pw != (unsigned)swap_pair_i32((int)pw);
      if (!wg_any<T / 64>(fail, wflags)) {  // every row satisfied before this CN phase
        conv = true;
        break;
      }
      if constexpr (SYN) {
#pragma unroll
        for (int r = 0; r < RC; ++r)
          if (!odd)  // alpha past the last edge (:274)
            a.syn[(long long)cw * c.M + c.cn_order[r * (T / 2) + (tid >> 1)]] = (double)syn0[r];
      }
    }

    unsigned nxt = 0;  // the next entry, in flight through the epilogue
    if (tid == 0) nxt = atomicAdd(queue, 1u);
    if (a.iter_count > 0) {
      if (a.uu_hat) {
        uint8_t *u = a.uu_hat + (long long)cw * c.K;
        for (int i = tid; i < c.K; i += T) u[i] = cch[ipos[i]];
      }
      if (a.cc_hat) {
        uint8_t *o = a.cc_hat + (long long)cw * c.N;
        for (int v = tid; v < c.N; v += T) o[v] = cch[c.reg_pos[v]];
      }
      if (a.parity_cnt) {
        int cnt = 0;
#pragma unroll
        for (int r = 0; r < RC; ++r) {
          int p = 0;  // ParityCheck of the final decisions
          const int cbase = c.row_ptr[c.cn_order[r * (T / 2) + (tid >> 1)]];
#pragma unroll
          for (int k = 0; k < H; ++k) p ^= cch[c.reg_pos[c.row_col[cbase + (odd ? H + k : k)]]];
          const int full = p ^ swap_pair_i32(p);
          if (!odd) cnt += full;
        }
        if (cnt) atomicAdd(&red[0], cnt);
      }
      if (a.ref_bits) {  // CntErr (sourcesink.cc:29-47): two 64-bit words per wave and round
        const int lane = tid & 63;
        int errs = 0;
        for (int w0 = tid >> 6; w0 < c.Kw; w0 += 2 * (T / 64)) {
          const int w1 = w0 + T / 64;
          const uint64_t r0 = refw[w0];
          const uint64_t r1 = w1 < c.Kw ? refw[w1] : 0ull;
          const int i0 = w0 * 64 + lane, i1 = w1 * 64 + lane;
          const int b0 = i0 < c.K ? cch[ipos[i0]] : 0;
          const int b1 = i1 < c.K && w1 < c.Kw ? cch[ipos[i1]] : 0;
          const uint64_t m0 = __ballot(b0), m1 = __ballot(b1);
          errs += __popcll(m0 ^ r0) + (w1 < c.Kw ? __popcll(m1 ^ r1) : 0);
        }
        if (lane == 0 && errs) atomicAdd(&red[1], errs);
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
        wcnt[CNT_VN_PHASES] += vn;
        wcnt[CNT_CN_PHASES] += (unsigned long long)iter;
        if (conv) wcnt[CNT_CONVERGED] += 1;
        if (a.ref_bits && a.iter_count > 0) {
          const int errs = red[1];
          wcnt[CNT_ERR_BIT] += (unsigned long long)errs;
          wcnt[CNT_ERR_BLK] += errs > 0 ? 1ull : 0ull;
          wcnt[CNT_TOT_BIT] += (unsigned long long)c.K;
          wcnt[CNT_TOT_BLK] += 1ull;
        }
      }
      red[3] = (int)nxt;  // after the reads above; read by all after the loop's barrier
      red[0] = 0;
      red[1] = 0;
    }
  }
  if (cnt_lds && tid == 0)  // the workgroup's sums (only thread 0 wrote them)
    for (int i = 0; i <= CNT_CONVERGED; ++i)
      if (wcnt[i]) atomicAdd(&a.counters[i], wcnt[i]);
}

template <int T, int RV, int RC, int DV, int DC, bool SYN, int DMB, bool EXACT>
hipError_t launch_f32_one(const DevCode &c, const BpLaunch &a, hipStream_t s) {
  auto kern = bp_regular_f32_kernel<T, RV, RC, DV, DC, SYN, DMB, EXACT>;
  return launch_persistent(kern, T, f32_lds_bytes(c.E, c.N, c.K), 1, kNoGridCap, false, a, s, c, a, a.queue);
}

// Without the fused demap there is no FAST division and one launch; with it,
// the FAST-demap launch, then the exact-demap launch over its defer list.
template <int T, int RV, int RC, int DV, int DC, bool SYN, int DMB>
hipError_t launch_f32_t(const DevCode &c, const BpLaunch &a, hipStream_t s) {
  const size_t lds = f32_lds_bytes(c.E, c.N, c.K);
  if (lds > kLdsLimit || c.N > c.E || c.K > 65536 || c.N > 65536 || c.Kw > kF32MaxKw) return hipErrorNotSupported;
  if constexpr (DMB == 0) {
    return launch_f32_one<T, RV, RC, DV, DC, SYN, 0, true>(c, a, s);
  } else {
    return launch_fast_then_exact(
        a, s, [&](const BpLaunch &b) { return launch_f32_one<T, RV, RC, DV, DC, SYN, DMB, false>(c, b, s); },
        [&](const BpLaunch &b) { return launch_f32_one<T, RV, RC, DV, DC, SYN, DMB, true>(c, b, s); });
  }
}

}  // namespace

bool bp_regular_f32_supported(const DevCode &c) {
  return c.reg_c2v && c.reg_pos && bp_regular_threads(c.N, c.M, c.E, c.dv_max, c.dc_max, c.regular) == 768 &&
         f32_lds_bytes(c.E, c.N, c.K) <= kLdsLimit && c.N <= c.E && c.Kw <= kF32MaxKw;
}

hipError_t launch_bp_regular_f32(const DevCode &c, const BpLaunch &a, hipStream_t s) {
  if (!bp_regular_f32_supported(c)) return hipErrorNotSupported;
  if (a.sym_y) {
    if (!bp_regular_fuses_demap(c, a.sym_bits) || a.cw_idx || a.p0_sel) return hipErrorNotSupported;
    return a.syn ? launch_f32_t<768, 3, 3, 3, 6, true, 2>(c, a, s) : launch_f32_t<768, 3, 3, 3, 6, false, 2>(c, a, s);
  }
  return a.syn ? launch_f32_t<768, 3, 3, 3, 6, true, 0>(c, a, s) : launch_f32_t<768, 3, 3, 3, 6, false, 0>(c, a, s);
}

}  // namespace kml
