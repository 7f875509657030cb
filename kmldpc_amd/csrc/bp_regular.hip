// bp_regular.hip — BP decoder specialised for regular (dv, dc) codes whose
// message state fits in LDS (PEG2304: dv = 3, dc = 6, 6912 edges).
//
// Arithmetic: bit-exact restatement of lab::BinaryLDPCCodec::Decoder
// (lib/lab/src/binaryldpccodec.cc:165-278), like bp.hip.
//
// Mapping onto a gfx950 CU (one workgroup of T threads per CU, all message
// slots in LDS, persistent over codewords via a dequeue counter):
//   * VN phase: thread t owns columns vn_order[r*T + t], r < RV, exactly
//     (N == RV*T): no predicates, RV independent chains per thread.
//   * CN phase: every check row is shared by an adjacent lane PAIR.  The even
//     lane runs the forward trellis (alpha, binaryldpccodec.cc:237-249) over the
//     row's v2c messages, the odd lane the backward trellis (beta, :251-273)
//     over the same messages in reverse; the lanes then swap the chain states
//     they need through one DPP quad_perm per word, and each computes half of
//     the row's c2v outputs.  c2v_k = clip(t0 / (t0 + t1)) with
//     t0 = a0*b0 + a1*b1, t1 = a0*b1 + a1*b0 is symmetric in (alpha_k, beta_k)
//     under IEEE arithmetic (products commute, the two-term sums commute), so
//     both lanes evaluate the same formula on (own state, partner state) and
//     the result is the reference's bit for bit.  2M == RC*T half-rows:
//     the CN phase has exactly as many lanes busy as the VN phase.
//   * the early-stop parity check rides on the CN phase: the VN phase leaves
//     each column's decision in the sign bit of its q1 words, each lane XORs
//     the ones of its half-row as its chain loads them, and the pair combines
//     the halves of its RC rows, packed into one word, through one DPP swap;
//     the workgroup OR is one barrier, one LDS byte per wave going in and one
//     LDS read and a scalar test coming out (bp_common.hpp wg_any2).  Measured
//     against the dword-per-wave vote it replaced, same box: the last waves'
//     wait at the CN phase's closing barrier 585 -> 400 cycles per phase,
//     8.59 -> 8.44 ms per step (-1.7%; profiles/r08_ab_headline_summary.txt).
//   * wave priorities: falling by step in the VN phase, by wave age in the CN
//     phase (kCnAgePrio).
//   * LDS placement (layout.hpp): the columns' lane assignment is annealed on
//     the host against the VN phase's bank conflicts, the hard decisions are
//     stored by lane position (contiguous byte stores), rows are stored in CN
//     position order with the lane pair's edges interleaved (the pair reads
//     slots 2st, 2st+1 of its row at step st: a per-lane base register plus an
//     immediate offset, conflict-free), and a c2v message goes to the lower or
//     upper half of its slot by bit 2 of the row's CN position.  The VN phase
//     reads it at the planned byte offset.
//   * every LDS address is kept absolute in a register (bp_common.hpp lds_ld).
#include <cstdlib>

#include <type_traits>

#include "bp_common.hpp"
#include "bp_launch.hpp"
#include "demap_common.hpp"
#include "kernels.hpp"

namespace kml {

namespace {

constexpr int kRedBytes = 16;

// Phase timing (stamps build, -DKML_STAMPS=1; tools/reg_stamps.py): thread 0's
// s_memtime deltas summed per workgroup in registers, flushed at the end:
// [0] queue + barrier, [1] demap / P0, [2] priors + barrier, [3] iterations,
// [4] epilogue (outputs, counts) + barrier, [5] result atomics, [6] codewords,
// [7] iterations run (CN phases).
#ifndef KML_STAMPS
#define KML_STAMPS 0
#endif
// CN-phase wave priorities: s > 0 ranks the waves by age (the youngest third
// highest) until step s, then all at 0 — the oldest waves otherwise win the
// arbiter's age tie-break and finish 1.2K cycles before the youngest (per-wave
// stamps); measured 5 (-0.7..0.9%) against falling-by-step (0), 2, 3 and 6.
// VN priorities by wave age for the whole phase measured +4%: they fall by step.
constexpr int kCnAgePrio = 5;
// Epilogue latency (stamps: 5.4 K + 1.3 K of ~180 K cycles per codeword): the
// codeword's reference bits for CntErr go straight from global memory into LDS
// in its prologue (global_load_lds: no register holds them, the latency hides
// under the demap / prior check instead of opening the epilogue), and the
// workgroup sums its counters in LDS, flushed with one global atomic each when
// the workgroup leaves.
//
// The next queue entry is taken at the start of a codeword's epilogue (thread
// 0's atomic in flight under CntErr and the epilogue's barrier) instead of
// between two barriers at the top of the loop: one barrier and the atomic's
// round trip leave the per-codeword critical path.
//
// The VN phase of iteration 0 in closed form (FAST decodes only).  InitMsg sets
// every c2v to (0.5, 0.5), and with a prior p in the FAST domain (+0, 1, or p
// and 1 - p >= 2^(40 dv - 960): bp_common.hpp fast_prior_ok) the column chain
// (binaryldpccodec.cc:177-212) is the identity on a = (p, RN(1 - p)):
//   forward: n = (a0 / 2, a1 / 2), exact halvings (no subnormals in the
//     domain); s = RN(a0 / 2 + a1 / 2) = RN(p + RN(1 - p)) / 2 = 1/2, because
//     p + RN(1 - p) rounds to exactly 1 (bp_common.hpp, "first backward
//     step"); (a0 / 2) / (1/2) = a0 exactly.  So every alpha, the column head
//     included, is a, and the decision is a0 > a1 ? 0 : 1.
//   backward: beta = (1, 1) gives t = a, sum 1, v2c = a; the next beta is
//     (0.5, 0.5) / 1, then (0.25, 0.25) / 0.5 = (0.5, 0.5), ...: t = a / 2,
//     sum 1/2, v2c = a.
// Every v2c of the column is (p, RN(1 - p)) for any column degree
// (tests/test_iter0_model.py restates the recursion in IEEE doubles): DV slot
// stores and one decision byte per column, no division and nothing to prove,
// so iteration 0 cannot raise the suspect flag itself (a forced one, sus0,
// still reaches the first closing barrier).  The exact kernel keeps the
// generic chain: its priors may be -0.0, subnormal or NaN, where the identity
// fails.  Measured alone, same box: 9.02 -> 8.69 ms per step (-3.7%;
// profiles/r07_ab_headline_summary.txt).
//
// Without syndrome output (SYN = false) nothing the CN phase of the last
// iteration of the budget writes is read again: the c2v slots feed only a next
// VN phase, the chain states only the soft syndromes, and the reference returns
// right after it (binaryldpccodec.cc:235-277).  What the decode still needs
// from that phase is the parity check that rides on it (ret, conv, the
// counters), so the phase loads the decision words of its half-rows (the high
// dwords of the q1 values) and votes: no trellis, no c2v stores, no DPP state
// swaps.  The phase still counts as run (iter, CNT_CN_PHASES).  Measured alone,
// same box: 9.02 -> 8.93 ms per step (-1.0%); with the closed-form iteration
// 0: 8.58 ms (-4.9%).
//
// The budget's last VN phase (SYN = false): that parity check reads only the
// decision bit, the sign of the high word of each slot's q1, so of the last
// iteration's VN phase only the forward chain and hard_decision are live: the
// backward pass of a column (three proven pair-divisions, the near-one one and
// three 16-byte stores) writes messages nobody reads.  The last iteration is
// peeled out of the loop (decode_reg, below the loop: the loop holds the
// generic iteration alone, and the peeled column code cannot disturb its
// register allocation): per column the generic forward chain as it stands
// (the same div2 calls, the same rerun when a quotient is unproven, the same
// hard_decision), the decision byte, and hb << 31 into the +12 word of each
// of the column's slots; then the barrier, the nine sign words read together
// and the same vote.  No numerical argument is needed: the decisions are the
// generic chain's own.  With a budget of 1 the peeled iteration is iteration
// 0 and takes the closed form's decision on the FAST path.  The redo decision
// is the loop's: sus is raised only by a forced redo (sus0) -- div2 sets a
// flag only in its DEFER form, whose flag is the column's `bad` (the column
// is rerun, settling each quotient), and the backward pass's unit-beta step
// and hard_decision call forms that settle or need no proof -- so dropping
// the backward pass drops no redo, and CNT_REDONE is the parent's.
constexpr int kRegMaxKw = 64;  // K <= N <= 2304 (bp_regular_threads): 36 words
#if KML_STAMPS
__device__ unsigned long long kml_reg_stamps[8];
// per wave (lane 0), summed over codewords: [0] VN compute, [1] VN barrier
// wait, [2] CN compute, [3] CN barrier wait (+ OR)
__device__ unsigned long long kml_reg_wave_stamps[16][4];
#define REG_WSTAMP(i)                                              \
  do {                                                             \
    if ((threadIdx.x & 63) == 0) {                                 \
      const unsigned long long _t = __builtin_amdgcn_s_memtime();  \
      ws_acc[(i)] += _t - ws_prev;                                 \
      ws_prev = _t;                                                \
    }                                                              \
  } while (0)
#define REG_STAMP(i)                                               \
  do {                                                             \
    if (tid == 0) {                                                \
      const unsigned long long _t = __builtin_amdgcn_s_memtime();  \
      rs_acc[(i)] += _t - rs_prev;                                 \
      rs_prev = _t;                                                \
    }                                                              \
  } while (0)
#else
#define REG_STAMP(i) \
  do {               \
  } while (0)
#define REG_WSTAMP(i) \
  do {                \
  } while (0)
#endif

// swap a double with the adjacent lane (quad_perm [1,0,3,2])
__device__ __forceinline__ double swap_pair(double x) {
  const int lo = __double2loint(x), hi = __double2hiint(x);
  const int lo2 = __builtin_amdgcn_mov_dpp(lo, 0xB1, 0xF, 0xF, false);
  const int hi2 = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xF, 0xF, false);
  return __hiloint2double(hi2, lo2);
}
__device__ __forceinline__ int swap_pair_i(int x) { return __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, false); }
// x (>= +0 or NaN) with its sign bit set to bit
__device__ __forceinline__ double with_sign(double x, int bit) {
  return __hiloint2double((__double2hiint(x) & 0x7FFFFFFF) | (bit << 31), __double2loint(x));
}

// PROF: CntErr of one iteration's decisions (the epilogue's, word for word),
// added into *perr; run by every wave between the VN phase's closing barrier
// and the CN phase's vote.
template <int T>
__device__ __forceinline__ void prof_count(const DevCode &c, const unsigned char *cch, const unsigned short *ipos,
                                           const uint64_t *refw, int *perr) {
  const int lane = threadIdx.x & 63;
  int errs = 0;
  for (int w0 = threadIdx.x >> 6; w0 < c.Kw; w0 += 2 * (T / 64)) {
    const int w1 = w0 + T / 64;
    const uint64_t r0 = refw[w0];
    const uint64_t r1 = w1 < c.Kw ? refw[w1] : 0ull;
    const int i0 = w0 * 64 + lane, i1 = w1 * 64 + lane;
    const int b0 = i0 < c.K ? cch[ipos[i0]] : 0;
    const int b1 = i1 < c.K && w1 < c.Kw ? cch[ipos[i1]] : 0;
    const uint64_t m0 = __ballot(b0), m1 = __ballot(b1);
    errs += __popcll(m0 ^ r0) + (w1 < c.Kw ? __popcll(m1 ^ r1) : 0);
  }
  if (lane == 0 && errs) atomicAdd(perr, errs);
}

// Returns true when a FAST decode met a quotient dd_check could not prove
// correctly rounded (exact_div.hpp): the caller redoes the codeword with
// FAST = false.  The decision is taken at the CN phase's closing barrier,
// before that iteration's syndromes are written, so everything a suspect
// decode wrote (slots, decisions, syndromes of earlier iterations) is what the
// exact decode rewrites identically or overwrites.
//
// PROF (iteration profile, kernels.hpp BpLaunch::cw_prof / prof): after the VN
// phase's closing barrier of iteration iter the decision bytes are that
// iteration's hard decisions (what a decode with budget iter + 1 returns unless
// it converged earlier), and nothing writes them before the next VN phase,
// which starts after the CN phase's closing wg_any.  Between the two barriers
// every wave counts its info-bit words against refw exactly as the epilogue's
// CntErr does and adds the sum into perr[iter] (LDS, zeroed by the caller
// before the loop's first barrier): no barrier of its own.
template <int T, int RV, int RC, int DV, int DC, bool SYN, bool FAST, bool PROF = false>
__device__ __forceinline__ bool decode_reg(const DevCode &c, const BpLaunch &a, int cw, unsigned char *smem,
                                           unsigned hd, const unsigned (&vaddr)[RV][DV], const double (&pv)[RV],
                                           const int (&crow)[RC], const unsigned (&rb)[RC], const unsigned (&rb2)[RC],
                                           const unsigned (&wb)[RC], int odd, int &iter_out, bool &conv_out,
                                           bool sus0 = false, const unsigned char *cch = nullptr,
                                           const unsigned short *ipos = nullptr, const uint64_t *refw = nullptr,
                                           int *perr = nullptr) {
  static_assert(DC % 2 == 0, "the lane-pair split assumes an even row degree");
  constexpr int H = DC / 2;
  __shared__ WgVotes wflags;  // wg_any (bp_common.hpp)
  int iter = 0;
  bool conv = false, sus = sus0;
#if KML_STAMPS
  unsigned long long ws_acc[4] = {0, 0, 0, 0}, ws_prev = __builtin_amdgcn_s_memtime();
#endif
  // SYN == false: the budget's last iteration is peeled (below the loop)
  const int loop_end = SYN ? a.iter_count : a.iter_count - 1;
  for (; iter < loop_end; ++iter) {
    // Wave priorities (s_setprio) fall as a wave advances through a phase, so
    // the SIMD arbiter (priority, then age) favours the waves that are behind:
    // the 3 waves of a SIMD reach the barrier together instead of the oldest
    // finishing first and the youngest running its dependent chains alone.
    // Measured: per-phase end-time spread 3100 -> 500 cycles, kernel -2.5%.
    __builtin_amdgcn_s_setprio(3);
    // The RV columns' chains are interleaved step by step in program order so
    // their dependent fma / rcp sequences overlap.  On the FAST path the
    // boundary state beta = (1, 1) is applied as the identity (x * 1.0 == x).
    if (FAST && iter == 0) {  // every v2c is the prior pair (proof above: "The VN phase of iteration 0")
#pragma unroll
      for (int r = 0; r < RV; ++r) {
        // an opaque copy: 1 - p would otherwise be shared with the generic
        // chain's and hoisted out of the iteration loop (RV more doubles live
        // through it: +32 bytes of private segment)
        double p = pv[r];
        asm volatile("" : "+v"(p));
        const double a1 = 1.0 - p;
        const int hb = p > a1 ? 0 : 1;
        const dbl2 m = dbl2{p, with_sign(a1, hb)};
#pragma unroll
        for (int k = 0; k < DV; ++k) lds_st<dbl2>(vaddr[r][k] & ~15u, m);
        lds_st<unsigned char>(hd + r * T, (unsigned char)hb);
      }
      __builtin_amdgcn_s_setprio(0);
    } else {
      // InitMsg (binaryldpccodec.cc:166-170): every c2v is 0.5 before the
      // first CN phase, so iteration 0 takes the constant instead of slots
      // initialised in LDS (every slot is written before it is read)
      double c0s[RV][DV];
#pragma unroll
      for (int r = 0; r < RV; ++r)
#pragma unroll
        for (int k = 0; k < DV; ++k) c0s[r][k] = iter == 0 ? 0.5 : lds_ld<double>(vaddr[r][k]);
      // one column's chains at a time (registers: see bp_coop.hip).  FAST: the
      // column's quotients unsettled (div2 DEFER), and in the rare case that
      // one of them could not be proven the column runs again settling each
      // (its slot and decision stores are rewritten before the barrier).
#pragma unroll
      for (int r = 0; r < RV; ++r) {
        auto column = [&](auto defer) -> bool {
          constexpr bool D = FAST && decltype(defer)::value;
          bool bad = false;
          double a0 = pv[r], a1 = 1.0 - pv[r], al0[DV], al1[DV];
          int hb = 0;
#pragma unroll
          for (int k = 0; k < DV; ++k) {
            al0[k] = a0;
            al1[k] = a1;
            const double c0 = c0s[r][k];
            const double n0 = a0 * c0;
            const double n1 = a1 * (1.0 - c0);
            if (k + 1 < DV)
              div2<FAST, false, D>(n0, n1, n0 + n1, a0, a1, bad);
            else {  // the posterior only feeds the hard decision
              hb = hard_decision<FAST>(n0, n1, sus);
              lds_st<unsigned char>(hd + r * T, (unsigned char)hb);
            }
          }
          double b0 = 1.0, b1 = 1.0;
#pragma unroll
          for (int k = DV - 1; k >= 0; --k) {
            const bool unit = FAST && k == DV - 1;  // beta = (1, 1)
            const double t0 = unit ? al0[k] : al0[k] * b0;
            const double t1 = unit ? al1[k] : al1[k] * b1;
            double q0, q1;
            if (unit)
              div2<FAST, true>(t0, t1, t0 + t1, q0, q1, sus);
            else
              div2<FAST, false, D>(t0, t1, t0 + t1, q0, q1, bad);
            lds_st<dbl2>(vaddr[r][k] & ~15u, dbl2{q0, with_sign(q1, hb)});
            if (k > 0) {
              const double c0 = c0s[r][k];
              if (unit) {
                b0 = c0;
                b1 = 1.0 - c0;
              } else {
                div2<FAST, false, D>(b0 * c0, b1 * (1.0 - c0), b0 * c0 + b1 * (1.0 - c0), b0, b1, bad);
              }
            }
          }
          return bad;
        };
        if (column(std::true_type{})) column(std::false_type{});
        if (r == RV / 2) __builtin_amdgcn_s_setprio(1);
      }
      __builtin_amdgcn_s_setprio(0);
    }
    REG_WSTAMP(0);
    __syncthreads();
    REG_WSTAMP(1);
    if constexpr (PROF) prof_count<T>(c, cch, ipos, refw, &perr[iter]);

    // The early-stop parity check rides on the CN phase: in steps 0..H-1 the
    // even lane loads the row's edges [0, H) and the odd lane [H, DC), whose
    // q1 words carry the columns' decisions in their sign bits.  The OR over
    // the workgroup is folded into the CN phase's closing barrier: the CN
    // phase runs speculatively, and a converged codeword (no failing row)
    // discards it — its slots are never read again and its syndromes are only
    // written when the phase counts.
    unsigned par[RC];

    // ------------------------------------------------------------ CN phase
    double syn0[RC];
    // Step s of the even lane advances alpha over edge s, of the odd lane beta
    // over edge DC-1-s.  From step H on, the pair swaps the chain states and
    // each lane finishes one c2v per step.  Within a step every message LOAD is
    // issued before the c2v STOREs (the partner's store of this step hits the
    // slot the lane is about to read), and LDS executes a wave's operations in
    // program order.
    {  // (the budget's last CN phase without syndrome output is below the loop)
      double x0[RC][H], x1[RC][H];  // lower-half chain states, kept for the swap
      double s0[RC], s1[RC];        // current chain state
#pragma unroll
      for (int r = 0; r < RC; ++r) {
        s0[r] = 1.0;
        s1[r] = 0.0;
        par[r] = 0;
      }
      {  // the youngest waves start the CN phase at the highest priority
        const int grp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) / 4;  // 0 oldest .. 2 youngest
        if (grp >= 2) __builtin_amdgcn_s_setprio(3);
        else if (grp == 1) __builtin_amdgcn_s_setprio(2);
        else __builtin_amdgcn_s_setprio(1);
      }
#pragma unroll
      for (int st = 0; st < DC; ++st) {
        if (st == kCnAgePrio) __builtin_amdgcn_s_setprio(0);
        const bool advance = SYN || st + 1 < DC;
        double m0[RC], m1[RC];
        if (advance) {
#pragma unroll
          for (int r = 0; r < RC; ++r) {
            // edge (odd ? DC-1-st : st): physical slot 2st+odd of the row while
            // st < H, 2(DC-1-st)+1-odd after (layout.cpp)
            const dbl2 m = st < H ? lds_ld<dbl2>(rb[r] + st * 32) : lds_ld<dbl2>(rb2[r] + (DC - 1 - st) * 32);
            if (st < H) par[r] ^= (unsigned)__double2hiint(m.y);
            m0[r] = m.x;
            m1[r] = fabs(m.y);  // clear the decision bit
          }
        }
        if (st < H) {
#pragma unroll
          for (int r = 0; r < RC; ++r) {
            x0[r][st] = s0[r];
            x1[r][st] = s1[r];
          }
        } else {
          // c2v of edge (odd ? st : DC-1-st) from (own state at DC-1-st, partner state at st)
          double t0[RC], ts[RC], q[RC];
#pragma unroll
          for (int r = 0; r < RC; ++r) {
            const double y0 = swap_pair(s0[r]);
            const double y1 = swap_pair(s1[r]);
            const double o0 = x0[r][DC - 1 - st], o1 = x1[r][DC - 1 - st];
            const bool unit = FAST && st == DC - 1;  // own state is the boundary (1, 0)
            t0[r] = unit ? y0 : o0 * y0 + o1 * y1;
            ts[r] = t0[r] + (unit ? y1 : o0 * y1 + o1 * y0);
          }
          cn_c2v_rows<RC, FAST>(t0, ts, q);  // the sums are within ulps of 1 (bp_common.hpp)
#pragma unroll
          for (int r = 0; r < RC; ++r) lds_st<double>(wb[r] + (DC - 1 - st) * 32, q[r]);
        }
        if (advance) {
          double n0[RC], n1[RC];
#pragma unroll
          for (int r = 0; r < RC; ++r) {
            const bool unit = FAST && st == 0;  // state (1, 0)
            n0[r] = unit ? m0[r] : s0[r] * m0[r] + s1[r] * m1[r];
            n1[r] = unit ? m1[r] : s0[r] * m1[r] + s1[r] * m0[r];
          }
          cn_norm_rows<RC, FAST>(n0, n1, s0, s1);
        }
      }
#pragma unroll
      for (int r = 0; r < RC; ++r) syn0[r] = s0[r];
    }
    // the pair's halves of all RC rows in one word (row r's sign bit ends up at
    // bit RC-1-r: each alignbit shifts the word left and brings the next row's
    // bit 31 in at bit 0), one swap for the lot
    unsigned pw = par[0] >> 31;
#pragma unroll
    for (int r = 1; r < RC; ++r) pw = __builtin_amdgcn_alignbit(pw, par[r], 31);
    const bool fail = pw != (unsigned)swap_pair_i((int)pw);
    REG_WSTAMP(2);
    const int wg = FAST ? wg_any2<T / 64>(fail, sus, wflags) : wg_any<T / 64>(fail, wflags);
    REG_WSTAMP(3);
    if (FAST && (wg & 2)) {  // an unproven quotient in this VN phase: redo exactly
      iter_out = iter;
      conv_out = false;
      return true;
    }
    if (!(wg & 1)) {  // every row satisfied before this CN phase
      conv = true;
      break;
    }
    if constexpr (SYN) {
#pragma unroll
      for (int r = 0; r < RC; ++r)
        if (!odd) a.syn[(long long)cw * c.M + crow[r]] = syn0[r];  // alpha past the last edge (:274)
    }
  }
  // The budget's last iteration without syndrome output, peeled (argument in
  // the header: "The budget's last VN phase"): below the loop, so that its
  // column code is not merged with the loop's.
  if constexpr (!SYN) {
    if (!conv && iter + 1 == a.iter_count) {
#if KML_STAMPS
      unsigned long long hot_acc[4];
      for (int i = 0; i < 4; ++i) {
        hot_acc[i] = ws_acc[i];
        ws_acc[i] = 0;
      }
#endif
      __builtin_amdgcn_s_setprio(3);
      int hbs[RV];
      if (FAST && iter == 0) {  // budget 1: the closed form's decisions
#pragma unroll
        for (int r = 0; r < RV; ++r) {
          double p = pv[r];
          asm volatile("" : "+v"(p));
          hbs[r] = p > 1.0 - p ? 0 : 1;
        }
      } else {
        double c0s[RV][DV];
#pragma unroll
        for (int r = 0; r < RV; ++r)
#pragma unroll
          for (int k = 0; k < DV; ++k) c0s[r][k] = iter == 0 ? 0.5 : lds_ld<double>(vaddr[r][k]);
        // The generic column's forward chain, as it stands in the loop.  It
        // is one dependent sequence per column (the loop's column overlaps it
        // with its backward chains), so the RV columns' deferring chains run
        // as one straight-line block that the scheduler interleaves; then the
        // rare reruns, then the decisions.
        double n0[RV], n1[RV];
        bool bad[RV];
        auto head = [&](int r, auto defer) {
          constexpr bool D = FAST && decltype(defer)::value;
          bad[r] = false;
          double a0 = pv[r], a1 = 1.0 - pv[r];
#pragma unroll
          for (int k = 0; k < DV; ++k) {
            const double c0 = c0s[r][k];
            n0[r] = a0 * c0;
            n1[r] = a1 * (1.0 - c0);
            if (k + 1 < DV) div2<FAST, false, D>(n0[r], n1[r], n0[r] + n1[r], a0, a1, bad[r]);
          }
        };
#pragma unroll
        for (int r = 0; r < RV; ++r) head(r, std::true_type{});
#pragma unroll
        for (int r = 0; r < RV; ++r)
          if (bad[r]) head(r, std::false_type{});
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int r = 0; r < RV; ++r) hbs[r] = hard_decision<FAST>(n0[r], n1[r], sus);  // the posterior's only use
      }
      // the decision byte, and the decision bit where the parity check below
      // reads it: the high word of each of the column's slots
#pragma unroll
      for (int r = 0; r < RV; ++r) {
        lds_st<unsigned char>(hd + r * T, (unsigned char)hbs[r]);
#pragma unroll
        for (int k = 0; k < DV; ++k) lds_st<unsigned>((vaddr[r][k] & ~15u) + 12, (unsigned)hbs[r] << 31);
      }
      __builtin_amdgcn_s_setprio(0);
      REG_WSTAMP(0);
      __syncthreads();
      REG_WSTAMP(1);
      if constexpr (PROF) prof_count<T>(c, cch, ipos, refw, &perr[iter]);
      // the parity check alone (argument above: "Without syndrome output"):
      // the pair's RC * H sign words, loaded together
      unsigned sw[RC][H];
#pragma unroll
      for (int r = 0; r < RC; ++r)
#pragma unroll
        for (int st = 0; st < H; ++st) sw[r][st] = lds_ld<unsigned>(rb[r] + st * 32 + 12);
      unsigned pw = 0;
#pragma unroll
      for (int r = 0; r < RC; ++r) {
        unsigned x = sw[r][0];
#pragma unroll
        for (int st = 1; st < H; ++st) x ^= sw[r][st];
        pw = r == 0 ? x >> 31 : __builtin_amdgcn_alignbit(pw, x, 31);
      }
      const bool fail = pw != (unsigned)swap_pair_i((int)pw);
      REG_WSTAMP(2);
      const int wg = FAST ? wg_any2<T / 64>(fail, sus, wflags) : wg_any<T / 64>(fail, wflags);
      REG_WSTAMP(3);
#if KML_STAMPS
      if ((threadIdx.x & 63) == 0) {  // the peeled iteration: rows 12..14 by wave group, [15][0] its count
        for (int i = 0; i < 4; ++i) {
          atomicAdd(&kml_reg_wave_stamps[12 + (threadIdx.x >> 8)][i], ws_acc[i]);
          ws_acc[i] = hot_acc[i];
        }
        if (threadIdx.x == 0) atomicAdd(&kml_reg_wave_stamps[15][0], 1ull);
      }
#endif
      if (FAST && (wg & 2)) {  // sus: a forced redo (sus0) alone, as in the loop (header: "The redo decision")
        iter_out = iter;
        conv_out = false;
        return true;
      }
      if (wg & 1)
        ++iter;  // the phase counts as run
      else
        conv = true;
    }
  }
#if KML_STAMPS
  if ((threadIdx.x & 63) == 0)
    for (int i = 0; i < 4; ++i) atomicAdd(&kml_reg_wave_stamps[threadIdx.x >> 6][i], ws_acc[i]);
#endif
  iter_out = iter;
  conv_out = conv;
  return false;
}

// Dynamic LDS: E slots of 16 B, the reduction words, N hard-decision bytes,
// then (fused demap only, 16-byte aligned) the codeword's N priors.
constexpr size_t p0s_offset(int E, int N) { return ((size_t)E * 16 + kRedBytes + (size_t)N + 15) & ~(size_t)15; }
// then the info bits' positions in the decision bytes (u16, K entries), staged
// once per workgroup for the epilogue's CntErr
constexpr size_t ipos_offset(int E, int N, int DMB) {
  return DMB > 0 ? p0s_offset(E, N) + (size_t)N * 8 : (((size_t)E * 16 + kRedBytes + (size_t)N + 1) & ~(size_t)1);
}
constexpr size_t reg_lds_bytes(int E, int N, int K, int DMB) { return ipos_offset(E, N, DMB) + (size_t)K * 2; }

// EXACT = false: the FAST kernel.  It decodes every codeword whose priors
// qualify (bp_common.hpp fast_prior_ok) on the FAST path and appends the rest,
// and every codeword whose FAST decode met an unproven quotient, to the defer
// list (a.defer_idx / a.defer_cnt; no outputs, no counters for those).
// EXACT = true: decodes its entries (the defer list) on the exact path (div_rn).
// Two kernels rather than one with both paths: the exact path's registers
// would otherwise be allocated (and spilled) in the FAST kernel too.
template <int T, int RV, int RC, int DV, int DC, bool SYN, int DMB, bool EXACT, bool PROF = false>
__global__ __launch_bounds__(T) void bp_regular_kernel(DevCode c, BpLaunch a, unsigned int *queue, int fast_allowed) {
  const double plo = fast_prior_lo(c.dv_max);  // FAST prior domain (bp_common.hpp)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ WgVotes pflags;  // wg_all of the FAST prior check (bp_common.hpp)
  // fused demap: the constellation and the exp table in LDS (demap_common.hpp)
  __shared__ double dcons[DMB > 0 ? (2 << DMB) : 2];
  __shared__ uint64_t detab[DMB > 0 ? 256 : 1];
  __shared__ uint64_t refw[kRegMaxKw];                    // this codeword's reference bits
  __shared__ unsigned long long wcnt[CNT_CONVERGED + 1];  // the workgroup's counters
  // PROF: the codeword's error bits per iteration, and the workgroup's sums per
  // budget {err_bit, err_blk, converged} (lane k alone touches wprof[k])
  __shared__ int perr[PROF ? kBpProfMaxIter : 1];
  __shared__ unsigned long long wprof[PROF ? kBpProfMaxIter : 1][3];
  static_assert(!PROF || !SYN, "the iteration profile has no syndrome output");
  double *p0s = reinterpret_cast<double *>(smem + p0s_offset(c.E, c.N));
  if constexpr (DMB > 0) {
    for (int k = threadIdx.x; k < (2 << DMB); k += T) dcons[k] = a.sym_cons[k];
    stage_exp_table(detab);
  }
  constexpr int H = (DC + 1) / 2;
  const int tid = threadIdx.x;
  const int odd = tid & 1;
  int *red = reinterpret_cast<int *>(smem + (size_t)c.E * 16);
  unsigned char *cch = smem + (size_t)c.E * 16 + kRedBytes;

  const unsigned smem_a = lds_addr(smem), cch_a = lds_addr(cch);
  unsigned short *ipos = reinterpret_cast<unsigned short *>(smem + ipos_offset(c.E, c.N, DMB));
  for (int i = tid; i < c.K; i += T) ipos[i] = (unsigned short)c.reg_pos[c.info_off + i];
  int vcol[RV];
  unsigned vaddr[RV][DV];
#pragma unroll
  for (int r = 0; r < RV; ++r) {
    const int v = c.vn_order[r * T + tid];
    const int b = c.col_ptr[v];
    vcol[r] = v;
#pragma unroll
    for (int k = 0; k < DV; ++k) {
      vaddr[r][k] = smem_a + (unsigned)c.reg_c2v[b + k];
      asm volatile("" : "+v"(vaddr[r][k]));
    }
  }
  const int chalf = ((tid >> 3) & 1) * 8;  // bit 2 of the CN position (tid >> 1)
  int crow[RC], cbase[RC];
  unsigned rb[RC], rb2[RC], wb[RC];
#pragma unroll
  for (int r = 0; r < RC; ++r) {
    const int row = c.cn_order[r * (T / 2) + (tid >> 1)];
    crow[r] = row;
    cbase[r] = c.row_ptr[row];
    // the row's slots sit at its CN position, the pair's edges interleaved (layout.cpp)
    rb[r] = smem_a + (unsigned)((r * (T / 2) + (tid >> 1)) * DC + odd) * 16;
    rb2[r] = rb[r] + 16 - 32 * odd;
    wb[r] = rb[r] + chalf;
    asm volatile("" : "+v"(rb[r]), "+v"(rb2[r]), "+v"(wb[r]));
  }

#if KML_STAMPS
  unsigned long long rs_prev = __builtin_amdgcn_s_memtime(), rs_acc[8] = {};
#endif
  const int B = a.B_dev ? (int)*a.B_dev : a.B;  // the exact kernel: the FAST kernel's defer count
  const bool ref_pre = a.ref_bits && a.iter_count > 0;  // (c.Kw <= kRegMaxKw: host check)
  if (a.counters && tid <= CNT_CONVERGED) wcnt[tid] = 0;  // ordered by the loop's first barrier
  if constexpr (PROF)
    if (tid < a.iter_count) wprof[tid][0] = wprof[tid][1] = wprof[tid][2] = 0;
  if (tid == 0) {  // the first entry; then each codeword's epilogue takes the next
    red[3] = (int)atomicAdd(queue, 1u);
    red[0] = 0;
    red[1] = 0;
  }
  for (;;) {
    __syncthreads();
    const int entry = red[3];
    REG_STAMP(0);
    if (entry >= B) break;
    const int cw = a.cw_idx ? a.cw_idx[entry] : entry;
    if constexpr (PROF)  // (the last epilogue's reads are behind the barrier above; the first VN barrier is ahead)
      if (tid < a.iter_count) perr[tid] = 0;
    if (ref_pre && tid < 2 * c.Kw)  // one dword per lane (the first waves), in flight through the prologue
      __builtin_amdgcn_global_load_lds(reinterpret_cast<const unsigned *>(a.ref_bits + (long long)cw * c.Kw) + tid,
                                       (__attribute__((address_space(3))) void *)(reinterpret_cast<unsigned *>(refw) +
                                                                                  (tid & ~63)),
                                       4, 0, 0);
    const double *p0;
    bool dok = true;  // FAST kernel: every symbol's FAST demap proven (else the exact kernel demaps the codeword)
    if constexpr (DMB > 0) {  // ModemLinearSystem::DeMapping of this codeword into LDS
      const int S = c.cc_len / DMB;
      const double2 hh = a.sym_h[(long long)cw * a.sym_h_stride + (a.sym_h_sel ? a.sym_h_sel[cw] : 0)];
      const double2 *yy = a.sym_y + (long long)cw * S;
      for (int j = tid; j < S; j += T) {
        const double2 v = yy[j];
        double out[DMB];
        if constexpr (EXACT)
          demap_symbol_t<DMB, false, lds_cons, false>((lds_cons)dcons, (lds_exptab)detab, v.x, v.y, hh.x, hh.y,
                                                          a.sym_var, out);
        else  // no exact fallback in the FAST kernel (its registers): a failing symbol defers the codeword
          dok &= demap_symbol_t<DMB, true, lds_cons, false>((lds_cons)dcons, (lds_exptab)detab, v.x, v.y, hh.x,
                                                              hh.y, a.sym_var, out);
#pragma unroll
        for (int b = 0; b < DMB; ++b) p0s[j * DMB + b] = out[b];
      }
      __syncthreads();
      p0 = p0s;
    } else {
      p0 = a.p0 + (long long)cw * a.p0_stride;
      if (a.p0_sel) p0 += (long long)a.p0_sel[cw] * a.p0_sel_stride;
    }

    REG_STAMP(1);
    double pv[RV];
    bool ok = dok;
#pragma unroll
    for (int r = 0; r < RV; ++r) {
      pv[r] = (vcol[r] >= c.punct) ? p0[vcol[r] - c.punct] : 0.5;
      ok = ok && fast_prior_ok(pv[r], plo);
    }
    // the LDS writes land before wave 0 passes the next barrier (the barriers wait lgkmcnt only)
    if (ref_pre) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const bool fast = wg_all<T / 64>(ok, pflags) && (fast_allowed & 1);
    REG_STAMP(2);

    int iter = 0;
    bool conv = false;
    if constexpr (!EXACT) {
      bool defer = !fast;
      if (fast && decode_reg<T, RV, RC, DV, DC, SYN, true, PROF>(c, a, cw, smem, cch_a + tid, vaddr, pv, crow, rb, rb2,
                                                                 wb, odd, iter, conv, (fast_allowed & 2) != 0, cch, ipos,
                                                                 refw, perr)) {
        defer = true;  // an unproven quotient: the exact kernel redoes the codeword
        if (tid == 0 && a.counters) atomicAdd(&a.counters[CNT_REDONE], 1ull);
      }
      if (defer) {
        if (tid == 0) {
          a.defer_idx[atomicAdd(a.defer_cnt, 1u)] = cw;
          red[3] = (int)atomicAdd(queue, 1u);  // (every thread has read red[3])
        }
        continue;
      }
    } else {
      decode_reg<T, RV, RC, DV, DC, SYN, false, PROF>(c, a, cw, smem, cch_a + tid, vaddr, pv, crow, rb, rb2, wb, odd,
                                                     iter, conv, false, cch, ipos, refw, perr);
    }

    REG_STAMP(3);
    unsigned nxt = 0;  // the next entry, in flight through the epilogue
    if (tid == 0) nxt = atomicAdd(queue, 1u);
#if KML_STAMPS
    if (tid == 0) {
      rs_acc[6] += 1;
      rs_acc[7] += (unsigned long long)iter;
    }
#endif
    if (a.iter_count > 0) {
      if (a.uu_hat) {
        uint8_t *u = a.uu_hat + (long long)cw * c.K;
        for (int i = tid; i < c.K; i += T) u[i] = cch[c.reg_pos[i + c.info_off]];
      }
      if (a.cc_hat) {
        uint8_t *o = a.cc_hat + (long long)cw * c.N;
        for (int v = tid; v < c.N; v += T) o[v] = cch[c.reg_pos[v]];
      }
      if (a.parity_cnt) {
        int cnt = 0;
#pragma unroll
        for (int r = 0; r < RC; ++r) {
          int p = 0;  // ParityCheck of the final decisions (once per codeword: the columns from global)
#pragma unroll
          for (int k = 0; k < H; ++k) {
            const int e = odd ? DC / 2 + k : k;
            p ^= cch[c.reg_pos[c.row_col[cbase[r] + (e < DC ? e : DC - 1)]]];
          }
          const int full = p ^ swap_pair_i(p);
          if (!odd) cnt += full;
        }
        if (cnt) atomicAdd(&red[0], cnt);
      }
      if (a.ref_bits) {  // CntErr (sourcesink.cc:29-47): two 64-bit words per wave and round, loads first
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
    REG_STAMP(4);
    if constexpr (PROF) {
      // Budget k + 1 returns the decisions of iteration min(k, last), last = the
      // last iteration whose VN phase ran; it converged when the parity check
      // passed at an iteration <= k.  Only a decode that finished gets here: a
      // deferred FAST decode left its counts in perr, zeroed again above.
      if (tid < a.iter_count) {
        const int last = conv ? iter : a.iter_count - 1;
        const int e = perr[tid < last ? tid : last];
        if (a.cw_prof) a.cw_prof[(long long)cw * a.cw_prof_stride + tid] = e;
        wprof[tid][0] += (unsigned long long)e;
        wprof[tid][1] += e > 0 ? 1ull : 0ull;
        wprof[tid][2] += conv && iter <= tid ? 1ull : 0ull;
      }
    }
    if (tid == 0) {
      if (a.ret) a.ret[cw] = iter + (iter < a.max_iter);
      if (a.parity_cnt) a.parity_cnt[cw] = red[0];
      if (a.cw_err && a.ref_bits) a.cw_err[cw] = a.iter_count > 0 ? red[1] : 0;
      if (a.iters) a.iters[cw] = iter;
      if (a.counters) {  // (summed in LDS: flushed at the exit)
        const unsigned long long vn = conv ? (unsigned long long)iter + 1 : (unsigned long long)iter;
        atomicAdd(&wcnt[CNT_VN_PHASES], vn);
        atomicAdd(&wcnt[CNT_CN_PHASES], (unsigned long long)iter);
        if (conv) atomicAdd(&wcnt[CNT_CONVERGED], 1ull);
        if (a.ref_bits && a.iter_count > 0) {
          const int errs = red[1];
          atomicAdd(&wcnt[CNT_ERR_BIT], (unsigned long long)errs);
          atomicAdd(&wcnt[CNT_ERR_BLK], errs > 0 ? 1ull : 0ull);
          atomicAdd(&wcnt[CNT_TOT_BIT], (unsigned long long)c.K);
          atomicAdd(&wcnt[CNT_TOT_BLK], 1ull);
        }
      }
      // after the reads above; read by all after the loop's barrier
      red[3] = (int)nxt;
      red[0] = 0;
      red[1] = 0;
    }
    REG_STAMP(5);
  }
  if (a.counters && tid == 0)  // the workgroup's sums (only thread 0 wrote them)
    for (int i = 0; i <= CNT_CONVERGED; ++i)
      if (wcnt[i]) atomicAdd(&a.counters[i], wcnt[i]);
  if constexpr (PROF)
    if (a.prof && tid < a.iter_count)  // (lane k's own sums)
      for (int j = 0; j < 3; ++j)
        if (wprof[tid][j]) atomicAdd(&a.prof[tid * 3 + j], wprof[tid][j]);
#if KML_STAMPS
  if (tid == 0)
    for (int i = 0; i < 8; ++i) atomicAdd(&kml_reg_stamps[i], rs_acc[i]);
#endif
}

template <int T, int RV, int RC, int DV, int DC, bool SYN, int DMB, bool EXACT, bool PROF = false>
hipError_t launch_reg_one(const DevCode &c, const BpLaunch &a, hipStream_t s, int fast_allowed) {
  auto kern = bp_regular_kernel<T, RV, RC, DV, DC, SYN, DMB, EXACT, PROF>;
  return launch_persistent(kern, T, reg_lds_bytes(c.E, c.N, c.K, DMB), 1, kNoGridCap, PROF, a, s, c, a, a.queue,
                           fast_allowed);
}

// FAST kernel, then the exact kernel over its defer list; with FAST division
// off, the exact kernel over the batch.
template <int T, int RV, int RC, int DV, int DC, bool SYN, int DMB, bool PROF = false>
hipError_t launch_reg_t(const DevCode &c, const BpLaunch &a, hipStream_t s, int fast_allowed) {
  const size_t lds = reg_lds_bytes(c.E, c.N, c.K, DMB);
  if (lds > kLdsLimit || c.K > 65536 || c.N > 65536 || c.Kw > kRegMaxKw) return hipErrorNotSupported;
  if (!(fast_allowed & 1)) return launch_reg_one<T, RV, RC, DV, DC, SYN, DMB, true, PROF>(c, a, s, 0);
  return launch_fast_then_exact(
      a, s,
      [&](const BpLaunch &b) { return launch_reg_one<T, RV, RC, DV, DC, SYN, DMB, false, PROF>(c, b, s, fast_allowed); },
      [&](const BpLaunch &b) { return launch_reg_one<T, RV, RC, DV, DC, SYN, DMB, true, PROF>(c, b, s, 0); });
}

}  // namespace

int bp_regular_threads(int N, int M, int E, int dv_max, int dc_max, int regular) {
  if (!regular || (size_t)E * 16 + kRedBytes + (size_t)N > kLdsLimit) return 0;
  // PEG2304-class: dv 3, dc 6, N = 3*768, 2M = 3*768
  if (dv_max == 3 && dc_max == 6 && N == 3 * 768 && 2 * M == 3 * 768) return 768;
  return 0;
}

hipError_t launch_bp_regular(const DevCode &c, const BpLaunch &a, hipStream_t s) {
  if (!c.reg_c2v || bp_regular_threads(c.N, c.M, c.E, c.dv_max, c.dc_max, c.regular) != 768)
    return hipErrorNotSupported;
  const int fast = bp_fast_mode(c);
  if (a.cw_prof || a.prof) {  // the iteration profile: its own instances (SYN = false), or an error
    if (hipError_t e = prof_launch_check(a)) return e;
    if (a.sym_y) {
      if (!bp_regular_fuses_demap(c, a.sym_bits) || a.cw_idx || a.p0_sel) return hipErrorNotSupported;
      return launch_reg_t<768, 3, 3, 3, 6, false, 2, true>(c, a, s, fast);
    }
    return launch_reg_t<768, 3, 3, 3, 6, false, 0, true>(c, a, s, fast);
  }
  if (a.sym_y) {
    if (!bp_regular_fuses_demap(c, a.sym_bits) || a.cw_idx || a.p0_sel) return hipErrorNotSupported;
    return a.syn ? launch_reg_t<768, 3, 3, 3, 6, true, 2>(c, a, s, fast)
                 : launch_reg_t<768, 3, 3, 3, 6, false, 2>(c, a, s, fast);
  }
  return a.syn ? launch_reg_t<768, 3, 3, 3, 6, true, 0>(c, a, s, fast)
               : launch_reg_t<768, 3, 3, 3, 6, false, 0>(c, a, s, fast);
}

#if KML_STAMPS
}  // namespace kml
extern "C" int kml_debug_reg_stamps(unsigned long long *out, int reset) {
  hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(kml::kml_reg_stamps), sizeof(kml::kml_reg_stamps));
  if (e == hipSuccess)  // then the per-wave phase sums (16 x 4)
    e = hipMemcpyFromSymbol(out + 8, HIP_SYMBOL(kml::kml_reg_wave_stamps), sizeof(kml::kml_reg_wave_stamps));
  if (reset) {
    unsigned long long zero[8 + 64] = {};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(kml::kml_reg_stamps), zero, sizeof(kml::kml_reg_stamps));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(kml::kml_reg_wave_stamps), zero, sizeof(kml::kml_reg_wave_stamps));
  }
  return e == hipSuccess ? 0 : -3;
}
namespace kml {
#endif

bool bp_regular_fuses_demap(const DevCode &c, int bits) {
  if (const char *e = getenv("KML_FUSED_DEMAP"))
    if (e[0] == '0') return false;
  return c.reg_c2v && bp_regular_threads(c.N, c.M, c.E, c.dv_max, c.dc_max, c.regular) == 768 && c.punct == 0 &&
         bits == 2 && c.cc_len % bits == 0 && reg_lds_bytes(c.E, c.N, c.K, 2) <= kLdsLimit;
}

}  // namespace kml

#if KML_DIV_STATS
KML_DIV_STATS_ACCESSOR(kml_debug_div_stats_reg)
#endif
