// demap_llr.hip — the max-log demapper of the min-sum mode's LLR front end
// (kml_demap_llr and KML_DEMAP_MAXLOG, include/kmldpc_amd.h).  A different
// demapper from the reference's: where demap.hip restates the probability-domain
// chain in fp64 (exact exponentials, proven divisions, 8 bytes of P0 per bit),
// this one writes one float LLR per bit from two minima of squared distances.
// tests/bp_llr_model.py (maxlog_llr) states the arithmetic in numpy and this
// kernel equals it bit for bit.
//
// The arithmetic contract.  Every value is IEEE binary32 with denormals kept
// (the code object's float_denorm_mode_32 is 3), no fma (-ffp-contract=off),
// each operation rounded once.  Rounded once to float on the way in: y[s] and h
// (fp64 in the interface), the context's normalised constellation points x_k
// (kml_constellation) and inv = (float)(1.0 / var), the division in fp64 on the
// host.  Per symbol s and point k:
//     gr = hr * xr_k - hi * xi_k        gi = hr * xi_k + hi * xr_k
//     er = yr - gr                      ei = yi - gi
//     d_k = er * er + ei * ei
// and for bit i of the symbol (most significant bit of the label first, as
// demap_common.hpp's demap_symbol_t: bit i of point k is (k >> (bits - 1 - i)) & 1)
//     L = (min over k with bit_i(k) = 1 of d_k  -  min over k with bit_i(k) = 0 of d_k) * inv,
// written where kml_demap writes that bit's P0: entry s * bits + i of the
// codeword.  Positive means bit 0, as log(P0 / P1) does.  The minimum of floats
// is exact, so the order of the scan is free.  No clamp and no clip: the output
// is the raw LLR (the decoder clamps what it reads).
//
// Mapping: a streaming kernel, 16 bytes in per symbol and 4 bytes out per bit.
// One symbol per thread, workgroups of 256 grid-striding over tiles of 256
// symbols; the points sit in LDS as floats and are read with uniform loads.  A
// codeword's LLRs are contiguous (cc_len = S * bits), so a tile's outputs are
// one run of 256 * bits floats: each thread parks its `bits` values in LDS and
// the workgroup stores the run with consecutive lanes on consecutive floats.
// The parking rows are kRow floats apart, kRow = 256 + ceil(32 / bits): the
// writes (one row per bit, consecutive lanes) and the reads (consecutive output
// floats: `bits` rows, 32 / bits symbols) both spread over the 32 banks.
#include <algorithm>

#include "bp_launch.hpp"
#include "kernels.hpp"

namespace kml {

namespace {

constexpr int kLlrThreads = 256;

template <int MB>
__global__ __launch_bounds__(kLlrThreads) void demap_llr_kernel(const double *__restrict__ cons,
                                                                const double2 *__restrict__ y, int S, int reps,
                                                                const double2 *__restrict__ h, int h_stride,
                                                                const int32_t *__restrict__ h_sel, float inv,
                                                                long long nsym, float *__restrict__ llr) {
  constexpr int KC = 1 << MB, T = kLlrThreads;
  constexpr int kRow = T + (32 + MB - 1) / MB;
  __shared__ float2 pts[KC];
  __shared__ float park[MB * kRow];
  const int tid = threadIdx.x;
  for (int k = tid; k < KC; k += T) pts[k] = make_float2((float)cons[2 * k], (float)cons[2 * k + 1]);
  __syncthreads();
  const float kInf = __int_as_float(0x7F800000);
  for (long long tile = (long long)blockIdx.x * T; tile < nsym; tile += (long long)gridDim.x * T) {
    const long long gid = tile + tid;
    if (gid < nsym) {
      const long long ent = gid / S;
      const int j = (int)(gid - ent * S);
      const double2 hd = h[ent * h_stride + (h_sel ? h_sel[ent] : 0)];
      const double2 yd = y[(ent / reps) * S + j];
      const float hr = (float)hd.x, hi = (float)hd.y, yr = (float)yd.x, yi = (float)yd.y;
      float m0[MB], m1[MB];
#pragma unroll
      for (int i = 0; i < MB; ++i) m0[i] = m1[i] = kInf;
#pragma unroll
      for (int k = 0; k < KC; ++k) {
        const float2 x = pts[k];
        const float gr = hr * x.x - hi * x.y;
        const float gi = hr * x.y + hi * x.x;
        const float er = yr - gr, ei = yi - gi;
        const float d = er * er + ei * ei;
#pragma unroll
        for (int i = 0; i < MB; ++i) {
          if ((k >> (MB - 1 - i)) & 1)
            m1[i] = fminf(m1[i], d);
          else
            m0[i] = fminf(m0[i], d);
        }
      }
#pragma unroll
      for (int i = 0; i < MB; ++i) park[i * kRow + tid] = (m1[i] - m0[i]) * inv;
    }
    __syncthreads();
    const long long left = nsym - tile;
    const int cnt = (int)(left < T ? left : T) * MB;  // floats of this tile
    float *out = llr + tile * MB;
    for (int q = tid; q < cnt; q += T) out[q] = park[(q % MB) * kRow + q / MB];
    __syncthreads();  // the next tile parks over these
  }
}

template <int MB>
hipError_t launch_llr(const double *cons, const double2 *y, int S, int reps, const double2 *h, int h_stride,
                      const int32_t *h_sel, float inv, long long nsym, float *llr, hipStream_t s) {
  const long long tiles = (nsym + kLlrThreads - 1) / kLlrThreads;
  const unsigned grid = (unsigned)std::min<long long>(tiles, 8LL * device_cus());
  hipLaunchKernelGGL(demap_llr_kernel<MB>, dim3(grid), dim3(kLlrThreads), 0, s, cons, y, S, reps, h, h_stride, h_sel,
                     inv, nsym, llr);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_demap_llr(int bits, const double *cons, const double2 *y, int S, int reps, const double2 *h,
                            int h_stride, const int32_t *h_sel, float inv, int n, float *llr, hipStream_t s) {
  if (n <= 0 || S <= 0) return hipSuccess;
  if (reps < 1) return hipErrorInvalidValue;
  const long long nsym = (long long)n * S;
  switch (bits) {
    case 1: return launch_llr<1>(cons, y, S, reps, h, h_stride, h_sel, inv, nsym, llr, s);
    case 2: return launch_llr<2>(cons, y, S, reps, h, h_stride, h_sel, inv, nsym, llr, s);
    case 3: return launch_llr<3>(cons, y, S, reps, h, h_stride, h_sel, inv, nsym, llr, s);
    case 4: return launch_llr<4>(cons, y, S, reps, h, h_stride, h_sel, inv, nsym, llr, s);
    case 6: return launch_llr<6>(cons, y, S, reps, h, h_stride, h_sel, inv, nsym, llr, s);
    default: return hipErrorNotSupported;
  }
}

}  // namespace kml
