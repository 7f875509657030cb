// capi_internal.hpp — what the C-ABI layer's files share: the context
// (context.cpp owns its lifetime, the profiler and run_bp), the receive path
// (receive.cpp) and the helpers the extern "C" entry points (capi.cpp) stage
// their arguments with.  Nothing here is exported from the library.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "../../include/kmldpc_amd.h"
#include "code.hpp"
#include "comm.hpp"
#include "config.hpp"
#include "kernels.hpp"
#include "layout.hpp"
#include "modem.hpp"

namespace kml_host __attribute__((visibility("hidden"))) {

// A device allocation that only grows; owned: freed with its holder.
struct DBuf {
  void *p = nullptr;
  size_t cap = 0;
  DBuf() = default;
  DBuf(const DBuf &) = delete;
  DBuf &operator=(const DBuf &) = delete;
  ~DBuf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    size_t want = std::max<size_t>(bytes, 256);
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T *as() const {
    return reinterpret_cast<T *>(p);
  }
};

struct Pending {
  std::string stage;
  hipEvent_t ev0, ev1;
  int cnt_slot;  // counter-arena slot for "bp" launches (-1 otherwise)
  double fixed_bytes;
};

struct Stat {
  int64_t launches = 0;
  double ms = 0, bytes = 0, flops = 0;
};

constexpr int kArenaSlots = 1024;

}  // namespace kml_host

struct kml_ctx {
  int device = 0;
  const char *bp_family = nullptr;  // kernel family of the last BP launch
  int precision = KML_PREC_F64;     // kml_set_precision: arithmetic of the final BP decodes
  int algorithm = KML_ALG_SPA;      // kml_set_algorithm: decoder of the final BP decodes
  float nms_alpha = 0.75f;          // ... and the min-sum normalisation factor
  int schedule = KML_SCHED_FLOODING;  // kml_set_schedule: row schedule of the min-sum decodes
  int demapper = KML_DEMAP_EXACT;   // kml_set_demapper: front end of the min-sum receive path
  int messages = KML_MSG_F32;       // kml_set_messages: message format of the layered min-sum decodes
  float nms_offset = 0.0f;          // kml_set_nms_offset: the min-sum offset correction (0: none)
  kml::LayeredPlan layered;         // its layers (empty: the code has none, kml_code_layers says KML_E_UNSUP)
  kml::LnmsPlanDev lnms_dev;        // ... and the device copy of the passes (d_lnms)
  kml::LnmsItemsDev lnms_items;     // ... and of the global-table instances' items (d_lnms_items)
  bool lnms_only = false;           // the code's only min-sum decoders are the layered ones (kernels.hpp bp_lnms_only_supported)
  hipStream_t stream = nullptr;
  hipStream_t cstream = nullptr;  // host-buffer frame uploads (kml_decode_frames' chunked path), made on first use
  kml::RunConfig rc;
  kml::LdpcCode code;
  kml::Modem modem;
  kml::DevCode dc{};
  double rot[8];
  using DBuf = kml_host::DBuf;
  // resident constants
  DBuf d_graph, d_cons, d_lnms, d_lnms_items;
  // algorithmic fp64 flops per executed VN / CN phase ("Roofline")
  double vn_flops = 0, cn_flops = 0;
  DBuf d_arena;  // kArenaSlots x CNT_N counters
  int arena_next = 0;
  DBuf d_queue, d_gslots, d_gsync, d_gcch;
  long long gslots_cap = 0;
  int coop_groups = 0;      // cooperative BP groups (0: kernel not used)
  bool coop_pending = false;  // a cooperative launch whose abort word is unchecked
  bool coop_this_call = false;  // the current API call made a cooperative launch (fail() settles it)
  bool coop_inherited = false;  // ... on top of an earlier call's unchecked launch (the abort word is shared)
  int inject_abort = -1;      // test hook (kml_debug_inject_abort): raise the abort after the n-th coop launch
  bool inject_fail = false;   // test hook (kml_debug_inject_abort(-2)): ... and fail that call before its sync
  kml::RcclComm *comm = nullptr;  // counter all-reduce over the ranks (kml_comm_init)
  DBuf w_comm;
  DBuf w_defer;  // BP launches: codewords the FAST kernel leaves to the exact kernel (+ count)
  DBuf w_ddefer;  // demap / candidate-metric launches: the same for symbols or codewords
  // workspaces
  DBuf w_y, w_h, w_h4, w_hhat, w_p0, w_uu, w_uh, w_uh4, w_ret, w_cch, w_syn, w_sel, w_met, w_pc, w_km, w_cwerr;
  DBuf w_prof, w_cwprof;  // kml_sim_decode_profile: prof[P][3], cw_prof[B][P]
  DBuf w_llr, w_post;     // the LLR front end: float priors (demap_llr's output), posteriors
  // soft syndrome metric: candidate / final syndromes, iteration counts, sums, decode lists
  DBuf s_synm, s_synf, s_itm, s_itf, s_Lm, s_Lf, s_list;
  // Sum of log(syndrom_soft) of the most recent decode that ran a CN phase on
  // this context (the reference codec's stale member array, reduced to what
  // the metric reads); -inf = the never-written (zero) array.
  double soft_state = -INFINITY;
  // resident simulation frames
  DBuf s_uu, s_cc, s_y, s_h;
  DBuf w_hc;  // caller candidates (kml_decode_candidates)
  int sim_B = 0;
  uint64_t sim_first = 0;
  // profiling
  bool prof = false;
  std::vector<kml_host::Pending> pend;
  std::map<std::string, kml_host::Stat> stats;
  std::string err;
};

namespace kml_host __attribute__((visibility("hidden"))) {

// ---- context.cpp
int fail(kml_ctx *c, int code, const std::string &msg);
int hip_fail(kml_ctx *c, hipError_t e, const char *what);
// Every entry point that takes a context starts here: a new API call, so the
// cooperative launches fail() settles are only this call's.
inline void call_begin(kml_ctx *c) {
  if (c) c->coop_this_call = false;
}
// Opens an entry point that uses the GPU: a new API call, the entry point's
// own argument check (its result and its message; no message = a bare
// KML_E_ARG), a context that has a GPU, and that GPU current.
int gpu_begin(kml_ctx *c, bool args_ok = true, const char *bad_args = nullptr);
// The schedule rule of a layered-only code (kml_ctx::lnms_only): in the
// min-sum mode under the flooding schedule there is no kernel to decode with,
// so every decode entry point asks here before it stages or launches anything.
// KML_OK, or KML_E_UNSUP with the message set; the context keeps its state.
int schedule_refusal(kml_ctx *c, const char *who);
int finish_create(kml_ctx *c);
void destroy(kml_ctx *c);
void drain_profile(kml_ctx *c);
int sync(kml_ctx *c);

#define HIPCHK(ctx, expr, what)                                      \
  do {                                                               \
    hipError_t _e = (expr);                                          \
    if (_e != hipSuccess) return kml_host::hip_fail(ctx, _e, what);  \
  } while (0)

#define TRY(x)                   \
  do {                           \
    int _r = (x);                \
    if (_r != KML_OK) return _r; \
  } while (0)

// One stage's profile record around the launches between construction and
// stop().  Events that are never handed on (an early return) are destroyed.
struct Timer {
  kml_ctx *c;
  Pending p;
  bool on;
  Timer(kml_ctx *ctx, const char *stage, int slot, double bytes) : c(ctx), on(ctx->prof) {
    if (!on) return;
    p.stage = stage;
    p.cnt_slot = slot;
    p.fixed_bytes = bytes;
    hipEventCreate(&p.ev0);
    hipEventCreate(&p.ev1);
    hipEventRecord(p.ev0, c->stream);
  }
  Timer(const Timer &) = delete;
  void stop() {
    if (!on) return;
    hipEventRecord(p.ev1, c->stream);
    c->pend.push_back(p);
    on = false;  // drain_profile owns the events now
  }
  ~Timer() {
    if (!on) return;
    hipEventDestroy(p.ev0);
    hipEventDestroy(p.ev1);
  }
};

inline unsigned long long *slot_ptr(kml_ctx *c, int s) {
  return c->d_arena.as<unsigned long long>() + (size_t)s * kml::CNT_N;
}
// The next counter slot of the arena, zeroed on the stream.
int fresh_slot(kml_ctx *c, int &slot);
// The tail of a counting call: the counter words at `cnt`, then each of `more`
// (a NULL dst is skipped), come back on the stream; one sync; then
// counters[0..n) (may be NULL) are set to the words, or grow by them (add).
struct D2H {
  void *dst;
  const void *src;
  size_t bytes;
};
int read_back(kml_ctx *c, const unsigned long long *cnt, uint64_t *counters, int n, bool add = false,
              std::initializer_list<D2H> more = {});

// Launch BP over n entries with a fresh counter slot (*slot_out, when asked
// for); reuse >= 0 accumulates into that (already zeroed) slot.
// metric = true: a candidate-metric decode of the blind front end, which stays
// fp64 sum-product in every mode (kml_set_precision and kml_set_algorithm
// change the final decodes only).
// llr: decode from float priors (kernels.hpp LlrIoDev) with the context's
// min-sum decoder, whose mode the context must be in; a.p0 is not read and
// a.p0_stride / a.p0_sel_stride count floats.  The max-log front end's
// candidate-metric decodes come this way too (metric stays false).
int run_bp(kml_ctx *c, kml::BpLaunch a, int *slot_out = nullptr, int reuse = -1, bool metric = false,
           const kml::LlrIoDev *llr = nullptr);
// The FAST demappers' defer list (kernels.hpp DemapDefer): at least `need`
// entries (the candidate metric defers whole codewords: need = B).
int demap_defer(kml_ctx *c, int need, kml::DemapDefer &d);
// launch_demap as one profiled "demap" stage (arguments as launch_demap's).
int run_demap(kml_ctx *c, const double2 *y, int reps, const double2 *h, int h_stride, const int32_t *h_sel, double var,
              int n, double *p0);
// launch_demap_llr as one profiled "demap" stage (arguments as run_demap's, float LLRs out).
int run_demap_llr(kml_ctx *c, const double2 *y, int reps, const double2 *h, int h_stride, const int32_t *h_sel,
                  double var, int n, float *llr);
// launch_kmeans as one profiled "kmeans" stage; its workspace is the context's.
int run_kmeans(kml_ctx *c, const double2 *y, int iters, int B, double2 *h_hat, double2 *h4, double2 *hat_out = nullptr);

// p stays the caller's buffer, or becomes `ws` grown to n elements when the caller gave none.
template <class T>
int or_workspace(kml_ctx *c, T *&p, DBuf &ws, size_t n) {
  if (p) return KML_OK;
  HIPCHK(c, ws.ensure(n * sizeof(T)), "hipMalloc(workspace)");
  p = ws.as<T>();
  return KML_OK;
}

// Stage a host or device input; returns a device pointer.
template <class T>
int stage_in(kml_ctx *c, DBuf &buf, const T *src, size_t n, int flags, const T *&dev) {
  if (flags & KML_DEVICE_PTRS) {
    dev = src;
    return KML_OK;
  }
  HIPCHK(c, buf.ensure(n * sizeof(T)), "hipMalloc(workspace)");
  if (n) HIPCHK(c, hipMemcpyAsync(buf.p, src, n * sizeof(T), hipMemcpyHostToDevice, c->stream), "H2D");
  dev = buf.as<T>();
  return KML_OK;
}

// One optional output of an entry point: where the kernels write it (dev: the
// caller's own device pointer under KML_DEVICE_PTRS, a workspace for a host
// pointer, NULL when the caller passed NULL) and, for a host pointer, what
// copy_out / zero_out bring back.
template <class T>
struct Out {
  T *dev = nullptr;
  T *host = nullptr;  // set only when the output is staged through a workspace
  size_t n = 0;
};
template <class T>
int stage_out(kml_ctx *c, DBuf &buf, T *dst, size_t n, int flags, Out<T> &o) {
  if (!dst) return KML_OK;
  if (flags & KML_DEVICE_PTRS) {
    o.dev = dst;
    return KML_OK;
  }
  HIPCHK(c, buf.ensure(n * sizeof(T)), "hipMalloc(workspace)");
  o.dev = buf.as<T>();
  o.host = dst;
  o.n = n;
  return KML_OK;
}
template <class T>
int copy_out(kml_ctx *c, const Out<T> &o) {
  if (!o.host || o.n == 0) return KML_OK;
  HIPCHK(c, hipMemcpyAsync(o.host, o.dev, o.n * sizeof(T), hipMemcpyDeviceToHost, c->stream), "D2H");
  return KML_OK;
}
// An output this call does not compute: zeros for a host caller; a device
// caller's memory stays untouched (the KML_DEVICE_PTRS contract).
template <class T>
void zero_out(const Out<T> &o) {
  if (o.host) memset(o.host, 0, o.n * sizeof(T));
}

// ---- receive.cpp
// Receive path shared by kml_decode_frames, kml_sim_decode and
// kml_sim_histogram.  All pointers are device pointers.
struct RecvIO {
  const double2 *y = nullptr;
  const double2 *true_h = nullptr;  // known channel (simulator.cc:132-133); NULL = blind
  const double2 *cand = nullptr;    // caller's candidates [B][ncand] (KmCodec::Decoder h_hats), ncand > 1
  int ncand = 0;
  uint8_t *uh = nullptr;            // uu_hat[B][K] (NULL: not kept)
  int32_t *chosen = nullptr;        // [B]
  double *met = nullptr;            // [B][4]
  int32_t *ret = nullptr;           // [B]
  double2 *hhat = nullptr;          // [B] k-means h_hat
  const uint64_t *ref_bits = nullptr;  // packed source bits for CntErr
  int32_t *cw_err = nullptr;           // [B] error bits per codeword
  // iteration profile of the final decode (kml_sim_decode_profile; kernels.hpp BpLaunch::cw_prof / prof)
  int32_t *cw_prof = nullptr;          // [B][max_iter]
  unsigned long long *prof = nullptr;  // [max_iter][3]
  // GetHistogramData instead of Decoder (simulator.cc:154-162): candidate
  // metrics only, no final decode; CntErr then sees the uu_hat left by the last
  // candidate's metric decode (5G metric), or all zeros for the hard PEG metric
  // (the reference's uu_hat buffer is uninitialised there).
  bool histogram = false;
  // soft metric stale-state rule: in the simulator (sim) the reference's codec
  // is copied per task of thread_block_number codewords, so the state restarts
  // at global indices that are multiples of it (and at the batch start);
  // kml_decode_frames carries it across calls like one KmCodec instance.
  bool sim = false;
  uint64_t first_cw = 0;
};
int receive(kml_ctx *c, const RecvIO &io, double snr, int B, int &bp_slot);
int decode_frames_chunked(kml_ctx *c, const double *y, const double *true_h, double snr, int B, uint8_t *uu_hat,
                          int32_t *chosen, double *metrics, int32_t *ret, double *h_hat, int CH);

}  // namespace kml_host
