// capi.cpp — the extern "C" entry points of include/kmldpc_amd.h: argument
// checks, staging of the caller's host or device buffers, and the calls into
// the context (context.cpp) and the receive path (receive.cpp).
#include "capi_internal.hpp"

namespace kml {
int ref_frames(const LdpcCode &code, const Modem &modem, int64_t *state, double snr, int n, uint8_t *uu_out,
               double *h_out, double *y_out);
}

using namespace kml_host;

namespace {

// context-free calls (kml_comm_unique_id) report through this thread's message
thread_local std::string g_free_err = "null context";

// Codewords per chunk of the host-buffer known-channel path (KML_HOST_CHUNK;
// 0 = one piece).
int host_chunk() {
  if (const char *e = getenv("KML_HOST_CHUNK")) return atoi(e);
  return 8192;
}

// Does RN16(a) give +0 for this a > 0?  (Half of binary16's smallest denormal, 2^-25, ties to even: zero.)
bool half_rounds_to_zero(float a) { return a <= 0x1p-25f; }

const double2 *as_c(const double *p) { return reinterpret_cast<const double2 *>(p); }
double2 *as_c(double *p) { return reinterpret_cast<double2 *>(p); }

// The outputs kml_decode_frames and kml_decode_candidates share, staged and
// handed to the receive path.
struct DecodeOuts {
  Out<uint8_t> uh;
  Out<int32_t> chosen, ret;
  Out<double> met;
};
int stage_decode_outs(kml_ctx *c, int B, uint8_t *uu_hat, int32_t *chosen, double *metrics, int32_t *ret, int flags,
                      DecodeOuts &o, RecvIO &io) {
  TRY(stage_out(c, c->w_uh, uu_hat, (size_t)B * c->code.K, flags, o.uh));
  TRY(stage_out(c, c->w_sel, chosen, (size_t)B, flags, o.chosen));
  TRY(stage_out(c, c->w_met, metrics, (size_t)B * 4, flags, o.met));
  TRY(stage_out(c, c->w_ret, ret, (size_t)B, flags, o.ret));
  io.uh = o.uh.dev;
  io.chosen = o.chosen.dev;
  io.met = o.met.dev;
  io.ret = o.ret.dev;
  io.histogram = (flags & KML_HISTOGRAM) != 0;
  return KML_OK;
}
// ... and their common end: histogram mode runs no final decode, so there is
// no BP return value.
int finish_decode(kml_ctx *c, const DecodeOuts &o, bool histogram) {
  TRY(copy_out(c, o.uh));
  if (histogram)
    zero_out(o.ret);
  else
    TRY(copy_out(c, o.ret));
  return sync(c);
}

int comm_allreduce(kml_ctx *c, void *vals, int n, bool f64) {
  call_begin(c);
  if (!c || (!vals && n > 0) || n < 0) return fail(c, KML_E_ARG, "kml_comm_allreduce: bad argument");
  if (!c->comm) return fail(c, KML_E_ARG, "kml_comm_allreduce: no communicator (kml_comm_init)");
  if (n == 0) return KML_OK;
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  const size_t bytes = (size_t)n * 8;
  HIPCHK(c, c->w_comm.ensure(bytes), "hipMalloc(comm)");
  HIPCHK(c, hipMemcpyAsync(c->w_comm.p, vals, bytes, hipMemcpyHostToDevice, c->stream), "H2D");
  std::string err;
  if (kml::rccl_allreduce(c->comm, c->w_comm.p, (size_t)n, f64, c->stream, err) != 0) return fail(c, KML_E_HIP, err);
  HIPCHK(c, hipMemcpyAsync(vals, c->w_comm.p, bytes, hipMemcpyDeviceToHost, c->stream), "D2H");
  HIPCHK(c, hipStreamSynchronize(c->stream), "hipStreamSynchronize");
  return KML_OK;
}

// Receive the resident batch (kml_sim_decode*): CntErr against its source bits.
int sim_receive(kml_ctx *c, double snr, int blind, bool histogram, int &slot, int32_t *cw_prof = nullptr,
                unsigned long long *prof = nullptr) {
  RecvIO io;
  io.cw_prof = cw_prof;
  io.prof = prof;
  io.y = c->s_y.as<double2>();
  io.true_h = blind ? nullptr : c->s_h.as<double2>();
  io.ref_bits = c->s_uu.as<uint64_t>();
  TRY(or_workspace(c, io.cw_err, c->w_cwerr, (size_t)c->sim_B));
  io.histogram = histogram;
  io.sim = true;
  io.first_cw = c->sim_first;
  if (histogram) TRY(or_workspace(c, io.met, c->w_met, 4 * (size_t)c->sim_B));
  return receive(c, io, snr, c->sim_B, slot);
}

// kml_*_probe: n_in doubles per entry in, n_out doubles per entry out.
int run_probe(kml_ctx *c, const double *in, int n, double *out, int n_in, int n_out,
              hipError_t (*launch)(const double *, int, double *, hipStream_t)) {
  TRY(gpu_begin(c, in && out && n >= 0));
  const double *d_in;
  TRY(stage_in(c, c->w_y, in, (size_t)n * n_in, 0, d_in));
  Out<double> o;
  TRY(stage_out(c, c->w_p0, out, (size_t)n * n_out, 0, o));
  HIPCHK(c, launch(d_in, n, o.dev, c->stream), "probe");
  TRY(copy_out(c, o));
  return sync(c);
}

// The profile's entry points: the pending launches are read first.
kml_host::Stat drained_stat(kml_ctx *c, const char *stage) {
  call_begin(c);
  if (c->device >= 0) hipSetDevice(c->device);
  drain_profile(c);
  auto it = c->stats.find(stage);
  return it != c->stats.end() ? it->second : Stat();
}

}  // namespace

extern "C" {

int kml_abi_version(void) { return KML_ABI_VERSION; }

int kml_create(const char *config_toml, const char *data_dir, int device, kml_ctx **out) {
  if (!out || !config_toml) return KML_E_ARG;
  *out = nullptr;
  kml_ctx *c = new kml_ctx();
  c->device = device;
  std::string err;
  if (!kml::load_run_config(config_toml, data_dir ? data_dir : "", c->rc, err)) {
    c->err = err;
    *out = c;  // keep the context so kml_last_error can report
    return KML_E_IO;
  }
  *out = c;
  return finish_create(c);
}

int kml_create_explicit(const char *matrix_file, const char *modem_file, int is5g, int active, int max_iter,
                        int metric_soft, int metric_iter, int device, kml_ctx **out) {
  if (!out || !matrix_file || !modem_file) return KML_E_ARG;
  kml_ctx *c = new kml_ctx();
  c->device = device;
  c->rc.matrix_file = matrix_file;
  c->rc.modem_file = modem_file;
  c->rc.is5g = is5g != 0;
  c->rc.active = active != 0;
  c->rc.max_iter = max_iter;
  c->rc.metric_soft = metric_soft != 0;
  c->rc.metric_iter = metric_iter;
  *out = c;
  return finish_create(c);
}

void kml_destroy(kml_ctx *c) {
  if (c) destroy(c);
}

const char *kml_last_error(const kml_ctx *c) { return c ? c->err.c_str() : g_free_err.c_str(); }

const char *kml_bp_kernel(const kml_ctx *c) { return c && c->bp_family ? c->bp_family : ""; }

int kml_set_precision(kml_ctx *c, int prec) {
  if (!c) return KML_E_ARG;
  call_begin(c);
  if (prec != KML_PREC_F64 && prec != KML_PREC_F32)
    return fail(c, KML_E_ARG, "kml_set_precision: unknown precision " + std::to_string(prec));
  if (prec == KML_PREC_F32) {
    if (c->device < 0 || !c->stream)
      return fail(c, KML_E_UNSUP, "kml_set_precision: a host-only context (device < 0) has no f32 decoder");
    if (!kml::bp_regular_f32_supported(c->dc))
      return fail(c, KML_E_UNSUP,
                  "kml_set_precision: the f32 decoder takes only PEG2304-class codes (regular, dv 3, dc 6, N = 2304, "
                  "M = 1152); the context stays in fp64");
  }
  c->precision = prec;
  return KML_OK;
}

int kml_get_precision(const kml_ctx *c) { return c ? c->precision : KML_E_ARG; }

int kml_set_algorithm(kml_ctx *c, int alg, double alpha) {
  if (!c) return KML_E_ARG;
  call_begin(c);
  if (alg != KML_ALG_SPA && alg != KML_ALG_NMS)
    return fail(c, KML_E_ARG, "kml_set_algorithm: unknown algorithm " + std::to_string(alg));
  if (alg == KML_ALG_SPA) {  // always accepted, alpha ignored; the schedule belongs to the min-sum mode
    c->algorithm = alg;
    c->schedule = KML_SCHED_FLOODING;
    c->demapper = KML_DEMAP_EXACT;  // ... and so does the max-log front end
    c->messages = KML_MSG_F32;      // ... and the binary16 message format
    c->nms_offset = 0.0f;           // ... and the offset correction
    return KML_OK;
  }
  if (alpha == 0.0) alpha = 0.75;
  if (!(alpha > 0.0 && alpha <= 1.0))  // NaN included
    return fail(c, KML_E_ARG, "kml_set_algorithm: alpha must be 0 (the default 0.75) or in (0, 1]");
  const float af = (float)alpha;
  if (!(af > 0.0f))
    return fail(c, KML_E_ARG, "kml_set_algorithm: alpha rounds to zero in single precision");
  if (c->messages == KML_MSG_F16 && half_rounds_to_zero(af))
    return fail(c, KML_E_ARG,
                "kml_set_algorithm: alpha rounds to zero in binary16 (KML_MSG_F16); the context keeps its algorithm");
  if (c->device < 0 || !c->stream)
    return fail(c, KML_E_UNSUP, "kml_set_algorithm: a host-only context (device < 0) has no min-sum decoder");
  if (c->precision != KML_PREC_F64)
    return fail(c, KML_E_UNSUP, "kml_set_algorithm: the min-sum decoder is not available in the f32 precision");
  if (kml::bp_generic_forced())
    return fail(c, KML_E_UNSUP, "kml_set_algorithm: the min-sum decoder is not available with KML_BP_KERNEL=generic");
  if (!kml::bp_irregular_nms_supported(c->dc) && !c->lnms_only)
    return fail(c, KML_E_UNSUP,
                "kml_set_algorithm: the min-sum decoder takes only the codes of bp_irregular_kernel (column degrees "
                "<= 9, row degrees in [2, 10], messages in LDS) and, in the layered schedule only, irregular codes of "
                "those degrees with E, M <= 65535, N < 65535 whose posteriors and messages (4 N + 4 E bytes) fit one "
                "CU's LDS; the context keeps its algorithm");
  c->algorithm = alg;
  c->nms_alpha = af;
  return KML_OK;
}

int kml_get_algorithm(const kml_ctx *c, double *alpha) {
  if (!c) return KML_E_ARG;
  if (alpha) *alpha = (double)c->nms_alpha;
  return c->algorithm;
}

int kml_set_schedule(kml_ctx *c, int sched) {
  if (!c) return KML_E_ARG;
  call_begin(c);
  if (sched != KML_SCHED_FLOODING && sched != KML_SCHED_LAYERED)
    return fail(c, KML_E_ARG, "kml_set_schedule: unknown schedule " + std::to_string(sched));
  if (sched == KML_SCHED_FLOODING) {  // always accepted; the binary16 format belongs to the layered schedule
    c->schedule = sched;
    c->messages = KML_MSG_F32;
    return KML_OK;
  }
  if (c->device < 0 || !c->stream)
    return fail(c, KML_E_UNSUP, "kml_set_schedule: a host-only context (device < 0) has no min-sum decoder");
  if (kml::bp_generic_forced())
    return fail(c, KML_E_UNSUP, "kml_set_schedule: the layered schedule is not available with KML_BP_KERNEL=generic");
  if (c->algorithm != KML_ALG_NMS)
    return fail(c, KML_E_UNSUP,
                "kml_set_schedule: the layered schedule belongs to the min-sum mode (kml_set_algorithm(KML_ALG_NMS) "
                "first); the context keeps its schedule");
  if (!c->lnms_dev.pass)  // (never in the min-sum mode: the plan is made for every code that mode accepts)
    return fail(c, KML_E_UNSUP, "kml_set_schedule: the code has no layer plan");
  c->schedule = sched;
  return KML_OK;
}

int kml_get_schedule(const kml_ctx *c) { return c ? c->schedule : KML_E_ARG; }

int kml_code_layers(const kml_ctx *c, int32_t *layer_ptr, int cap) {
  if (!c || cap < 0 || (cap > 0 && !layer_ptr)) return KML_E_ARG;
  const std::vector<int32_t> &lp = c->layered.layer_ptr;
  if (lp.empty()) return KML_E_UNSUP;
  const int n = std::min<int>(cap, (int)lp.size());
  for (int i = 0; i < n; i++) layer_ptr[i] = lp[i];
  return (int)lp.size() - 1;
}

int kml_set_demapper(kml_ctx *c, int demapper) {
  if (!c) return KML_E_ARG;
  call_begin(c);
  if (demapper != KML_DEMAP_EXACT && demapper != KML_DEMAP_MAXLOG)
    return fail(c, KML_E_ARG, "kml_set_demapper: unknown demapper " + std::to_string(demapper));
  if (demapper == KML_DEMAP_EXACT) {  // always accepted
    c->demapper = demapper;
    return KML_OK;
  }
  if (c->device < 0 || !c->stream)
    return fail(c, KML_E_UNSUP, "kml_set_demapper: a host-only context (device < 0) has no min-sum decoder");
  if (kml::bp_generic_forced())
    return fail(c, KML_E_UNSUP, "kml_set_demapper: the max-log front end is not available with KML_BP_KERNEL=generic");
  if (c->algorithm != KML_ALG_NMS)
    return fail(c, KML_E_UNSUP,
                "kml_set_demapper: the max-log front end belongs to the min-sum mode (kml_set_algorithm(KML_ALG_NMS) "
                "first); the context keeps its demapper");
  c->demapper = demapper;
  return KML_OK;
}

int kml_get_demapper(const kml_ctx *c) { return c ? c->demapper : KML_E_ARG; }

int kml_set_messages(kml_ctx *c, int fmt) {
  if (!c) return KML_E_ARG;
  call_begin(c);
  if (fmt != KML_MSG_F32 && fmt != KML_MSG_F16)
    return fail(c, KML_E_ARG, "kml_set_messages: unknown message format " + std::to_string(fmt));
  if (fmt == KML_MSG_F32) {  // always accepted
    c->messages = fmt;
    return KML_OK;
  }
  if (c->device < 0 || !c->stream)
    return fail(c, KML_E_UNSUP, "kml_set_messages: a host-only context (device < 0) has no min-sum decoder");
  if (kml::bp_generic_forced())
    return fail(c, KML_E_UNSUP, "kml_set_messages: the binary16 format is not available with KML_BP_KERNEL=generic");
  if (c->algorithm != KML_ALG_NMS || c->schedule != KML_SCHED_LAYERED)
    return fail(c, KML_E_UNSUP,
                "kml_set_messages: the binary16 format belongs to the layered min-sum decoder "
                "(kml_set_algorithm(KML_ALG_NMS) and kml_set_schedule(KML_SCHED_LAYERED) first; the flooding schedule "
                "has no binary16 kernel); the context keeps its format");
  if (half_rounds_to_zero(c->nms_alpha))
    return fail(c, KML_E_ARG, "kml_set_messages: the context's alpha rounds to zero in binary16");
  if (c->nms_offset > 0.0f && half_rounds_to_zero(c->nms_offset))
    return fail(c, KML_E_ARG, "kml_set_messages: the context's min-sum offset rounds to zero in binary16");
  c->messages = fmt;
  return KML_OK;
}

int kml_get_messages(const kml_ctx *c) { return c ? c->messages : KML_E_ARG; }

int kml_set_nms_offset(kml_ctx *c, double beta) {
  if (!c) return KML_E_ARG;
  call_begin(c);
  if (!(beta >= 0.0 && beta <= 256.0))  // NaN included
    return fail(c, KML_E_ARG, "kml_set_nms_offset: beta must be in [0, 256]");
  if (beta == 0.0) {  // always accepted: the decoders without the correction
    c->nms_offset = 0.0f;
    return KML_OK;
  }
  const float bf = (float)beta;
  if (!(bf > 0.0f)) return fail(c, KML_E_ARG, "kml_set_nms_offset: beta rounds to zero in single precision");
  if (c->messages == KML_MSG_F16 && half_rounds_to_zero(bf))
    return fail(c, KML_E_ARG,
                "kml_set_nms_offset: beta rounds to zero in binary16 (KML_MSG_F16); the context keeps its offset");
  if (c->device < 0 || !c->stream)
    return fail(c, KML_E_UNSUP, "kml_set_nms_offset: a host-only context (device < 0) has no min-sum decoder");
  if (kml::bp_generic_forced())
    return fail(c, KML_E_UNSUP, "kml_set_nms_offset: the offset correction is not available with KML_BP_KERNEL=generic");
  if (c->algorithm != KML_ALG_NMS)
    return fail(c, KML_E_UNSUP,
                "kml_set_nms_offset: the offset correction belongs to the min-sum mode (kml_set_algorithm(KML_ALG_NMS) "
                "first); the context keeps its offset");
  c->nms_offset = bf;
  return KML_OK;
}

int kml_get_nms_offset(const kml_ctx *c, double *beta) {
  if (!c || !beta) return KML_E_ARG;
  *beta = (double)c->nms_offset;
  return KML_OK;
}

int kml_dims(const kml_ctx *c, int32_t *d) {
  if (!c || !d) return KML_E_ARG;
  const kml::LdpcCode &L = c->code;
  d[KML_DIM_M] = L.M;
  d[KML_DIM_NCOL] = L.N;
  d[KML_DIM_K] = L.K;
  d[KML_DIM_CCLEN] = L.cc_len;
  d[KML_DIM_Z] = L.Z;
  d[KML_DIM_E] = L.E;
  d[KML_DIM_CHK] = L.chk;
  d[KML_DIM_MAXITER] = c->rc.max_iter;
  d[KML_DIM_BITS] = c->modem.bits;
  d[KML_DIM_KC] = c->modem.Kc;
  d[KML_DIM_S] = c->modem.bits ? L.cc_len / c->modem.bits : 0;
  kml::DevCode tmp{};
  tmp.E = L.E;
  tmp.N = L.N;
  d[KML_DIM_BP_LDS] = kml::bp_uses_lds(tmp) ? 1 : 0;
  d[KML_DIM_PART_G] = c->dc.pt_G;
  return KML_OK;
}

int kml_code_perm(const kml_ctx *c, int32_t *perm) {
  if (!c || !perm) return KML_E_ARG;
  memcpy(perm, c->code.perm.data(), sizeof(int32_t) * c->code.perm.size());
  return KML_OK;
}

int kml_code_graph(const kml_ctx *c, int32_t *rp, int32_t *rc, int32_t *cp, int32_t *cs) {
  if (!c) return KML_E_ARG;
  const kml::LdpcCode &L = c->code;
  if (rp) memcpy(rp, L.row_ptr.data(), 4 * L.row_ptr.size());
  if (rc) memcpy(rc, L.row_col.data(), 4 * L.row_col.size());
  if (cp) memcpy(cp, L.col_ptr.data(), 4 * L.col_ptr.size());
  if (cs) memcpy(cs, L.col_slot.data(), 4 * L.col_slot.size());
  return KML_OK;
}

int kml_constellation(const kml_ctx *c, double *pts) {
  if (!c || !pts) return KML_E_ARG;
  memcpy(pts, c->modem.pts.data(), sizeof(double) * c->modem.pts.size());
  return KML_OK;
}

int kml_encode(const kml_ctx *c, const uint8_t *uu, uint8_t *cc, int B) {
  if (!c || !uu || !cc || B < 0) return KML_E_ARG;
  for (int b = 0; b < B; b++) c->code.encode(uu + (size_t)b * c->code.K, cc + (size_t)b * c->code.cc_len);
  return KML_OK;
}

int kml_bp_decode(kml_ctx *c, const double *p0, int B, int iter_count, uint8_t *uu_hat, int32_t *ret, uint8_t *cc_hat,
                  double *syn, int flags) {
  const bool ok = c && p0 && B >= 0 && iter_count >= 0;
  if (ok && B == 0) return KML_OK;
  TRY(gpu_begin(c, ok, "kml_bp_decode: bad argument"));
  TRY(schedule_refusal(c, "kml_bp_decode"));
  if (syn && c->algorithm == KML_ALG_NMS)
    return fail(c, KML_E_UNSUP, "kml_bp_decode: the min-sum decoder (KML_ALG_NMS) has no syndrom_soft: syn must be NULL");
  const kml::LdpcCode &L = c->code;
  const double *d_p0;
  TRY(stage_in(c, c->w_p0, p0, (size_t)B * L.cc_len, flags, d_p0));
  Out<uint8_t> uh, cch;
  Out<int32_t> rt;
  Out<double> sy;
  TRY(stage_out(c, c->w_uh, uu_hat, (size_t)B * L.K, flags, uh));
  TRY(stage_out(c, c->w_ret, ret, (size_t)B, flags, rt));
  TRY(stage_out(c, c->w_cch, cc_hat, (size_t)B * L.N, flags, cch));
  TRY(stage_out(c, c->w_syn, syn, (size_t)B * L.M, flags, sy));
  // syndrom_soft semantics: rows not rewritten keep the caller's values
  if (sy.host) HIPCHK(c, hipMemcpyAsync(sy.dev, syn, sizeof(double) * sy.n, hipMemcpyHostToDevice, c->stream), "H2D");
  kml::BpLaunch a;
  a.B = B;
  a.iter_count = iter_count;
  a.max_iter = c->rc.max_iter;
  a.p0 = d_p0;
  a.p0_stride = L.cc_len;
  a.uu_hat = uh.dev;
  a.ret = rt.dev;
  a.cc_hat = cch.dev;
  a.syn = sy.dev;
  TRY(run_bp(c, a));
  // the reference writes uu_hat (and cc_hat_) only inside its iteration loop
  // (binaryldpccodec.cc:177-216): with iter_count = 0 the kernels write
  // neither, and the caller's arrays stay as they were
  if (iter_count > 0) {
    TRY(copy_out(c, uh));
    TRY(copy_out(c, cch));
  }
  TRY(copy_out(c, rt));
  TRY(copy_out(c, sy));
  return sync(c);
}

int kml_demap(kml_ctx *c, const double *y, const double *h, double var, int B, double *p0, int flags) {
  const bool ok = c && y && h && p0 && B >= 0;
  if (ok && B == 0) return KML_OK;
  TRY(gpu_begin(c, ok, "kml_demap: bad argument"));
  const int S = c->code.cc_len / c->modem.bits;
  const double *d_y, *d_h;
  TRY(stage_in(c, c->w_y, y, (size_t)B * S * 2, flags, d_y));
  TRY(stage_in(c, c->w_h, h, (size_t)B * 2, flags, d_h));
  Out<double> o;
  TRY(stage_out(c, c->w_p0, p0, (size_t)B * c->code.cc_len, flags, o));
  TRY(run_demap(c, as_c(d_y), 1, as_c(d_h), 1, nullptr, var, B, o.dev));
  TRY(copy_out(c, o));
  return sync(c);
}

int kml_demap_llr(kml_ctx *c, const double *y, const double *h, double var, int B, float *llr, int flags) {
  const bool ok = c && y && h && llr && B >= 0 && var > 0.0;
  if (ok && (c->device < 0 || !c->stream)) {
    call_begin(c);
    return fail(c, KML_E_UNSUP, "kml_demap_llr: host-only context (device < 0): no GPU operations");
  }
  if (ok && B == 0) return KML_OK;
  TRY(gpu_begin(c, ok, "kml_demap_llr: bad argument"));
  const int S = c->code.cc_len / c->modem.bits;
  const double *d_y, *d_h;
  TRY(stage_in(c, c->w_y, y, (size_t)B * S * 2, flags, d_y));
  TRY(stage_in(c, c->w_h, h, (size_t)B * 2, flags, d_h));
  Out<float> o;
  TRY(stage_out(c, c->w_llr, llr, (size_t)B * c->code.cc_len, flags, o));
  TRY(run_demap_llr(c, as_c(d_y), 1, as_c(d_h), 1, nullptr, var, B, o.dev));
  TRY(copy_out(c, o));
  return sync(c);
}

int kml_llr_decode(kml_ctx *c, const float *llr, int B, int iter_count, uint8_t *uu_hat, int32_t *ret, uint8_t *cc_hat,
                   float *llr_out, int flags) {
  const bool ok = c && llr && B >= 0 && iter_count >= 0;
  if (ok) {  // the refusals, before anything is staged or launched
    call_begin(c);
    if (c->device < 0 || !c->stream)
      return fail(c, KML_E_UNSUP, "kml_llr_decode: a host-only context (device < 0) has no min-sum decoder");
    if (c->algorithm != KML_ALG_NMS)
      return fail(c, KML_E_UNSUP,
                  "kml_llr_decode: float LLRs are decoded by the min-sum mode only (kml_set_algorithm(KML_ALG_NMS) "
                  "first)");
    TRY(schedule_refusal(c, "kml_llr_decode"));
    if (llr_out && c->schedule == KML_SCHED_FLOODING && !kml::bp_irregular_nms_post_supported(c->dc))
      return fail(c, KML_E_UNSUP,
                  "kml_llr_decode: the flooding kernel's posterior output (N more floats of LDS) does not fit this code; "
                  "llr_out must be NULL");
  }
  if (ok && B == 0) return KML_OK;
  TRY(gpu_begin(c, ok, "kml_llr_decode: bad argument"));
  const kml::LdpcCode &L = c->code;
  const float *d_llr;
  TRY(stage_in(c, c->w_llr, llr, (size_t)B * L.cc_len, flags, d_llr));
  Out<uint8_t> uh, cch;
  Out<int32_t> rt;
  Out<float> po;
  TRY(stage_out(c, c->w_uh, uu_hat, (size_t)B * L.K, flags, uh));
  TRY(stage_out(c, c->w_ret, ret, (size_t)B, flags, rt));
  TRY(stage_out(c, c->w_cch, cc_hat, (size_t)B * L.N, flags, cch));
  TRY(stage_out(c, c->w_post, llr_out, (size_t)B * L.N, flags, po));
  kml::BpLaunch a;
  a.B = B;
  a.iter_count = iter_count;
  a.max_iter = c->rc.max_iter;
  a.p0_stride = L.cc_len;
  a.uu_hat = uh.dev;
  a.ret = rt.dev;
  a.cc_hat = cch.dev;
  kml::LlrIoDev lio;
  lio.llr = d_llr;
  lio.post = po.dev;
  TRY(run_bp(c, a, nullptr, -1, false, &lio));
  if (iter_count > 0) {  // with iter_count = 0 the kernels write none of these: the caller's arrays stay
    TRY(copy_out(c, uh));
    TRY(copy_out(c, cch));
    TRY(copy_out(c, po));
  }
  TRY(copy_out(c, rt));
  return sync(c);
}

int kml_kmeans(kml_ctx *c, const double *y, int B, int iters, double *h_hat, double *h4, int flags) {
  const bool ok = c && y && B >= 0 && iters >= 0;
  if (ok && B == 0) return KML_OK;
  TRY(gpu_begin(c, ok, "kml_kmeans: bad argument"));
  const int S = c->code.cc_len / c->modem.bits;
  const double *d_y;
  TRY(stage_in(c, c->w_y, y, (size_t)B * S * 2, flags, d_y));
  // the kernel writes both outputs whether or not the caller wants them
  Out<double> hh, hr;
  TRY(stage_out(c, c->w_hhat, h_hat, (size_t)B * 2, flags, hh));
  TRY(stage_out(c, c->w_h4, h4, (size_t)B * 8, flags, hr));
  TRY(or_workspace(c, hh.dev, c->w_hhat, (size_t)B * 2));
  TRY(or_workspace(c, hr.dev, c->w_h4, (size_t)B * 8));
  TRY(run_kmeans(c, as_c(d_y), iters, B, as_c(hh.dev), as_c(hr.dev)));
  TRY(copy_out(c, hh));
  TRY(copy_out(c, hr));
  return sync(c);
}

int kml_kmeans_state(kml_ctx *c, const double *y, int B, int iters, double *clusters, int32_t *idx, int flags) {
  const bool ok = c && y && B >= 0 && iters >= 0;
  if (ok && B == 0) return KML_OK;
  TRY(gpu_begin(c, ok, "kml_kmeans_state: bad argument"));
  const int S = c->code.cc_len / c->modem.bits;
  const int Kc = c->modem.Kc;
  const double *d_y;
  TRY(stage_in(c, c->w_y, y, (size_t)B * S * 2, flags, d_y));
  HIPCHK(c, c->w_hhat.ensure(sizeof(double2) * B), "hipMalloc");
  HIPCHK(c, c->w_h4.ensure(sizeof(double2) * 4 * B), "hipMalloc");
  HIPCHK(c, c->w_h.ensure(sizeof(double2) * B), "hipMalloc");  // the final hatH
  Out<double> cl;
  Out<int32_t> ix;
  TRY(stage_out(c, c->w_met, clusters, (size_t)B * Kc * 2, flags, cl));
  TRY(stage_out(c, c->w_cwerr, idx, (size_t)B * S, flags, ix));
  TRY(run_kmeans(c, as_c(d_y), iters, B, c->w_hhat.as<double2>(), c->w_h4.as<double2>(), c->w_h.as<double2>()));
  HIPCHK(c, kml::launch_kmeans_state(Kc, c->d_cons.as<double>(), as_c(d_y), S, B, c->w_h.as<double2>(), as_c(cl.dev),
                                     ix.dev, c->stream),
         "kmeans_state");
  TRY(copy_out(c, cl));
  TRY(copy_out(c, ix));
  return sync(c);
}

int kml_comm_unique_id(uint8_t *id) {
  std::string err;
  if (!id) return KML_E_ARG;
  if (kml::rccl_unique_id(id, err) == 0) return KML_OK;
  g_free_err = "kml_comm_unique_id: " + err;
  return KML_E_UNSUP;
}

int kml_comm_init(kml_ctx *c, const uint8_t *id, int world, int rank) {
  TRY(gpu_begin(c, id && world >= 1 && rank >= 0 && rank < world, "kml_comm_init: bad argument"));
  if (c->comm) return fail(c, KML_E_ARG, "kml_comm_init: the context already has a communicator");
  std::string err;
  c->comm = kml::rccl_init(id, world, rank, err);
  return c->comm ? KML_OK : fail(c, KML_E_UNSUP, err);
}

int kml_comm_size(const kml_ctx *c) { return c ? kml::rccl_size(c->comm) : 0; }

int kml_comm_allreduce_u64(kml_ctx *c, uint64_t *vals, int n) { return comm_allreduce(c, vals, n, false); }
int kml_comm_allreduce_f64(kml_ctx *c, double *vals, int n) { return comm_allreduce(c, vals, n, true); }

int kml_debug_inject_abort(kml_ctx *c, int nth) {
  call_begin(c);
  if (!c) return KML_E_ARG;
  c->inject_fail = nth == -2;
  c->inject_abort = nth == -2 ? 0 : nth;
  return KML_OK;
}

int kml_decode_frames(kml_ctx *c, const double *y, const double *true_h, double snr, int B, uint8_t *uu_hat,
                      int32_t *chosen, double *metrics, int32_t *ret, double *h_hat, int flags) {
  const bool ok = c && y && uu_hat && B >= 0;
  if (ok && B == 0) return KML_OK;
  TRY(gpu_begin(c, ok, "kml_decode_frames: bad argument"));
  TRY(schedule_refusal(c, "kml_decode_frames"));
  if (!(flags & (KML_DEVICE_PTRS | KML_HISTOGRAM)) && (true_h || !c->rc.metric_soft)) {
    const int CH = host_chunk();
    if (CH > 0 && B > CH) {
      if (!true_h) return decode_frames_chunked(c, y, nullptr, snr, B, uu_hat, chosen, metrics, ret, h_hat, CH);
      if (chosen) memset(chosen, 0, sizeof(int32_t) * B);  // single candidate (kmcodec.cc:66-67)
      if (metrics) memset(metrics, 0, sizeof(double) * 4 * B);
      if (h_hat) memset(h_hat, 0, sizeof(double) * 2 * B);
      return decode_frames_chunked(c, y, true_h, snr, B, uu_hat, nullptr, nullptr, ret, nullptr, CH);
    }
  }
  const int S = c->code.cc_len / c->modem.bits;
  const double *d_y, *d_h = nullptr;
  TRY(stage_in(c, c->w_y, y, (size_t)B * S * 2, flags, d_y));
  if (true_h) TRY(stage_in(c, c->w_h, true_h, (size_t)B * 2, flags, d_h));
  DecodeOuts o;
  Out<double> hh;
  RecvIO io;
  TRY(stage_decode_outs(c, B, uu_hat, chosen, metrics, ret, flags, o, io));
  TRY(stage_out(c, c->w_hhat, h_hat, (size_t)B * 2, flags, hh));
  io.y = as_c(d_y);
  io.true_h = as_c(d_h);
  io.hhat = as_c(hh.dev);
  int slot;
  TRY(receive(c, io, snr, B, slot));
  if (true_h && !io.histogram) {  // single candidate: chosen = 0, metrics unset (kmcodec.cc:66-67)
    zero_out(o.chosen);
    zero_out(o.met);
  } else {
    TRY(copy_out(c, o.chosen));
    TRY(copy_out(c, o.met));
  }
  if (true_h)  // no k-means ran
    zero_out(hh);
  else
    TRY(copy_out(c, hh));
  return finish_decode(c, o, io.histogram);
}

int kml_decode_candidates(kml_ctx *c, const double *y, const double *h_hats, int nc, double snr, int B,
                          uint8_t *uu_hat, int32_t *chosen, double *metrics, int32_t *ret, int flags) {
  const bool ok = c && y && h_hats && uu_hat && B >= 0 && nc >= 1 && nc <= 4;
  // one estimate: Decoder computes no metric (kmcodec.cc:66-67); GetHistogramData
  // (kmcodec.cc:75-79, KML_HISTOGRAM) computes that candidate's metric, as the
  // known-channel histogram path of kml_decode_frames does
  if (ok && nc == 1) return kml_decode_frames(c, y, h_hats, snr, B, uu_hat, chosen, metrics, ret, nullptr, flags);
  if (ok && B == 0) return KML_OK;
  TRY(gpu_begin(c, ok, "kml_decode_candidates: bad argument (need 1 <= nc <= 4)"));
  TRY(schedule_refusal(c, "kml_decode_candidates"));
  const int S = c->code.cc_len / c->modem.bits;
  const double *d_y, *d_hc;
  TRY(stage_in(c, c->w_y, y, (size_t)B * S * 2, flags, d_y));
  TRY(stage_in(c, c->w_hc, h_hats, (size_t)B * nc * 2, flags, d_hc));
  DecodeOuts o;
  RecvIO io;
  TRY(stage_decode_outs(c, B, uu_hat, chosen, metrics, ret, flags, o, io));
  io.y = as_c(d_y);
  io.cand = as_c(d_hc);
  io.ncand = nc;
  int slot;
  TRY(receive(c, io, snr, B, slot));
  TRY(copy_out(c, o.chosen));
  TRY(copy_out(c, o.met));
  return finish_decode(c, o, io.histogram);
}

int kml_count_errors(kml_ctx *c, const uint8_t *uu, const uint8_t *uu_hat, int B, uint64_t *counters, int flags) {
  const bool ok = c && uu && uu_hat && counters && B >= 0;
  if (ok && B == 0) return KML_OK;
  TRY(gpu_begin(c, ok, "kml_count_errors: bad argument"));
  const size_t n = (size_t)B * c->code.K;
  const uint8_t *d_uu, *d_uh;
  TRY(stage_in(c, c->w_uu, uu, n, flags, d_uu));
  TRY(stage_in(c, c->w_uh, uu_hat, n, flags, d_uh));
  int slot;
  TRY(fresh_slot(c, slot));
  HIPCHK(c, kml::launch_count_bytes(d_uu, d_uh, c->code.K, B, slot_ptr(c, slot), c->stream), "count");
  return read_back(c, slot_ptr(c, slot), counters, 4, true);
}

int kml_sim_generate(kml_ctx *c, double snr, uint64_t seed, uint64_t first_cw, int B) {
  TRY(gpu_begin(c, B >= 0, "kml_sim_generate: bad argument"));
  const kml::LdpcCode &L = c->code;
  const int S = L.cc_len / c->modem.bits;
  const int Cw = (L.cc_len + 63) / 64;
  HIPCHK(c, c->s_uu.ensure(sizeof(uint64_t) * (size_t)B * L.Kw), "hipMalloc(sim uu)");
  HIPCHK(c, c->s_cc.ensure(sizeof(uint64_t) * (size_t)B * Cw), "hipMalloc(sim cc)");
  HIPCHK(c, c->s_y.ensure(sizeof(double2) * (size_t)B * S), "hipMalloc(sim y)");
  HIPCHK(c, c->s_h.ensure(sizeof(double2) * (size_t)B), "hipMalloc(sim h)");
  double var, sigma, ns;
  kml::channel_constants(snr, var, sigma, ns);
  kml::FrameLaunch f;
  f.B = B;
  f.seed = seed;
  f.first_cw = first_cw;
  f.noise_scale = ns;
  f.uu_bits = c->s_uu.as<uint64_t>();
  f.cc_bits = c->s_cc.as<uint64_t>();
  f.y = c->s_y.as<double2>();
  f.h = c->s_h.as<double2>();
  Timer t(c, "framegen", -1, 0.0);
  HIPCHK(c, kml::launch_framegen(c->dc, c->modem.bits, c->d_cons.as<double>(), f, c->stream), "framegen");
  t.stop();
  c->sim_B = B;
  c->sim_first = first_cw;
  return sync(c);
}

int kml_sim_decode(kml_ctx *c, double snr, int blind, uint64_t *counters, int do_sync) {
  TRY(gpu_begin(c, do_sync || !counters, "counters need sync != 0"));
  TRY(schedule_refusal(c, "kml_sim_decode"));
  if (c->sim_B == 0) return KML_OK;
  int slot = 0;
  TRY(sim_receive(c, snr, blind, false, slot));
  return counters ? read_back(c, slot_ptr(c, slot), counters, kml::CNT_N) : KML_OK;
}

int kml_sim_decode_ex(kml_ctx *c, double snr, int blind, int histogram, int32_t *cw_err, double *metrics,
                      uint64_t *counters) {
  TRY(gpu_begin(c));
  TRY(schedule_refusal(c, "kml_sim_decode_ex"));
  const size_t B = (size_t)c->sim_B;
  if (B == 0) {
    if (counters) memset(counters, 0, sizeof(uint64_t) * kml::CNT_N);
    return KML_OK;
  }
  int slot = 0;
  TRY(sim_receive(c, snr, blind, histogram != 0, slot));
  if (metrics && !histogram) memset(metrics, 0, sizeof(double) * 4 * B);
  return read_back(c, slot_ptr(c, slot), counters, kml::CNT_N, false,
                   {{cw_err, c->w_cwerr.p, sizeof(int32_t) * B},
                    {histogram ? metrics : nullptr, c->w_met.p, sizeof(double) * 4 * B}});
}

int kml_sim_decode_profile(kml_ctx *c, double snr, int blind, uint64_t *prof, int32_t *cw_prof, uint64_t *counters) {
  call_begin(c);
  if (!c) return KML_E_ARG;
  // every refusal is decided here, before anything is launched
  if (c->device < 0 || !c->stream)
    return fail(c, KML_E_UNSUP, "kml_sim_decode_profile: host-only context (device < 0): no GPU operations");
  const int P = c->rc.max_iter;
  if (P < 1) return fail(c, KML_E_ARG, "kml_sim_decode_profile: max_iter must be >= 1");
  if (c->precision != KML_PREC_F64)
    return fail(c, KML_E_UNSUP, "kml_sim_decode_profile: the iteration profile is not available in the f32 mode");
  if (c->algorithm != KML_ALG_SPA)
    return fail(c, KML_E_UNSUP,
                "kml_sim_decode_profile: the iteration profile is not available in the min-sum mode (KML_ALG_NMS)");
  if (c->rc.metric_soft)
    return fail(c, KML_E_UNSUP,
                "kml_sim_decode_profile: the iteration profile is not available with the soft-syndrome metric "
                "(metric_type = 1)");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  if (const char *why = kml::bp_profile_refusal(c->dc, P))
    return fail(c, KML_E_UNSUP, std::string("kml_sim_decode_profile: ") + why);
  const size_t B = (size_t)c->sim_B, prof_bytes = sizeof(unsigned long long) * 3 * (size_t)P;
  if (prof) memset(prof, 0, prof_bytes);
  if (B == 0) {
    if (counters) memset(counters, 0, sizeof(uint64_t) * kml::CNT_N);
    return KML_OK;
  }
  HIPCHK(c, c->w_prof.ensure(prof_bytes), "hipMalloc(prof)");
  HIPCHK(c, c->w_cwprof.ensure(sizeof(int32_t) * B * P), "hipMalloc(cw_prof)");
  HIPCHK(c, hipMemsetAsync(c->w_prof.p, 0, prof_bytes, c->stream), "memset");
  int slot = 0;
  TRY(sim_receive(c, snr, blind, false, slot, c->w_cwprof.as<int32_t>(), c->w_prof.as<unsigned long long>()));
  return read_back(c, slot_ptr(c, slot), counters, kml::CNT_N, false,
                   {{prof, c->w_prof.p, prof_bytes}, {cw_prof, c->w_cwprof.p, sizeof(int32_t) * B * P}});
}

int kml_run_config(const kml_ctx *c, double *f, int64_t *n) {
  if (!c) return KML_E_ARG;
  const kml::RunConfig &r = c->rc;
  const double fv[3] = {r.min_snr, r.max_snr, r.step_snr};
  const int64_t nv[10] = {r.max_err_blk, r.max_num_blk, r.thread_num_blk, r.known_h,     r.is5g,
                          r.metric_soft, r.metric_iter, r.histogram,      r.max_iter,    r.active};
  if (f) std::copy(fv, fv + 3, f);
  if (n) std::copy(nv, nv + 10, n);
  return KML_OK;
}

int kml_sync(kml_ctx *c) {
  TRY(gpu_begin(c));
  return sync(c);
}

int kml_sim_load(kml_ctx *c, double snr, const uint8_t *uu, const double *y, const double *h, int B,
                 uint64_t first_cw) {
  TRY(gpu_begin(c, B >= 0 && (B == 0 || (uu && y && h)), "kml_sim_load: bad argument"));
  const kml::LdpcCode &L = c->code;
  const int S = L.cc_len / c->modem.bits;
  HIPCHK(c, c->s_uu.ensure(sizeof(uint64_t) * (size_t)std::max(B, 1) * L.Kw), "hipMalloc(sim uu)");
  HIPCHK(c, c->s_y.ensure(sizeof(double2) * (size_t)std::max(B, 1) * S), "hipMalloc(sim y)");
  HIPCHK(c, c->s_h.ensure(sizeof(double2) * (size_t)std::max(B, 1)), "hipMalloc(sim h)");
  TRY(sync(c));
  // source bits packed as the frame generator writes them: bit i of word i/64
  std::vector<uint64_t> w((size_t)B * L.Kw, 0);
  for (int b = 0; b < B; b++)
    for (int i = 0; i < L.K; i++)
      if (uu[(size_t)b * L.K + i]) w[(size_t)b * L.Kw + (i >> 6)] |= 1ull << (i & 63);
  if (B > 0) {
    HIPCHK(c, hipMemcpy(c->s_uu.p, w.data(), w.size() * 8, hipMemcpyHostToDevice), "H2D");
    HIPCHK(c, hipMemcpy(c->s_y.p, y, sizeof(double2) * (size_t)B * S, hipMemcpyHostToDevice), "H2D");
    HIPCHK(c, hipMemcpy(c->s_h.p, h, sizeof(double2) * (size_t)B, hipMemcpyHostToDevice), "H2D");
  }
  c->sim_B = B;
  c->sim_first = first_cw;
  return KML_OK;
}

int kml_sim_frames(kml_ctx *c, uint8_t *uu, double *y, double *h) {
  TRY(gpu_begin(c));
  const kml::LdpcCode &L = c->code;
  const int B = c->sim_B, S = L.cc_len / c->modem.bits;
  TRY(sync(c));
  if (uu) {
    std::vector<uint64_t> w((size_t)B * L.Kw);
    HIPCHK(c, hipMemcpy(w.data(), c->s_uu.p, w.size() * 8, hipMemcpyDeviceToHost), "D2H");
    for (int b = 0; b < B; b++)
      for (int i = 0; i < L.K; i++) uu[(size_t)b * L.K + i] = (w[(size_t)b * L.Kw + (i >> 6)] >> (i & 63)) & 1;
  }
  if (y) HIPCHK(c, hipMemcpy(y, c->s_y.p, sizeof(double2) * (size_t)B * S, hipMemcpyDeviceToHost), "D2H");
  if (h) HIPCHK(c, hipMemcpy(h, c->s_h.p, sizeof(double2) * (size_t)B, hipMemcpyDeviceToHost), "D2H");
  return KML_OK;
}

int kml_prof_enable(kml_ctx *c, int on) {
  call_begin(c);
  if (!c) return KML_E_ARG;
  c->prof = on != 0;
  return KML_OK;
}

int kml_prof_reset(kml_ctx *c) {
  call_begin(c);
  if (!c) return KML_E_ARG;
  drain_profile(c);
  c->stats.clear();
  return KML_OK;
}

int kml_prof_read_flops(kml_ctx *c, const char *stage, double *alg_flops) {
  if (!c || !stage || !alg_flops) return KML_E_ARG;
  *alg_flops = drained_stat(c, stage).flops;
  return KML_OK;
}

int kml_prof_read(kml_ctx *c, const char *stage, int64_t *launches, double *total_ms, double *alg_bytes) {
  if (!c || !stage) return KML_E_ARG;
  const Stat s = drained_stat(c, stage);
  if (launches) *launches = s.launches;
  if (total_ms) *total_ms = s.ms;
  if (alg_bytes) *alg_bytes = s.bytes;
  return KML_OK;
}

int kml_ref_frames(const kml_ctx *c, int64_t *state, double snr, int n, uint8_t *uu, double *true_h, double *y) {
  if (!c || !state || n < 0 || (n > 0 && (!uu || !true_h || !y))) return KML_E_ARG;
  return kml::ref_frames(c->code, c->modem, state, snr, n, uu, true_h, y);
}

int kml_log_probe(kml_ctx *c, const double *in, int n, double *out) {
  return run_probe(c, in, n, out, 1, 1, kml::launch_log_probe);
}
int kml_math_probe(kml_ctx *c, const double *in, int n, double *out) {
  return run_probe(c, in, n, out, 4, 4, kml::launch_math_probe);
}
int kml_div_probe(kml_ctx *c, const double *in, int n, double *out) {
  return run_probe(c, in, n, out, 3, 12, kml::launch_div_probe);
}

}  // extern "C"
