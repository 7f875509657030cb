// receive.cpp — the receive path (KmCodec::Decoder / GetHistogramData,
// kmcodec.cc:54-163) over the kernels: known channel, or candidate channel
// estimates + a syndrome metric + the final decode; and kml_decode_frames'
// chunked host-buffer variant.
#include "capi_internal.hpp"
#include "soft_walk.hpp"

namespace kml_host {
namespace {

// The final decode of a receive: max_iter iterations, the caller's outputs.
// After metric_decodes (nc > 0) its P0 is the chosen candidate's, in w_p0.
kml::BpLaunch final_launch(kml_ctx *c, const RecvIO &io, int B, int nc = 0, const int32_t *chosen = nullptr) {
  kml::BpLaunch a;
  a.B = B;
  a.iter_count = c->rc.max_iter;
  a.max_iter = c->rc.max_iter;
  a.uu_hat = io.uh;
  a.ret = io.ret;
  a.ref_bits = io.ref_bits;
  a.cw_err = io.cw_err;
  a.cw_prof = io.cw_prof;  // the final decode only: the candidate-metric launches are their own BpLaunch
  a.cw_prof_stride = c->rc.max_iter;
  a.prof = io.prof;
  if (nc) {
    a.p0 = c->w_p0.as<double>();
    a.p0_stride = (long long)c->code.cc_len * nc;
    a.p0_sel = chosen;
    a.p0_sel_stride = (long long)c->code.cc_len;
  }
  return a;
}

// Demap every codeword with h[b * h_stride + (h_sel ? h_sel[b] : 0)], then
// decode: in the BP prologue when the regular kernel can, a launch of its own
// otherwise.
int demap_then_bp(kml_ctx *c, kml::BpLaunch a, const double2 *y, const double2 *h, int h_stride, const int32_t *h_sel,
                  double var, int &bp_slot) {
  if (kml::bp_regular_fuses_demap(c->dc, c->modem.bits)) {
    a.sym_y = y;
    a.sym_h = h;
    a.sym_h_stride = h_stride;
    a.sym_h_sel = h_sel;
    a.sym_cons = c->d_cons.as<double>();
    a.sym_var = var;
    a.sym_bits = c->modem.bits;
    return run_bp(c, a, &bp_slot);
  }
  const size_t cc = (size_t)c->code.cc_len;
  HIPCHK(c, c->w_p0.ensure(sizeof(double) * cc * a.B), "hipMalloc(p0)");
  TRY(run_demap(c, y, 1, h, h_stride, h_sel, var, a.B, c->w_p0.as<double>()));
  a.p0 = c->w_p0.as<double>();
  a.p0_stride = (long long)cc;
  return run_bp(c, a, &bp_slot);
}

// The max-log front end (KML_DEMAP_MAXLOG, the min-sum mode only).
bool maxlog(const kml_ctx *c) { return c->demapper == KML_DEMAP_MAXLOG && c->algorithm == KML_ALG_NMS; }

// demap_then_bp under it: float LLRs from demap_llr into w_llr, decoded by the
// context's min-sum kernel (there is no fused form).
int demap_llr_then_bp(kml_ctx *c, kml::BpLaunch a, const double2 *y, const double2 *h, int h_stride,
                      const int32_t *h_sel, double var, int &bp_slot) {
  const size_t cc = (size_t)c->code.cc_len;
  HIPCHK(c, c->w_llr.ensure(sizeof(float) * cc * a.B), "hipMalloc(llr)");
  TRY(run_demap_llr(c, y, 1, h, h_stride, h_sel, var, a.B, c->w_llr.as<float>()));
  kml::LlrIoDev lio;
  lio.llr = c->w_llr.as<float>();
  a.p0_stride = (long long)cc;
  return run_bp(c, a, &bp_slot, -1, false, &lio);
}

// The candidates' metric decodes (5G hard metric and soft metric): P0 of all
// nc * B candidates into w_p0, then BP for metric_iter iterations with the
// outputs `m` asks for.  Histogram mode keeps their uu_hat (w_uh4): CntErr
// reads the last candidate's.  Under KML_DEMAP_MAXLOG (5G hard metric only: the
// soft metric is refused in the min-sum mode) the candidates' max-log LLRs go
// into w_llr instead and the context's min-sum decoder runs the metric_iter
// iterations.
int metric_decodes(kml_ctx *c, const RecvIO &io, double var, int B, const double2 *hc, int nc, kml::BpLaunch &m) {
  const size_t cc = (size_t)c->code.cc_len, nB = (size_t)nc * B;
  m.B = (int)nB;
  m.iter_count = c->rc.metric_iter;
  m.max_iter = c->rc.max_iter;
  m.p0_stride = (long long)cc;
  if (io.histogram) {
    HIPCHK(c, c->w_uh4.ensure(nB * c->code.K), "hipMalloc(uh4)");
    m.uu_hat = c->w_uh4.as<uint8_t>();
  }
  if (maxlog(c)) {  // max-log LLRs of the candidates into w_llr, the context's min-sum decoder
    HIPCHK(c, c->w_llr.ensure(sizeof(float) * cc * nB), "hipMalloc(llr)");
    TRY(run_demap_llr(c, io.y, nc, hc, 1, nullptr, var, (int)nB, c->w_llr.as<float>()));
    kml::LlrIoDev lio;
    lio.llr = c->w_llr.as<float>();
    return run_bp(c, m, nullptr, -1, false, &lio);
  }
  HIPCHK(c, c->w_p0.ensure(sizeof(double) * cc * nB), "hipMalloc(p0)");
  TRY(run_demap(c, io.y, nc, hc, 1, nullptr, var, (int)nB, c->w_p0.as<double>()));
  m.p0 = c->w_p0.as<double>();
  return run_bp(c, m, nullptr, -1, true);
}

// Histogram mode ends here: CntErr into `cnt` against the uu_hat the last of
// the nc candidates' metric decodes left in w_uh4 — or against zeros where no
// decode ran (nc = 0: the hard PEG metric) — and the same bits to io.uh.
int histogram_tail(kml_ctx *c, const RecvIO &io, int B, int nc, unsigned long long *cnt) {
  const int K = c->code.K, Kw = c->code.Kw;
  const uint8_t *last = nc ? c->w_uh4.as<uint8_t>() + (size_t)(nc - 1) * K : nullptr;
  if (io.ref_bits)
    HIPCHK(c, kml::launch_count_packed(io.ref_bits, Kw, K, last, (long long)nc * K, B, io.cw_err, cnt, c->stream),
           "count");
  if (io.uh && !last) HIPCHK(c, hipMemsetAsync(io.uh, 0, (size_t)B * K, c->stream), "memset uh");
  if (io.uh && last)
    HIPCHK(c, hipMemcpy2DAsync(io.uh, K, last, (size_t)nc * K, K, B, hipMemcpyDeviceToDevice, c->stream), "copy uh");
  return KML_OK;
}

// Soft syndrome metric: the candidates' decodes and log sums run batched on the
// GPU; kml::SoftWalk (soft_walk.hpp) resolves the stale syndrom_soft_ reads on
// the host and says, round by round, which codewords' choices are known — they
// are decoded — and whose final decode it must see before it can go on.
int soft_receive(kml_ctx *c, const RecvIO &io, double var, int B, const double2 *hc, int nc, int32_t *d_chosen,
                 double *d_met, int &bp_slot) {
  const int M = c->code.M;
  // the walk takes a final decode for a repeat of its candidate's metric
  // decode and feeds its syndromes to the next codeword's metrics: one arithmetic
  if (c->precision != KML_PREC_F64)
    return fail(c, KML_E_UNSUP, "the soft-syndrome metric (metric_type = 1) is not available in the f32 mode");
  const size_t nB = (size_t)nc * B;
  HIPCHK(c, c->s_synm.ensure(sizeof(double) * (size_t)M * nB), "hipMalloc(syn)");
  HIPCHK(c, c->s_itm.ensure(sizeof(int32_t) * nB), "hipMalloc(iters)");
  HIPCHK(c, c->s_Lm.ensure(sizeof(double) * nB), "hipMalloc(L)");
  kml::BpLaunch m;
  m.syn = c->s_synm.as<double>();
  m.iters = c->s_itm.as<int32_t>();
  TRY(metric_decodes(c, io, var, B, hc, nc, m));
  {
    Timer t(c, "metric", -1, (double)nB * M * 8.0);
    HIPCHK(c, kml::launch_soft_sum(m.syn, M, m.iters, nullptr, (int)nB, c->s_Lm.as<double>(), c->stream), "soft sum");
    t.stop();
  }
  std::vector<int32_t> itm(nB);
  std::vector<double> Lm(nB);
  HIPCHK(c, hipMemcpyAsync(itm.data(), m.iters, sizeof(int32_t) * nB, hipMemcpyDeviceToHost, c->stream), "D2H");
  HIPCHK(c, hipMemcpyAsync(Lm.data(), c->s_Lm.p, sizeof(double) * nB, hipMemcpyDeviceToHost, c->stream), "D2H");
  TRY(sync(c));

  kml::SoftWalk w(B, nc, c->rc.metric_iter, c->rc.max_iter, itm.data(), Lm.data(), c->soft_state, io.sim, io.first_cw,
                  c->rc.thread_num_blk);
  auto upload_chosen = [&] {
    return hipMemcpyAsync(d_chosen, w.chosen.data(), sizeof(int32_t) * B, hipMemcpyHostToDevice, c->stream);
  };
  auto upload_met = [&] {
    return hipMemcpyAsync(d_met, w.met.data(), sizeof(double) * 4 * B, hipMemcpyHostToDevice, c->stream);
  };
  if (io.histogram) {  // GetHistogramData: metric decodes only
    w.metrics_only();
    if (!io.sim) c->soft_state = w.state;
    HIPCHK(c, upload_chosen(), "H2D");
    HIPCHK(c, upload_met(), "H2D");
    TRY(fresh_slot(c, bp_slot));
    TRY(histogram_tail(c, io, B, nc, slot_ptr(c, bp_slot)));
    return sync(c);
  }

  // final decodes, in rounds
  HIPCHK(c, c->s_synf.ensure(sizeof(double) * (size_t)M * B), "hipMalloc(syn final)");
  HIPCHK(c, c->s_itf.ensure(sizeof(int32_t) * B), "hipMalloc(iters final)");
  HIPCHK(c, c->s_Lf.ensure(sizeof(double) * B), "hipMalloc(L final)");
  HIPCHK(c, c->s_list.ensure(sizeof(int32_t) * B), "hipMalloc(list)");
  kml::BpLaunch a = final_launch(c, io, B, nc, d_chosen);
  a.syn = c->s_synf.as<double>();
  a.iters = c->s_itf.as<int32_t>();
  TRY(fresh_slot(c, bp_slot));
  while (!w.done()) {
    const kml::SoftWalk::Round r = w.next();
    int32_t *d_list = c->s_list.as<int32_t>() + r.first;
    HIPCHK(c, upload_chosen(), "H2D");
    HIPCHK(c, hipMemcpyAsync(d_list, w.list.data() + r.first, sizeof(int32_t) * r.n, hipMemcpyHostToDevice, c->stream),
           "H2D list");
    a.B = r.n;
    a.cw_idx = d_list;
    TRY(run_bp(c, a, nullptr, bp_slot));
    if (r.feedback >= 0) {  // the round's last codeword: its final decode sets the state
      HIPCHK(c, kml::launch_soft_sum(a.syn, M, a.iters, d_list + (r.n - 1), 1, c->s_Lf.as<double>(), c->stream),
             "soft sum");
      int32_t itf = 0;
      double Lf = 0.0;
      HIPCHK(c, hipMemcpyAsync(&itf, a.iters + r.feedback, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream), "D2H");
      HIPCHK(c, hipMemcpyAsync(&Lf, c->s_Lf.as<double>() + r.feedback, sizeof(Lf), hipMemcpyDeviceToHost, c->stream),
             "D2H");
      TRY(sync(c));
      w.feed(itf, Lf);
    }
  }
  if (!io.sim) c->soft_state = w.state;
  HIPCHK(c, upload_met(), "H2D");
  return sync(c);
}

}  // namespace

int receive(kml_ctx *c, const RecvIO &io, double snr, int B, int &bp_slot) {
  double var, sigma, ns;
  kml::channel_constants(snr, var, sigma, ns);
  // the soft walk reads the final decodes' syndrom_soft, which min-sum does not
  // have: refused before k-means or anything else is launched
  if (c->algorithm == KML_ALG_NMS && c->rc.metric_soft && !(io.true_h && !io.histogram))
    return fail(c, KML_E_UNSUP,
                "the soft-syndrome metric (metric_type = 1) is not available in the min-sum mode (KML_ALG_NMS)");
  // KML_DEMAP_MAXLOG: the final decode's priors, and a 5G code's candidate
  // metric decodes, come from demap_llr and run the context's min-sum decoder;
  // k-means, the hard metric of a non-5G code, launch_select and the histogram
  // tail are the exact mode's
  const bool llr = maxlog(c);
  auto demap_bp = [&](const double2 *h, int h_stride, const int32_t *h_sel) {
    return llr ? demap_llr_then_bp(c, final_launch(c, io, B), io.y, h, h_stride, h_sel, var, bp_slot)
               : demap_then_bp(c, final_launch(c, io, B), io.y, h, h_stride, h_sel, var, bp_slot);
  };
  if (io.true_h && !io.histogram)  // known channel: no candidates, no metric
    return demap_bp(io.true_h, 1, nullptr);
  // candidate channel estimates: the caller's, the true h (histogram on the
  // known-H path), or k-means + 4 rotations (simulator.cc:136-148)
  const double2 *hc = io.cand ? io.cand : io.true_h;
  int nc = io.cand ? io.ncand : 1;
  if (!hc) {
    double2 *hh = io.hhat;
    HIPCHK(c, c->w_h4.ensure(sizeof(double2) * 4 * B), "hipMalloc(h4)");
    TRY(or_workspace(c, hh, c->w_hhat, (size_t)B));
    TRY(run_kmeans(c, io.y, 20, B, hh, c->w_h4.as<double2>()));
    hc = c->w_h4.as<double2>();
    nc = 4;
  }
  int32_t *chosen = io.chosen;
  double *met = io.met;
  TRY(or_workspace(c, chosen, c->w_sel, (size_t)B));
  TRY(or_workspace(c, met, c->w_met, (size_t)4 * B));
  if (c->rc.metric_soft) return soft_receive(c, io, var, B, hc, nc, chosen, met, bp_slot);
  // histogram mode: the counters go to a fresh arena slot (read back like BP's)
  unsigned long long *hist_cnt = nullptr;
  if (io.histogram) {
    TRY(fresh_slot(c, bp_slot));
    hist_cnt = slot_ptr(c, bp_slot);
  }
  if (!c->code.is5g) {  // hard metric on the demapper output (kmcodec.cc:109-117)
    const int S = c->code.cc_len / c->modem.bits;
    Timer t(c, "metric", -1, (double)B * nc * S * 16.0);
    kml::DemapDefer dd;
    TRY(demap_defer(c, B, dd));
    HIPCHK(c, kml::launch_cand_metric(c->dc, c->modem.bits, c->d_cons.as<double>(), io.y, S, hc, nc, var, B, met,
                                      chosen, dd, c->stream),
           "cand_metric");
    t.stop();
    if (io.histogram) return histogram_tail(c, io, B, 0, hist_cnt);
    return demap_bp(hc, nc, chosen);
  }
  // 5G: metric = parity count after metric_iter BP iterations (kmcodec.cc:157-160)
  HIPCHK(c, c->w_pc.ensure(sizeof(int32_t) * nc * B), "hipMalloc(pc)");
  kml::BpLaunch m;
  m.parity_cnt = c->w_pc.as<int32_t>();
  TRY(metric_decodes(c, io, var, B, hc, nc, m));
  HIPCHK(c, kml::launch_select(m.parity_cnt, nc, B, met, chosen, c->stream), "select");
  if (io.histogram) return histogram_tail(c, io, B, nc, hist_cnt);
  if (llr) {  // the chosen candidate's LLRs are in w_llr, addressed as its P0 would be in w_p0
    kml::LlrIoDev lio;
    lio.llr = c->w_llr.as<float>();
    return run_bp(c, final_launch(c, io, B, nc, chosen), &bp_slot, -1, false, &lio);
  }
  return run_bp(c, final_launch(c, io, B, nc, chosen), &bp_slot);
}

// kml_decode_frames with HOST buffers, in chunks: the frames of chunk i + 1
// cross PCIe on the copy stream while chunk i decodes on the context's stream
// (which waits on the upload's event), and chunk i's outputs come back before
// chunk i + 1 is launched.  Chunks decode in order on one stream, so every
// codeword sees what it sees in one call: the known-channel and hard-metric
// decodes have no cross-codeword state (the soft metric's stale syndrom_soft_
// has; its calls stay in one piece).  Only the transfers move.  chosen /
// metrics / h_hat are the blind path's outputs (NULL on the known path).
int decode_frames_chunked(kml_ctx *c, const double *y, const double *true_h, double snr, int B, uint8_t *uu_hat,
                          int32_t *chosen, double *metrics, int32_t *ret, double *h_hat, int CH) {
  const int S = c->code.cc_len / c->modem.bits, K = c->code.K;
  const size_t ycw = (size_t)S * 2;  // doubles per codeword
  HIPCHK(c, c->w_y.ensure((size_t)B * ycw * sizeof(double)), "hipMalloc(workspace)");
  if (true_h) HIPCHK(c, c->w_h.ensure((size_t)B * 2 * sizeof(double)), "hipMalloc(workspace)");
  HIPCHK(c, c->w_uh.ensure((size_t)B * K), "hipMalloc(workspace)");
  if (ret) HIPCHK(c, c->w_ret.ensure((size_t)B * sizeof(int32_t)), "hipMalloc(workspace)");
  if (chosen) HIPCHK(c, c->w_sel.ensure((size_t)B * sizeof(int32_t)), "hipMalloc(workspace)");
  if (metrics) HIPCHK(c, c->w_met.ensure((size_t)B * 4 * sizeof(double)), "hipMalloc(workspace)");
  if (h_hat) HIPCHK(c, c->w_hhat.ensure((size_t)B * 2 * sizeof(double)), "hipMalloc(workspace)");
  if (!c->cstream) HIPCHK(c, hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking), "hipStreamCreate");
  const int n = (B + CH - 1) / CH;
  std::vector<hipEvent_t> ev(n, nullptr);
  int rc = KML_OK;
  auto upload = [&](int i) -> int {
    const size_t b0 = (size_t)i * CH, nb = std::min<size_t>(CH, B - b0);
    HIPCHK(c, hipEventCreateWithFlags(&ev[i], hipEventDisableTiming), "hipEventCreate");
    HIPCHK(c, hipMemcpyAsync(c->w_y.as<double>() + b0 * ycw, y + b0 * ycw, nb * ycw * sizeof(double),
                             hipMemcpyHostToDevice, c->cstream), "H2D");
    if (true_h)
      HIPCHK(c, hipMemcpyAsync(c->w_h.as<double>() + b0 * 2, true_h + b0 * 2, nb * 2 * sizeof(double),
                               hipMemcpyHostToDevice, c->cstream), "H2D");
    HIPCHK(c, hipEventRecord(ev[i], c->cstream), "hipEventRecord");
    return KML_OK;
  };
  rc = upload(0);
  for (int i = 0; i < n && rc == KML_OK; ++i) {
    const size_t b0 = (size_t)i * CH;
    const int nb = (int)std::min<size_t>(CH, B - b0);
    if (hipStreamWaitEvent(c->stream, ev[i], 0) != hipSuccess) {
      rc = fail(c, KML_E_HIP, "hipStreamWaitEvent");
      break;
    }
    RecvIO io;
    io.y = reinterpret_cast<const double2 *>(c->w_y.as<double>() + b0 * ycw);
    io.true_h = true_h ? reinterpret_cast<const double2 *>(c->w_h.as<double>() + b0 * 2) : nullptr;
    io.uh = c->w_uh.as<uint8_t>() + b0 * K;
    io.ret = ret ? c->w_ret.as<int32_t>() + b0 : nullptr;
    io.chosen = chosen ? c->w_sel.as<int32_t>() + b0 : nullptr;
    io.met = metrics ? c->w_met.as<double>() + b0 * 4 : nullptr;
    io.hhat = h_hat ? reinterpret_cast<double2 *>(c->w_hhat.as<double>() + b0 * 2) : nullptr;
    int slot;
    if ((rc = receive(c, io, snr, nb, slot)) != KML_OK) break;
    if (i + 1 < n && (rc = upload(i + 1)) != KML_OK) break;  // overlaps chunk i's decode
    // the chunk's rows of one output (`per` elements per codeword) back to the caller's array, if wanted
    auto back = [&](auto *dst, const void *src, size_t per) {
      return !dst || hipMemcpyAsync(dst + b0 * per, src, sizeof(*dst) * per * nb, hipMemcpyDeviceToHost, c->stream) ==
                         hipSuccess;
    };
    if (!(back(uu_hat, io.uh, K) && back(ret, io.ret, 1) && back(chosen, io.chosen, 1) && back(metrics, io.met, 4) &&
          back(h_hat, io.hhat, 2))) {
      rc = fail(c, KML_E_HIP, "D2H");
      break;
    }
  }
  if (rc != KML_OK) {  // leave no upload in flight into the workspaces
    hipStreamSynchronize(c->cstream);
    hipStreamSynchronize(c->stream);
  } else {
    rc = sync(c);
  }
  for (hipEvent_t e : ev)
    if (e) hipEventDestroy(e);
  return rc;
}

}  // namespace kml_host
