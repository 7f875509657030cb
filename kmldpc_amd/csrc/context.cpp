// context.cpp — the context behind the C ABI: one context = one GPU + one HIP
// stream + one code/modem.  Its creation (planner + graph upload) and
// destruction, the error and abort-word bookkeeping, the stage profiler, and
// the BP / demap / k-means launches every path above goes through.
#include <cstdio>

#include "bp_launch.hpp"
#include "capi_internal.hpp"

namespace kml_host {

// An error return of a call that made a cooperative launch and will not reach
// its sync(): the launch's abort word is settled here (waited for, dropped with
// the call's error), so the next call's first launch clears it instead of
// inheriting it (a stale timeout reported against a healthy call).  A pending
// launch of an EARLIER call (kml_sim_decode with do_sync = 0) stays pending
// for its own kml_sync: when this call's launches shared its abort word
// (coop_inherited) and the word is set, it stays pending.
static bool coop_aborted(kml_ctx *c, unsigned *why = nullptr) {  // reads the shared abort word
  kml::BpLaunch a;
  a.gsync = c->d_gsync.p;
  return kml::bp_coop_aborted(a, c->coop_groups, c->stream, why);
}

int fail(kml_ctx *c, int code, const std::string &msg) {
  if (c) {
    c->err = msg;
    if (c->coop_pending && c->coop_this_call) {
      bool keep = false;
      if (c->stream) {
        (void)hipStreamSynchronize(c->stream);
        if (c->coop_inherited) keep = coop_aborted(c);
      }
      c->coop_pending = keep;
      c->coop_this_call = false;
    }
  }
  return code;
}

int hip_fail(kml_ctx *c, hipError_t e, const char *what) {
  return fail(c, KML_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

int gpu_begin(kml_ctx *c, bool args_ok, const char *bad_args) {
  call_begin(c);
  if (!c || !args_ok) return bad_args ? fail(c, KML_E_ARG, bad_args) : KML_E_ARG;
  if (c->device < 0 || !c->stream) return fail(c, KML_E_ARG, "host-only context (device < 0): no GPU operations");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return KML_OK;
}

int schedule_refusal(kml_ctx *c, const char *who) {
  if (!c->lnms_only || c->algorithm != KML_ALG_NMS || c->schedule != KML_SCHED_FLOODING) return KML_OK;
  return fail(c, KML_E_UNSUP,
              std::string(who) +
                  ": this code's min-sum decoders are the layered ones only (it has no round plan of the flooding "
                  "kernel): kml_set_schedule(KML_SCHED_LAYERED) first; nothing was launched");
}

namespace {
// Packs the graph's arrays into one device allocation: add() each array,
// copy `host` to the device once, then ptr() each handle.
struct GraphPacker {
  std::vector<unsigned char> host;
  const unsigned char *base = nullptr;  // the device copy, set after the upload
  template <class T>
  size_t add(const std::vector<T> &v, size_t min_elems = 0) {
    const size_t off = (host.size() + 255) & ~size_t(255);
    host.resize(off + std::max(v.size(), min_elems) * sizeof(T), 0);
    if (!v.empty()) memcpy(host.data() + off, v.data(), v.size() * sizeof(T));
    return off;
  }
  template <class T>
  const T *ptr(size_t handle) const {
    return reinterpret_cast<const T *>(base + handle);
  }
};

int upload_code(kml_ctx *c) {
  const kml::LdpcCode &L = c->code;
  int regular = 1, irr_ok = 1;
  for (int j = 0; j < L.N; j++) {
    const int dv = L.col_ptr[j + 1] - L.col_ptr[j];
    if (dv != L.dv_max) regular = 0;
    if (dv < 1 || dv > 9) irr_ok = 0;
  }
  for (int i = 0; i < L.M; i++) {
    const int dc = L.row_ptr[i + 1] - L.row_ptr[i];
    if (dc != L.dc_max) regular = 0;
    if (dc < 2 || dc > 10) irr_ok = 0;
  }
  const int reg_T = kml::bp_regular_threads(L.N, L.M, L.E, L.dv_max, L.dc_max, regular);
  kml::RegularLayout plan;
  if (reg_T > 0) kml::plan_regular_layout(L, plan);
  const std::vector<int32_t> &vn_order = reg_T > 0 ? plan.order : L.vn_order;
  if (reg_T <= 0) {  // column -> vn position, used by the cooperative kernel
    plan.pos.assign(L.N, 0);
    for (int p = 0; p < L.N; p++) plan.pos[L.vn_order[p]] = p;
  }
  // partition plan of the partitioned cooperative kernel (codes whose slots exceed one CU's LDS)
  kml::PartitionPlan part;
  const int part_G = kml::bp_part_group_size(L.N, L.M, L.E, L.dv_max, L.dc_max, regular);
  if (part_G > 0 && !kml::plan_partition(L, part_G, part)) part.G = 0;
  if (part.G && getenv("KML_PLAN_VERBOSE"))
    fprintf(stderr, "partition plan: G %d, %d cut edges, mirrors <= %d, VN bank model cost %lld -> %lld\n", part.G,
            part.ncut, part.mirror_max, part.anneal_initial, part.anneal_final);
  int part_xmax = 0;
  for (int m = 0; part.G && m < part.G; m++)
    part_xmax = std::max({part_xmax, part.xr_ptr[m + 1] - part.xr_ptr[m], part.xc_ptr[m + 1] - part.xc_ptr[m]});
  if (part.G && !kml::part_plan_fits(part.G, L.N, L.M, L.E, part.ncut, part.mirror_max, part_xmax)) part.G = 0;
  // round plan of the irregular-code kernel (layout.hpp IrregularPlan)
  kml::IrregularPlan irr;
  if (!regular && !kml::plan_irregular(L, kml::kIrrThreads, kml::kIrrVnPairMax, kml::kIrrCnPairMax, irr))
    irr = kml::IrregularPlan();

  // all int32 arrays + the encoder words in one allocation
  GraphPacker g;
  const size_t row_ptr = g.add(L.row_ptr), row_col = g.add(L.row_col), col_ptr = g.add(L.col_ptr);
  const size_t col_slot = g.add(L.col_slot), vn_ord = g.add(vn_order), cn_ord = g.add(L.cn_order);
  const size_t enc_info = g.add(L.enc_info, 1);
  const size_t reg_c2v = g.add(plan.c2v_addr), reg_pos = g.add(plan.pos);
  const size_t pt_vn = g.add(part.vn), pt_cn = g.add(part.cn), pt_pos = g.add(part.pos), pt_vaddr = g.add(part.vaddr);
  const size_t pt_xr = g.add(part.xr), pt_xr_ptr = g.add(part.xr_ptr), pt_xc = g.add(part.xc);
  const size_t pt_xc_ptr = g.add(part.xc_ptr), pt_vx = g.add(part.vx), pt_rx = g.add(part.rx);
  const size_t irr_vn = g.add(irr.vn), irr_cn = g.add(irr.cn), irr_cn_base = g.add(irr.cn_base);
  const size_t irr_col_slot = g.add(irr.col_slot);
  HIPCHK(c, c->d_graph.ensure(g.host.size()), "hipMalloc(graph)");
  HIPCHK(c, hipMemcpy(c->d_graph.p, g.host.data(), g.host.size(), hipMemcpyHostToDevice), "upload graph");
  g.base = c->d_graph.as<unsigned char>();
  auto i32 = [&](size_t handle, bool present = true) { return present ? g.ptr<int32_t>(handle) : nullptr; };
  kml::DevCode &d = c->dc;
  d.row_ptr = i32(row_ptr);
  d.row_col = i32(row_col);
  d.col_ptr = i32(col_ptr);
  d.col_slot = i32(col_slot);
  d.vn_order = i32(vn_ord);
  d.cn_order = i32(cn_ord);
  d.enc_info = g.ptr<uint64_t>(enc_info);
  d.reg_c2v = i32(reg_c2v, reg_T > 0);
  d.reg_pos = i32(reg_pos);
  d.pt_G = part.G;
  d.pt_vn = i32(pt_vn, part.G);
  d.pt_cn = i32(pt_cn, part.G);
  d.pt_pos = i32(pt_pos, part.G);
  d.pt_vaddr = i32(pt_vaddr, part.G);
  d.pt_xr = i32(pt_xr, part.G);
  d.pt_xr_ptr = i32(pt_xr_ptr, part.G);
  d.pt_xc = i32(pt_xc, part.G);
  d.pt_xc_ptr = i32(pt_xc_ptr, part.G);
  d.pt_vx = i32(pt_vx, part.G);
  d.pt_rx = i32(pt_rx, part.G);
  d.irr_vn = i32(irr_vn, !irr.vn.empty());
  d.irr_cn = i32(irr_cn, !irr.cn.empty());
  d.irr_cn_base = i32(irr_cn_base, !irr.cn.empty());
  d.irr_col_slot = i32(irr_col_slot, !irr.cn.empty());
  d.irr_slots = irr.n_slots;
  d.pt_ncut = part.ncut;
  d.pt_mirror = part.mirror_max;
  d.pt_pairs = part.all_pairs ? 1 : 0;
  for (int m = 0; m < 8; m++) {
    d.pt_xr_n[m] = m < part.G ? part.xr_ptr[m + 1] - part.xr_ptr[m] : 0;
    d.pt_xc_n[m] = m < part.G ? part.xc_ptr[m + 1] - part.xc_ptr[m] : 0;
  }
  d.M = L.M;
  d.N = L.N;
  d.E = L.E;
  d.K = L.K;
  d.cc_len = L.cc_len;
  d.punct = L.punct;
  d.info_off = L.info_off;
  d.chk = L.chk;
  d.Kw = L.Kw;
  d.dv_max = L.dv_max;
  d.dc_max = L.dc_max;
  d.is5g = L.is5g ? 1 : 0;
  d.active = L.active ? 1 : 0;
  d.regular = regular;
  d.irr_ok = irr_ok;

  HIPCHK(c, c->d_cons.ensure(sizeof(double) * (c->modem.pts.size() + 8)), "hipMalloc(cons)");
  std::vector<double> cr(c->modem.pts);
  cr.insert(cr.end(), c->rot, c->rot + 8);
  HIPCHK(c, hipMemcpy(c->d_cons.p, cr.data(), sizeof(double) * cr.size(), hipMemcpyHostToDevice), "upload cons");
  HIPCHK(c, c->d_arena.ensure(sizeof(unsigned long long) * kml::CNT_N * kArenaSlots), "hipMalloc(counters)");
  HIPCHK(c, c->d_queue.ensure(256), "hipMalloc(queue)");
  const long long need = kml::bp_gslots_needed(d);
  if (need > 0) {
    HIPCHK(c, c->d_gslots.ensure((size_t)need * sizeof(double2)), "hipMalloc(gslots)");
    c->gslots_cap = need;
  }
  c->coop_groups = kml::bp_coop_groups(d);
  if (c->coop_groups > 0) {
    HIPCHK(c, c->d_gsync.ensure(kml::bp_coop_sync_bytes(c->coop_groups)), "hipMalloc(gsync)");
    // "no abort" from the start: run_bp marks a launch pending before it knows
    // its family, and one that lands on the generic bp_kernel (KML_BP_KERNEL=
    // generic, or the cooperative launcher declining) never writes the abort
    // word that sync() then reads
    HIPCHK(c, hipMemset(c->d_gsync.p, 0, kml::bp_coop_sync_bytes(c->coop_groups)), "memset(gsync)");
    HIPCHK(c, c->d_gcch.ensure((size_t)c->coop_groups * L.N), "hipMalloc(gcch)");
  }
  // layer plan of the layered min-sum kernel (layout.hpp LayeredPlan), in an
  // allocation of its own: it reaches the kernel beside DevCode, not in it
  bool planned = kml::bp_irregular_nms_supported(d);
  if (planned) {
    kml::plan_layered(L, c->layered);
  } else if (!regular && irr_ok) {  // a layered-only code?  (the gate needs the plan's pass count)
    kml::plan_layered(L, c->layered);
    planned = c->lnms_only = kml::bp_lnms_only_supported(d, (int)c->layered.pass.size());
    if (!planned) c->layered = kml::LayeredPlan();
  }
  if (planned) {
    const size_t bytes = c->layered.pass.size() * sizeof(int32_t);
    HIPCHK(c, c->d_lnms.ensure(bytes), "hipMalloc(layer plan)");
    HIPCHK(c, hipMemcpy(c->d_lnms.p, c->layered.pass.data(), bytes, hipMemcpyHostToDevice), "upload layer plan");
    c->lnms_dev.pass = c->d_lnms.as<int32_t>();
    c->lnms_dev.npass = (int)c->layered.pass.size();
    // ... and every lane's share of every pass, for the global-table instances
    std::vector<uint32_t> items;
    if (kml::layered_items(L, c->layered, items)) {
      HIPCHK(c, c->d_lnms_items.ensure(items.size() * sizeof(uint32_t)), "hipMalloc(layer items)");
      HIPCHK(c, hipMemcpy(c->d_lnms_items.p, items.data(), items.size() * sizeof(uint32_t), hipMemcpyHostToDevice),
             "upload layer items");
      c->lnms_items.item = c->d_lnms_items.as<uint2>();
    }
  }
  return KML_OK;
}

// The layer plan of a host-only context: bp_irregular_nms_supported and
// bp_lnms_only_supported restated on the host plan (no DevCode without a GPU),
// so kml_code_layers answers for the same codes with and without one.
void plan_layers_host(kml_ctx *c) {
  const kml::LdpcCode &L = c->code;
  bool regular = true, irr_ok = true;
  for (int j = 0; j < L.N; j++) {
    const int dv = L.col_ptr[j + 1] - L.col_ptr[j];
    regular &= dv == L.dv_max;
    irr_ok &= dv >= 1 && dv <= 9;
  }
  for (int i = 0; i < L.M; i++) {
    const int dc = L.row_ptr[i + 1] - L.row_ptr[i];
    regular &= dc == L.dc_max;
    irr_ok &= dc >= 2 && dc <= 10;
  }
  if (regular || !irr_ok) return;
  kml::plan_layered(L, c->layered);
  kml::IrregularPlan irr;
  bool nms_ok = kml::plan_irregular(L, kml::kIrrThreads, kml::kIrrVnPairMax, kml::kIrrCnPairMax, irr);
  if (nms_ok) {
    const size_t fixed = (size_t)L.E * 2 + 16 + (size_t)L.N;  // the slot table, the tallies, the decision bytes
    const size_t sibling = (size_t)irr.n_slots * 16 + (size_t)L.cc_len * 8 + fixed;
    const size_t nms = (size_t)irr.n_slots * 8 + (size_t)L.cc_len * 4 + fixed;
    nms_ok = irr.n_slots <= 16383 && sibling <= kml::kLdsLimit && nms <= kml::kLdsLimit;
  }
  if (nms_ok) return;
  // ... and bp_lnms_only_supported: the layered-only codes
  c->lnms_only = kml::lnms_only_shape_ok(L.N, L.M, L.E, (int)c->layered.pass.size());
  if (!c->lnms_only) c->layered = kml::LayeredPlan();
}

// FP64 work of one VN / CN phase of the exact algorithm: per column of degree
// d, 68d - 23 flops; per row of degree d, 73d - 52 flops (fma = 2, mul / add /
// sub / rcp = 1; each normalisation pair = one reciprocal refinement + two
// residual corrections, the minimal exact-IEEE sequence).
void phase_flops(kml_ctx *c) {
  const kml::LdpcCode &L = c->code;
  double v = 0, r = 0;
  for (int j = 0; j < L.N; j++) v += 68.0 * (L.col_ptr[j + 1] - L.col_ptr[j]) - 23.0;
  for (int i = 0; i < L.M; i++) r += 73.0 * (L.row_ptr[i + 1] - L.row_ptr[i]) - 52.0;
  c->vn_flops = v;
  c->cn_flops = r;
}
}  // namespace

int finish_create(kml_ctx *c) {
  std::string err;
  if (!c->code.load(c->rc.matrix_file, c->rc.is5g, c->rc.active, false, err)) return fail(c, KML_E_IO, err);
  phase_flops(c);
  if (!c->modem.load(c->rc.modem_file, err)) return fail(c, KML_E_IO, err);
  if (c->code.cc_len % c->modem.bits != 0)  // modemlinearsystem.cc:7-12
    return fail(c, KML_E_ARG, "(cc_len = " + std::to_string(c->code.cc_len) + ") % (input_len = " +
                                  std::to_string(c->modem.bits) + ") != 0");
  if (c->modem.bits != 1 && c->modem.bits != 2 && c->modem.bits != 3 && c->modem.bits != 4 && c->modem.bits != 6)
    return fail(c, KML_E_UNSUP, "bits per symbol must be 1, 2, 3, 4 or 6");
  kml::rotation_factors(c->rot);
  if (c->device < 0) {  // host-only context: planner + encoder, no GPU
    plan_layers_host(c);
    return KML_OK;
  }
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  HIPCHK(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking), "hipStreamCreate");
  return upload_code(c);
}

// The stream's work, the profile and the communicator go first, then the
// buffers (each DBuf frees itself with the context), then the streams.  A
// host-only or half-created context owns no stream and no allocation.
void destroy(kml_ctx *c) {
  const bool gpu = c->stream && c->device >= 0;
  const hipStream_t stream = c->stream, cstream = c->cstream;
  if (gpu) {
    hipSetDevice(c->device);
    hipStreamSynchronize(stream);
    drain_profile(c);
    kml::rccl_destroy(c->comm);
  }
  delete c;
  if (gpu) {
    hipStreamDestroy(stream);
    if (cstream) hipStreamDestroy(cstream);
  }
}

// ---- profiling
void drain_profile(kml_ctx *c) {
  if (c->pend.empty()) return;
  hipStreamSynchronize(c->stream);
  for (auto &p : c->pend) {
    float ms = 0;
    hipEventElapsedTime(&ms, p.ev0, p.ev1);
    Stat &s = c->stats[p.stage];
    s.launches++;
    s.ms += ms;
    double bytes = p.fixed_bytes;
    if (p.cnt_slot >= 0) {
      unsigned long long h[kml::CNT_N];
      hipMemcpy(h, slot_ptr(c, p.cnt_slot), sizeof(h), hipMemcpyDeviceToHost);
      const double E = c->code.E, N = c->code.N, vn = (double)h[kml::CNT_VN_PHASES], cn = (double)h[kml::CNT_CN_PHASES];
      bytes += vn * (24.0 * E + 9.0 * N) + cn * 24.0 * E;
      s.flops += vn * c->vn_flops + cn * c->cn_flops;
    }
    s.bytes += bytes;
    hipEventDestroy(p.ev0);
    hipEventDestroy(p.ev1);
  }
  c->pend.clear();
}

int fresh_slot(kml_ctx *c, int &slot) {
  slot = c->arena_next;
  c->arena_next = (c->arena_next + 1) % kArenaSlots;
  HIPCHK(c, hipMemsetAsync(slot_ptr(c, slot), 0, sizeof(unsigned long long) * kml::CNT_N, c->stream), "memset");
  return KML_OK;
}

int read_back(kml_ctx *c, const unsigned long long *cnt, uint64_t *counters, int n, bool add,
              std::initializer_list<D2H> more) {
  unsigned long long h[kml::CNT_N];
  HIPCHK(c, hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, c->stream), "D2H");
  for (const D2H &m : more)
    if (m.dst) HIPCHK(c, hipMemcpyAsync(m.dst, m.src, m.bytes, hipMemcpyDeviceToHost, c->stream), "D2H");
  TRY(sync(c));
  for (int i = 0; counters && i < n; i++) counters[i] = (add ? counters[i] : 0) + h[i];
  return KML_OK;
}

int run_bp(kml_ctx *c, kml::BpLaunch a, int *slot_out, int reuse, bool metric, const kml::LlrIoDev *llr) {
  if (llr && (metric || c->algorithm != KML_ALG_NMS))  // (callers check first: no fp64 kernel reads float priors)
    return fail(c, KML_E_UNSUP, "float LLR priors are decoded by the min-sum mode (KML_ALG_NMS) only");
  a.prec = metric ? KML_PREC_F64 : c->precision;
  if (!metric) TRY(schedule_refusal(c, "bp launch"));  // (the entry points ask first)
  kml::OmsDev oms;
  if (!metric && c->algorithm == KML_ALG_NMS) {  // (never with the f32 precision: kml_set_algorithm)
    if (a.syn) return fail(c, KML_E_UNSUP, "the min-sum decoder (KML_ALG_NMS) has no syndrom_soft: syn must be NULL");
    a.prec = c->schedule == KML_SCHED_LAYERED ? (c->messages == KML_MSG_F16 ? 4 : 3) : 2;
    a.nms_alpha = c->nms_alpha;
    oms.beta = c->nms_offset;  // (> 0 only in this mode: kml_set_nms_offset, kml_set_algorithm)
  }
  int slot = reuse;
  if (reuse < 0) TRY(fresh_slot(c, slot));
  a.counters = slot_ptr(c, slot);
  HIPCHK(c, c->w_defer.ensure(sizeof(int32_t) * ((size_t)a.B + 16)), "hipMalloc(defer list)");
  a.defer_idx = c->w_defer.as<int32_t>();
  a.defer_cnt = reinterpret_cast<unsigned *>(c->w_defer.as<int32_t>() + a.B);
  a.gslots = c->d_gslots.as<double2>();
  a.gslots_cap = c->gslots_cap;
  a.queue = c->d_queue.as<unsigned int>();
  a.gsync = c->d_gsync.p;
  a.gcch = c->d_gcch.as<uint8_t>();
  // the abort word is cleared only by the first cooperative launch after the
  // last sync(): a timeout in any launch before the check (e.g. chunk 0 of a
  // chunked host-buffer call) stays set until sync() reports it
  a.reset_abort = !c->coop_pending;
  if (c->coop_groups > 0) {
    if (!c->coop_this_call) c->coop_inherited = c->coop_pending;  // the call's first cooperative launch
    c->coop_pending = c->coop_this_call = true;
  }
  Timer t(c, "bp", slot, (double)a.B * 8.0 * c->code.cc_len);
  const char *msg = nullptr;
  hipError_t e = kml::launch_bp(c->dc, a, c->stream, &msg, &c->bp_family, &c->lnms_dev, llr,
                                oms.beta > 0.0f ? &oms : nullptr, &c->lnms_items);
  t.stop();
  if (e != hipSuccess) return msg ? fail(c, KML_E_UNSUP, msg) : hip_fail(c, e, "bp launch");
  if (c->inject_abort >= 0 && c->coop_groups > 0 && c->inject_abort-- == 0)  // as if a group barrier timed out
  {
    HIPCHK(c, kml::bp_coop_raise_abort(a, c->coop_groups, c->stream), "inject abort");
    if (c->inject_fail) {
      c->inject_fail = false;
      return fail(c, KML_E_HIP, "injected failure after a cooperative launch (kml_debug_inject_abort)");
    }
  }
  if (slot_out) *slot_out = slot;
  return KML_OK;
}

int demap_defer(kml_ctx *c, int need, kml::DemapDefer &d) {
  const int cap = std::max(need, 65536);
  HIPCHK(c, c->w_ddefer.ensure(sizeof(int32_t) * ((size_t)cap + 16)), "hipMalloc(demap defer list)");
  d.idx = c->w_ddefer.as<int32_t>();
  d.cnt = reinterpret_cast<unsigned *>(d.idx + cap);
  d.cap = cap;
  return KML_OK;
}

int run_demap(kml_ctx *c, const double2 *y, int reps, const double2 *h, int h_stride, const int32_t *h_sel, double var,
              int n, double *p0) {
  const int S = c->code.cc_len / c->modem.bits;
  Timer t(c, "demap", -1, (double)n * S * (16.0 + 8.0 * c->modem.bits));
  kml::DemapDefer dd;
  TRY(demap_defer(c, 0, dd));
  HIPCHK(c, kml::launch_demap(c->modem.bits, c->d_cons.as<double>(), y, S, reps, h, h_stride, h_sel, var, n, p0, dd,
                              c->stream),
         "demap");
  t.stop();
  return KML_OK;
}

int run_demap_llr(kml_ctx *c, const double2 *y, int reps, const double2 *h, int h_stride, const int32_t *h_sel,
                  double var, int n, float *llr) {
  const int S = c->code.cc_len / c->modem.bits;
  Timer t(c, "demap", -1, (double)n * S * (16.0 + 4.0 * c->modem.bits));
  HIPCHK(c, kml::launch_demap_llr(c->modem.bits, c->d_cons.as<double>(), y, S, reps, h, h_stride, h_sel,
                                  (float)(1.0 / var), n, llr, c->stream),
         "demap_llr");
  t.stop();
  return KML_OK;
}

int run_kmeans(kml_ctx *c, const double2 *y, int iters, int B, double2 *h_hat, double2 *h4, double2 *hat_out) {
  const int S = c->code.cc_len / c->modem.bits;
  const double *cons = c->d_cons.as<double>();
  HIPCHK(c, c->w_km.ensure(kml::kmeans_workspace_bytes(S, B)), "hipMalloc(kmeans)");
  Timer t(c, "kmeans", -1, (double)B * S * 16.0);
  HIPCHK(c, kml::launch_kmeans(c->modem.Kc, cons, cons + c->modem.pts.size(), y, S, iters, B, h_hat, h4, c->w_km.p,
                               c->stream, hat_out),
         "kmeans");
  t.stop();
  return KML_OK;
}

int sync(kml_ctx *c) {
  HIPCHK(c, hipStreamSynchronize(c->stream), "hipStreamSynchronize");
  if (c->coop_pending) {
    c->coop_pending = false;
    unsigned why = 0;
    if (coop_aborted(c, &why)) {
      static const char *const site[] = {"raised by the host", "group barrier", "v2c mailbox poll", "c2v mailbox poll",
                                         "early-stop flag poll"};
      const unsigned k = why >> 24;
      return fail(c, KML_E_HIP,
                  std::string("cooperative BP kernel aborted: ") + (k == 0 ? "" : "timed out at ") + (k < 5 ? site[k] : "?") +
                      (why ? ", workgroup " + std::to_string(why & 0xFFFFFFu) : std::string()));
    }
  }
  return KML_OK;
}

}  // namespace kml_host
