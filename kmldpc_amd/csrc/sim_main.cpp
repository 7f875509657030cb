// sim_main.cpp — `kmldpc_sim`, the drop-in for the reference executable
// (kmldpc/kmldpc.cpp): reads config.toml (or argv[1]), runs the SNR sweep of
// Simulator::Simulate (src/simulator.cc:24-67) on one GPU through the C ABI, and
// prints the reference's console lines (timestamped [INFO] records, per-point
// progress every 100 blocks, the BER / FER result tables, total time), teeing
// them to logs/<time>-kmldpc.logger when a logs/ directory exists.
//
// Differences, by design: the SNR points run one after another on the GPU
// (the reference runs them on concurrent threads, interleaving their progress
// lines); frames come from the counter-based GPU generator, so the numbers are
// statistically, not bitwise, equal to a reference run (bitwise parity of the
// receive path is established on the reference's own frames, tests/); the
// per-codeword debug records the reference writes only to the log file
// ("Generated H", "Hhat = ... Metric", "hatIndex") are not produced.
//
// Environment: KML_DEVICE (GPU ordinal, default 0), KML_BATCH (codewords per
// GPU round, default 32768), KML_SEED (frame seed, default 0 like
// CLCRandNum::SetSeed(0) in kmldpc.cpp:22), KML_PRECISION (f64 or f32, also
// `--precision f64|f32` on the command line: the BP decode arithmetic,
// kml_set_precision; an f32 run states the mode in its first line),
// KML_ALGORITHM (spa, nms or nms:alpha, also `--algorithm spa|nms[:alpha]`: the
// decoder of the final BP decodes, kml_set_algorithm; an nms run states the
// mode in its first line), KML_SCHEDULE (flooding or layered, also
// `--schedule flooding|layered`: the row schedule of the min-sum decodes,
// kml_set_schedule; layered needs nms and states itself in the line after the
// algorithm's), KML_DEMAPPER (exact or maxlog, also `--demapper exact|maxlog`:
// the front end of the min-sum receive path, kml_set_demapper; maxlog needs nms
// and states itself in the line after the schedule's), KML_MESSAGES (f32 or f16,
// also `--messages f32|f16`: the message format of the layered min-sum decodes,
// kml_set_messages; f16 needs nms and layered and states itself in the line
// after the demapper's), KML_OFFSET (a number in [0, 256], also `--offset B`:
// the offset correction of the min-sum check-node rule, kml_set_nms_offset; a
// B above 0 needs nms and states itself in the line after the message
// format's; an unparsable or out-of-range B is a usage error, exit status 2).
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <sys/stat.h>
#include <vector>

#include "../../include/kmldpc_amd.h"

namespace {

FILE *g_log = nullptr;

std::string now_string() {  // Log::get_time (log.cc:77-87)
  std::time_t t = std::time(nullptr);
  char buf[50] = {0};
  strftime(buf, sizeof buf, "%Y-%m-%d %H:%M:%S", localtime(&t));
  return buf;
}

void emit(const char *tag, const std::string &msg) {
  const std::string line = "[" + now_string() + "]" + tag + msg + "\n";
  fputs(line.c_str(), stdout);
  fflush(stdout);
  if (g_log) {
    fputs(line.c_str(), g_log);
    fflush(g_log);
  }
}
void info(const std::string &m) { emit(" \x1b[32;1m[INFO]\x1b[0m ", m); }
void error(const std::string &m) { emit(" \x1b[31;1m[ERROR]\x1b[0m ", m); }

std::string fmt(const char *f, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

// SourceSink::PrintResult (sourcesink.cc:50-65): zero-filled width-7 counters,
// 14-digit BER / FER.
void print_result(double snr, const uint64_t *c) {
  const double ber = c[2] ? (double)c[0] / (double)c[2] : 0.0;
  const double fer = c[3] ? (double)c[1] / (double)c[3] : 0.0;
  info(fmt("SNR = %03.3f Total blk = %07llu Error blk = %07llu Error bit = %07llu BER = %.14f FER = %.14f", snr,
           (unsigned long long)c[3], (unsigned long long)c[1], (unsigned long long)c[0], ber, fer));
}

struct Progress {
  double snr;
};
void on_progress(const uint64_t *c, void *user) { print_result(static_cast<Progress *>(user)->snr, c); }

std::string dir_of(const std::string &p) {
  const size_t k = p.find_last_of('/');
  return k == std::string::npos ? std::string(".") : p.substr(0, k);
}

// std::to_string(double) == "%f"
std::string hist_name(double snr) { return "histogram_" + fmt("%f", snr) + ".txt"; }

}  // namespace

int main(int argc, char **argv) {
  const auto begin = std::chrono::steady_clock::now();
  struct stat st;
  if (stat("logs", &st) == 0 && S_ISDIR(st.st_mode)) {
    const std::string name = "logs/" + now_string() + "-kmldpc.logger";
    g_log = fopen(name.c_str(), "w");
  }
  std::string cfg = "config.toml", prec = getenv("KML_PRECISION") ? getenv("KML_PRECISION") : "f64";
  std::string alg = getenv("KML_ALGORITHM") ? getenv("KML_ALGORITHM") : "spa";
  std::string sched = getenv("KML_SCHEDULE") ? getenv("KML_SCHEDULE") : "flooding";
  std::string demapper = getenv("KML_DEMAPPER") ? getenv("KML_DEMAPPER") : "exact";
  std::string messages = getenv("KML_MESSAGES") ? getenv("KML_MESSAGES") : "f32";
  std::string offset = getenv("KML_OFFSET") ? getenv("KML_OFFSET") : "0";
  for (int i = 1; i < argc; i++) {
    const std::string arg = argv[i];
    if (arg == "--precision" && i + 1 < argc)
      prec = argv[++i];
    else if (arg.rfind("--precision=", 0) == 0)
      prec = arg.substr(12);
    else if (arg == "--algorithm" && i + 1 < argc)
      alg = argv[++i];
    else if (arg.rfind("--algorithm=", 0) == 0)
      alg = arg.substr(12);
    else if (arg == "--schedule" && i + 1 < argc)
      sched = argv[++i];
    else if (arg.rfind("--schedule=", 0) == 0)
      sched = arg.substr(11);
    else if (arg == "--demapper" && i + 1 < argc)
      demapper = argv[++i];
    else if (arg.rfind("--demapper=", 0) == 0)
      demapper = arg.substr(11);
    else if (arg == "--messages" && i + 1 < argc)
      messages = argv[++i];
    else if (arg.rfind("--messages=", 0) == 0)
      messages = arg.substr(11);
    else if (arg == "--offset" && i + 1 < argc)
      offset = argv[++i];
    else if (arg.rfind("--offset=", 0) == 0)
      offset = arg.substr(9);
    else
      cfg = arg;
  }
  if (prec != "f64" && prec != "f32") {
    error("--precision / KML_PRECISION must be f64 or f32");
    return 255;
  }
  // spa | nms | nms:alpha (alpha = 0: the library's default, 0.75)
  double alpha = 0.0;
  bool alg_ok = alg == "spa" || alg == "nms";
  if (alg.rfind("nms:", 0) == 0 && alg.size() > 4) {
    char *end = nullptr;
    alpha = strtod(alg.c_str() + 4, &end);
    alg_ok = *end == '\0' && alpha > 0.0 && alpha <= 1.0;
    alg = "nms";
  }
  if (!alg_ok) {
    error("--algorithm / KML_ALGORITHM must be spa, nms or nms:alpha with 0 < alpha <= 1");
    return 255;
  }
  if (sched != "flooding" && sched != "layered") {
    error("--schedule / KML_SCHEDULE must be flooding or layered");
    return 255;
  }
  if (sched == "layered" && alg != "nms") {
    error("--schedule layered needs --algorithm nms: the schedule belongs to the min-sum mode");
    return 255;
  }
  if (demapper != "exact" && demapper != "maxlog") {
    error("--demapper / KML_DEMAPPER must be exact or maxlog");
    return 255;
  }
  if (demapper == "maxlog" && alg != "nms") {
    error("--demapper maxlog needs --algorithm nms: the max-log front end belongs to the min-sum mode");
    return 255;
  }
  if (messages != "f32" && messages != "f16") {
    error("--messages / KML_MESSAGES must be f32 or f16");
    return 255;
  }
  if (messages == "f16" && !(alg == "nms" && sched == "layered")) {
    error("--messages f16 needs --algorithm nms --schedule layered: the binary16 format belongs to the layered "
          "min-sum decoder");
    return 255;
  }
  double beta = 0.0;
  {
    char *end = nullptr;
    beta = strtod(offset.c_str(), &end);
    if (offset.empty() || *end != '\0' || !(beta >= 0.0 && beta <= 256.0)) {  // (NaN included)
      error("--offset / KML_OFFSET must be a number in [0, 256]");
      return 2;
    }
    if (beta > 0.0 && alg != "nms") {
      error("--offset needs --algorithm nms: the offset correction belongs to the min-sum mode");
      return 2;
    }
  }
  if (prec == "f32") info("BP decode precision: f32 (single precision, not bit-exact with the reference)");
  if (alg == "nms")
    info(fmt("BP decode algorithm: nms (normalized min-sum, alpha = %g; not the reference's decoder)",
             alpha > 0.0 ? (double)(float)alpha : 0.75));
  if (sched == "layered") info("BP decode schedule: layered");
  if (demapper == "maxlog") info("Demapper: maxlog (max-log LLR front end; not the reference's demapper)");
  if (messages == "f16") info("BP message format: f16 (binary16 decoder state; two codewords a workgroup)");
  if (beta != 0.0) info(fmt("BP min-sum offset: %g", (double)(float)beta));
  info("Start simulation");
  {
    FILE *f = fopen(cfg.c_str(), "rb");
    if (!f) {
      error("Encouter error while opening config.toml");  // kmldpc.cpp:36 (sic)
      info("Simulation done");
      return 0;
    }
    fclose(f);
  }
  const int device = getenv("KML_DEVICE") ? atoi(getenv("KML_DEVICE")) : 0;
  const int batch = getenv("KML_BATCH") ? atoi(getenv("KML_BATCH")) : 32768;
  const uint64_t seed = getenv("KML_SEED") ? strtoull(getenv("KML_SEED"), nullptr, 10) : 0;
  kml_ctx *ctx = nullptr;
  if (kml_create(cfg.c_str(), dir_of(cfg).c_str(), device, &ctx) != KML_OK) {
    error(ctx ? kml_last_error(ctx) : "kml_create failed");
    kml_destroy(ctx);
    return 255;  // the reference exits with -1 on setup errors
  }
  if (prec == "f32" && kml_set_precision(ctx, KML_PREC_F32) != KML_OK) {
    error(kml_last_error(ctx));
    kml_destroy(ctx);
    return 255;
  }
  if (alg == "nms" && kml_set_algorithm(ctx, KML_ALG_NMS, alpha) != KML_OK) {
    error(kml_last_error(ctx));
    kml_destroy(ctx);
    return 255;
  }
  if (sched == "layered" && kml_set_schedule(ctx, KML_SCHED_LAYERED) != KML_OK) {
    error(kml_last_error(ctx));
    kml_destroy(ctx);
    return 255;
  }
  if (demapper == "maxlog" && kml_set_demapper(ctx, KML_DEMAP_MAXLOG) != KML_OK) {
    error(kml_last_error(ctx));
    kml_destroy(ctx);
    return 255;
  }
  if (messages == "f16" && kml_set_messages(ctx, KML_MSG_F16) != KML_OK) {
    error(kml_last_error(ctx));
    kml_destroy(ctx);
    return 255;
  }
  if (beta != 0.0 && kml_set_nms_offset(ctx, beta) != KML_OK) {
    error(kml_last_error(ctx));
    kml_destroy(ctx);
    return 255;
  }
  double f[3];
  int64_t n[10];
  kml_run_config(ctx, f, n);
  const double min_snr = f[0], max_snr = f[1], step_snr = f[2];
  info(n[4] ? "Using 5G LDPC." : "Using traditional LDPC.");  // kmcodec.cc:27,32
  info(fmt("[%.3f,%.3f,%.3f]", min_snr, step_snr, max_snr));  // simulator.cc:16-18
  info(fmt("[MAX_ERROR_BLK = %lld,MAX_BLK = %lld]", (long long)n[0], (long long)n[1]));
  const unsigned long points = (unsigned long)((max_snr - min_snr) / step_snr + 1);
  std::vector<double> snrs, ber, fer;
  int rc = KML_OK;
  for (unsigned long i = 0; i < points && rc == KML_OK; i++) {
    const double snr = min_snr + step_snr * i;
    kml_point_cfg pc{};
    pc.snr = snr;
    pc.rank = 0;
    pc.world = 1;
    pc.batch = batch > 0 ? batch : 32768;
    pc.max_blocks = n[1] > 0 ? (uint64_t)n[1] : 0;
    pc.max_err = n[0] > 0 ? (uint64_t)n[0] : 0;
    pc.report_every = 100;
    const std::string hist = hist_name(snr);
    pc.hist_path = n[7] ? hist.c_str() : nullptr;
    Progress pr{snr};
    uint64_t c[4] = {0, 0, 0, 0};
    const uint64_t point_seed = seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)(i + 1));
    rc = kml_sim_point(ctx, &pc, point_seed, nullptr, nullptr, on_progress, &pr, c);
    if (rc != KML_OK) {
      error(kml_last_error(ctx));
      break;
    }
    print_result(snr, c);  // Simulator::run's final PrintResult
    snrs.push_back(snr);
    ber.push_back(c[2] ? (double)c[0] / (double)c[2] : 0.0);
    fer.push_back(c[3] ? (double)c[1] / (double)c[3] : 0.0);
  }
  if (rc == KML_OK) {
    info("BER Result");
    for (size_t i = 0; i < snrs.size(); i++) info(fmt("%03.3f %.14f", snrs[i], ber[i]));
    info("FER Result");
    for (size_t i = 0; i < snrs.size(); i++) info(fmt("%03.3f %.14f", snrs[i], fer[i]));
  }
  kml_destroy(ctx);
  info("Simulation done");
  const auto end = std::chrono::steady_clock::now();
  long long ms = std::chrono::duration_cast<std::chrono::milliseconds>(end - begin).count();
  const long long mins = ms / 60000, secs = ms / 1000 - mins * 60;
  ms -= mins * 60 * 1000;
  info(fmt("Total time cost: %lldmin:%lldsec:%lldms", mins, secs, ms));
  if (g_log) fclose(g_log);
  return rc == KML_OK ? 0 : 1;
}
