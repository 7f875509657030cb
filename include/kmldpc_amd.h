/* kmldpc_amd.h — C ABI of the MI355X-native kmldpc hot path.
 *
 * Drop-in boundary for the per-codeword receive loop of trganda/kmldpc
 * (paths relative to /root/reference/kmldpc).  The reference has no FFI; its
 * boundary is a set of C++ classes.  Each entry point below replaces one of
 * them, batched over B codewords:
 *
 *   kml_create                lab::BinaryLDPCCodec(const toml::value&)            lib/lab/include/binaryldpccodec.h:16
 *                             lab::Binary5GLDPCCodec(const toml::value&)           lib/lab/include/binary5gldpccodec.h:12
 *                             lab::Modem(const toml::value&)                       lib/lab/include/modem.h:13
 *                             KmCodec(toml::value)                                 include/kmcodec.h:16
 *   kml_bp_decode             virtual int BinaryLDPCCodec::Decoder(const double *M2V, int *uu_hat, int iter_count)
 *                                                                                  lib/lab/include/binaryldpccodec.h:20
 *                                                                                  (override binary5gldpccodec.h:17)
 *   kml_demap                 void ModemLinearSystem::DeMapping(thetaList, double *bitLin, double *bitLout)
 *                                                                                  lib/lab/include/modemlinearsystem.h:20-22
 *   kml_kmeans                kmldpc::KMeans(data, constellations, iter); Run(); clusters()
 *                                                                                  include/kmeans.h:14-22
 *                             + h_hat = clusters[0]/c[0] and its 4 rotations       src/simulator.cc:145-148
 *   kml_kmeans_state          KMeans::clusters(), KMeans::idx() after Run()          include/kmeans.h:18-19
 *                                                                                  (src/kmeans.cc:72-83, 86-94)
 *   kml_kmeans_dump_mat       void KMeans::DumpToMat(std::string&, std::vector<complex>& append)
 *                                                                                  include/kmeans.h:21, src/kmeans.cc:99-109
 *                             (host only; the reference needs matio, this writes the level-5 file itself)
 *   kml_decode_frames         void KmCodec::Decoder(ModemLinearSystem&, const std::vector<complex>& h_hats, int *uu_hat)
 *                                                                                  include/kmcodec.h:23-25
 *   kml_decode_candidates     the same KmCodec::Decoder with the caller's h_hats (any 1..4 estimates)
 *                                                                                  include/kmcodec.h:23-25
 *   kml_count_errors          void SourceSink::CntErr(const int*, const int*, int, int)  lib/lab/include/sourcesink.h:15
 *   kml_sim_*                 the throughput driver: frame generation + receive + counting for one
 *                             SNR point of Simulator::run_blocks (src/simulator.cc:112-168)
 *   kml_sim_decode_profile    no counterpart: the reference answers "BER / FER at iteration budget k" with
 *                             one run per [ldpc] max_iter = k.  In BinaryLDPCCodec::Decoder iter_count only
 *                             bounds the loop (lib/lab/src/binaryldpccodec.cc:175-277; the 5G override
 *                             likewise), so one decode with budget P holds every budget's answer; this
 *                             entry point returns all P of them from one receive of the resident batch.
 *
 * Conventions
 *   - Every call returns 0 on success or a negative KML_E* code and never exits
 *     the process (the reference logs and exit(-1)s).  kml_last_error() holds
 *     the message of the last failure on that context (with a NULL context: the
 *     last failure of a context-free call, kml_comm_unique_id, on this thread).
 *   - Bits (uu, uu_hat, cc_hat) are one byte per bit (0/1) unless a name says
 *     "_bits" (packed little-endian uint64 words).  Complex numbers are
 *     interleaved (re, im) doubles.
 *   - Pointers are host pointers unless KML_DEVICE_PTRS is set in `flags`, in
 *     which case they must be device pointers on the context's GPU; results are
 *     complete when the call returns (the context's HIP stream is synchronised).
 *   - A context is bound to one GPU and one HIP stream and is not thread-safe;
 *     use one context per GPU / per thread.
 */
#ifndef KMLDPC_AMD_H
#define KMLDPC_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KML_ABI_VERSION 2  /* 2: KML_DIM_PART_G (KML_DIM_COUNT 13) */

enum {
  KML_OK = 0,
  KML_E_ARG = -1,    /* bad argument */
  KML_E_IO = -2,     /* cannot open / parse a config, H-matrix or constellation file */
  KML_E_HIP = -3,    /* HIP runtime failure */
  KML_E_UNSUP = -4,  /* configuration not supported */
  KML_E_NOMEM = -5
};

enum {
  KML_DEVICE_PTRS = 1,
  /* kml_decode_frames: KmCodec::GetHistogramData instead of Decoder — the
   * candidate metrics only, no final decode; uu_hat is what the last metric
   * decode left (BP-based metrics) or zeros (hard PEG metric). */
  KML_HISTOGRAM = 2
};

typedef struct kml_ctx kml_ctx;

/* dims[]: index names for kml_dims */
enum {
  KML_DIM_M = 0,        /* check rows */
  KML_DIM_NCOL = 1,     /* internal columns (incl. punctured) */
  KML_DIM_K = 2,        /* info bits (code_dim) */
  KML_DIM_CCLEN = 3,    /* transmitted bits */
  KML_DIM_Z = 4,        /* 5G lifting factor */
  KML_DIM_E = 5,        /* edges */
  KML_DIM_CHK = 6,      /* GF(2) rank (code_chk) */
  KML_DIM_MAXITER = 7,  /* [ldpc] max_iter */
  KML_DIM_BITS = 8,     /* bits per symbol */
  KML_DIM_KC = 9,       /* constellation points */
  KML_DIM_S = 10,       /* symbols per codeword */
  KML_DIM_BP_LDS = 11,  /* 1 if the decoder keeps messages in LDS */
  KML_DIM_PART_G = 12,  /* workgroups per codeword of the partitioned decoder (4), 0 when not used */
  KML_DIM_COUNT = 13
};

/* Create a context from a reference config.toml.  Relative matrix_file /
 * modem_file paths are resolved against data_dir (NULL or "" = the CWD, as
 * the reference does).  device = HIP device ordinal; device < 0 creates a
 * host-only context (planner, encoder, constellation; no GPU calls). */
int kml_create(const char *config_toml, const char *data_dir, int device, kml_ctx **out);
/* Same without a config file: the [ldpc]/[modem]/[xcodec] keys given directly. */
int kml_create_explicit(const char *matrix_file, const char *modem_file, int is5g, int active, int max_iter,
                        int metric_soft, int metric_iter, int device, kml_ctx **out);
void kml_destroy(kml_ctx *ctx);
const char *kml_last_error(const kml_ctx *ctx);
int kml_abi_version(void);
/* Name of the BP kernel family the context last launched ("bp_regular_kernel",
 * "bp_irregular_kernel", "bp_part_kernel" (the partitioned cooperative kernel,
 * PEG8064), "bp_kernel"; "" before any decode). */
const char *kml_bp_kernel(const kml_ctx *ctx);

/* Arithmetic of the BP decoder, per context.  KML_PREC_F64 (the default) is the
 * bit-exact restatement of the reference.  KML_PREC_F32 is an opt-in
 * single-precision decoder for Monte-Carlo BER / FER work ("bp_regular_f32_kernel"
 * in kml_bp_kernel): the same schedule, stop rule and return value with float
 * messages and hardware reciprocals.  It is NOT bit-exact with the reference
 * and promises no particular bit of uu_hat, ret, cc_hat or syn.  What it does
 * guarantee, and the test suite checks against the reference arithmetic on
 * seed-17 streams (QPSK at 2 dB, 16QAM at 8 dB, 64QAM at 13 dB): at most 2 % of
 * the codewords differ in uu_hat, in ret or in cc_hat; a call's results do not
 * depend on the batch size or on the codeword's place in the batch and repeat
 * from call to call; the fused and the separate demap paths agree bit for bit
 * within the mode.  The mode changes the final BP decode of kml_bp_decode,
 * kml_decode_frames, kml_decode_candidates, kml_sim_decode(_ex) and
 * kml_sim_point only: the demapper, k-means and the candidate metrics (chosen,
 * metrics, h_hat) stay fp64 and unchanged, and syn is still double (float
 * values widened).  The soft-syndrome metric (metric_type = 1), whose
 * candidates' metrics depend on earlier final decodes, returns KML_E_UNSUP
 * in the f32 mode.
 * kml_set_precision returns KML_E_UNSUP, and leaves the context in fp64, when
 * the context's code does not take the f32 kernel (only PEG2304-class codes do:
 * regular, dv 3, dc 6, N = 2304, M = 1152) or the context is host-only, and
 * KML_E_ARG for an unknown value.  There is no fallback in either direction. */
enum { KML_PREC_F64 = 0, KML_PREC_F32 = 1 };
int kml_set_precision(kml_ctx *ctx, int prec);
int kml_get_precision(const kml_ctx *ctx);

/* Decoding algorithm of the final BP decodes, per context.  KML_ALG_SPA (the
 * default) is the reference's sum-product decoder, bit-exact; it is always
 * accepted and alpha is ignored.  KML_ALG_NMS is an opt-in normalized min-sum
 * decoder for the codes that take bp_irregular_kernel (5G BG2 K960 and other
 * irregular codes whose messages fit in LDS; "bp_irregular_nms_kernel" in
 * kml_bp_kernel).  It is a different decoder: its results are NOT the
 * reference's.  What is fixed instead is its arithmetic, which
 * tests/bp_nms_model.py restates in numpy and the kernel equals bit for bit
 * (uu_hat, ret, cc_hat).  Every value is IEEE binary32 with denormals kept, no
 * fma, each operation rounded once:
 *   prior     q = min(max(P0, 1e-12), 1 - 1e-12) in fp64,
 *             L = (float)(log(q) - log(1 - q)) (fp64 logs and subtraction);
 *             a punctured 5G column has L = +0; messages start at +0;
 *   VN phase  column v, edges in column order (kml_code_graph's col_ptr /
 *             col_slot): t = L; t = t + c2v_k for every k in order; T = t;
 *             decision T > 0 ? 0 : 1 (a tie decides 1);
 *             v2c_k = clamp(T - c2v_k, -256.0f, 256.0f);
 *   stop      after the VN phase, when every check row's decisions have even
 *             parity, before the CN phase; ret = iter + (iter < max_iter);
 *             iter_count = 0 leaves uu_hat / cc_hat as passed;
 *   CN phase  row with incoming m_j: a_j = min over i != j of |m_i|,
 *             s_j = XOR over i != j of the IEEE sign bits of m_i (-0 counts as
 *             negative), c2v_j = RN(alpha * a_j) with its sign bit set to s_j.
 * alpha is the normalisation factor: 0 selects the default 0.75, otherwise
 * 0 < alpha <= 1, rounded once to float (1 is plain min-sum); any other value,
 * NaN included, and an unknown alg return KML_E_ARG.
 * The scope is that of kml_set_precision: the final decode of kml_bp_decode,
 * kml_decode_frames, kml_decode_candidates, kml_sim_decode(_ex) and
 * kml_sim_point; k-means, the demapper and the candidate metrics (BG2's
 * metric_iter decodes included) stay fp64 sum-product, so chosen, metrics and
 * h_hat are bit-identical in both algorithms.  CNT_REDONE stays 0;
 * kml_prof_read_flops keeps applying the sum-product rule and is not
 * meaningful in this mode.
 * Layered-only codes.  An irregular code with column degrees in [1, 9] and row
 * degrees in [2, 10] that does NOT take bp_irregular_kernel (no round plan:
 * N > 2304, e.g. the BG2 structure at Z > 96) is accepted too when E <= 65535,
 * M <= 65535, N < 65535 and its posteriors and messages fit one CU's LDS
 * (4 N + 4 E + N bytes and the pass words within 160 KiB: BG2 at R = 1/2 up to
 * Z = 384, K = 3840).  Such a code has the layered decoders only (below):
 * kml_set_algorithm(KML_ALG_NMS) succeeds and leaves the schedule at flooding,
 * and until kml_set_schedule(KML_SCHED_LAYERED) every decode entry point
 * (kml_bp_decode, kml_llr_decode, kml_decode_frames, kml_decode_candidates,
 * kml_sim_decode(_ex), kml_sim_point) returns KML_E_UNSUP before anything is
 * launched, the demapper and k-means included; kml_last_error names the
 * schedule setter and the context keeps its state.  Under the exact demapper
 * such a code's candidate metric decodes are the generic bp_kernel's.
 * KML_E_UNSUP, with the context's algorithm unchanged: a host-only context, a
 * code that takes neither bp_irregular_kernel nor the rule above (regular
 * codes: PEG2304, PEG8064; degrees outside the ranges; codes whose posteriors
 * and messages exceed one CU), a context in the f32 precision (a guard: no code
 * takes both kernels), and KML_BP_KERNEL=generic.  In NMS mode a non-NULL
 * syn (min-sum has no syndrom_soft), the soft-syndrome metric (metric_type =
 * 1) and kml_sim_decode_profile return KML_E_UNSUP before anything is
 * launched.  There is no fallback in either direction. */
enum { KML_ALG_SPA = 0, KML_ALG_NMS = 1 };
int kml_set_algorithm(kml_ctx *ctx, int alg, double alpha);
int kml_get_algorithm(const kml_ctx *ctx, double *alpha /* may be NULL */);

/* Row schedule of the min-sum decodes, per context: a third axis beside
 * precision and algorithm.  KML_SCHED_FLOODING (the default) is the decoder
 * above: one VN phase over all columns, then one CN phase over all rows.
 * KML_SCHED_LAYERED is the schedule a 5G receiver runs
 * ("bp_irregular_lnms_kernel" in kml_bp_kernel): one posterior per column, the
 * rows taken in index order, each reading what the rows before it left.  It
 * reaches the flooding schedule's error rate in about half the iterations.
 * Its arithmetic is tests/bp_lnms_model.py's, which the kernel equals bit for
 * bit (uu_hat, ret, cc_hat).  Priors, alpha, the +-256 clamp, the tie rule and
 * the number format are the flooding decoder's (above):
 *   state     T[v] = L[v], one posterior per column; c2v[e] = +0, one message
 *             per edge in row-major order;
 *   loop      hard = (T > 0 ? 0 : 1); it = 0; then, repeatedly: when every
 *             check row of hard has even parity, stop (converged); when
 *             it == iter_count, stop; otherwise one sweep, it += 1,
 *             hard = (T > 0 ? 0 : 1);
 *   sweep     rows r = 0 .. M-1 in index order; for each edge j of r (column
 *             v_j): m_j = clamp(T[v_j] - c2v_j, -256.0f, 256.0f); then
 *             a_j = min over i != j of |m_i|, s_j = XOR over i != j of the
 *             IEEE sign bits of m_i (-0 counts as negative),
 *             c2v_j = RN(alpha * a_j) with its sign bit set to s_j, and
 *             T[v_j] = m_j + c2v_j;
 *   result    ret = it + (it < max_iter); uu_hat / cc_hat are hard;
 *             iter_count = 0 leaves them as passed.
 * A budget of k uses all k sweeps: the decisions are those of the posteriors
 * the k-th sweep left.  (The flooding schedule never reads its last CN phase;
 * the difference is deliberate.)  Counters: `it` CN phases, it + 1 (converged)
 * or it VN phases; CNT_REDONE stays 0.
 * A layer is a maximal run of consecutive rows with pairwise disjoint columns,
 * found greedily in row order: a row that shares a column with the open layer
 * closes it and opens the next.  Its rows touch disjoint T and c2v entries, so
 * the kernel works on them in parallel and still computes the serial sweep:
 * layers are a matter of speed, not of the arithmetic.  kml_code_layers returns
 * the number of layers nl and writes min(cap, nl + 1) entries of layer_ptr
 * (layer l = rows [layer_ptr[l], layer_ptr[l + 1])); it works on a host-only
 * context and answers KML_E_UNSUP for a code the min-sum mode does not take
 * (5G BG2 K960: 12 layers of 96 rows; the layered-only codes of
 * kml_set_algorithm are taken: BG2's structure at Z = 384 has 12 layers of 384
 * rows).
 * Where the code tables (the column of every edge, the row pointers) fit in
 * LDS beside the decoder state, the kernel stages them there; otherwise, or
 * with KML_LNMS_TABLES=global in the environment (read once per process), it
 * runs the global-table instances, which read every lane's share of a pass
 * from a table in global memory ("bp_irregular_lnms_gt_kernel" /
 * "bp_irregular_lnms_h16_gt_kernel" in kml_bp_kernel).  Both compute the same.
 * The schedule belongs to the min-sum mode.  KML_SCHED_FLOODING is always
 * accepted (on a layered-only code the decode entry points then answer
 * KML_E_UNSUP, see kml_set_algorithm).  KML_SCHED_LAYERED returns KML_E_UNSUP, and the context keeps its
 * schedule, on a host-only context, on a context whose algorithm is not
 * KML_ALG_NMS, and with KML_BP_KERNEL=generic; an unknown value returns
 * KML_E_ARG.  kml_set_algorithm(KML_ALG_SPA) returns the schedule to flooding;
 * kml_set_algorithm(KML_ALG_NMS, alpha) keeps it.  The scope and the refusals
 * (syn, the soft-syndrome metric, kml_sim_decode_profile) are those of
 * kml_set_algorithm.  There is no fallback to another kernel. */
#define KML_SCHED_FLOODING 0
#define KML_SCHED_LAYERED 1
int kml_set_schedule(kml_ctx *ctx, int sched);
int kml_get_schedule(const kml_ctx *ctx);
int kml_code_layers(const kml_ctx *ctx, int32_t *layer_ptr, int cap);

/* The LLR front end of the min-sum mode: a max-log demapper that writes float
 * LLRs, min-sum decodes that take float LLRs and can return posteriors, and a
 * per-context switch, a fourth axis beside precision, algorithm and schedule,
 * that puts both on the receive path.  Like the min-sum mode it is a different
 * receiver from the reference's: it is held to tests/bp_llr_model.py, which the
 * kernels equal bit for bit, not to the reference.
 * Max-log demapper (kml_demap_llr, kmldpc_amd/csrc/demap_llr.hip).  Every value
 * is IEEE binary32 with denormals kept (the code object's float_denorm_mode_32
 * is 3), no fma, each operation rounded once.  Rounded once to float on the way
 * in: y[s] and h (fp64 in the interface), the normalised constellation points
 * x_k (kml_constellation) and inv = (float)(1.0 / var), the division in fp64.
 * Per symbol s and point k:
 *   gr = hr*xr_k - hi*xi_k, gi = hr*xi_k + hi*xr_k, er = yr - gr, ei = yi - gi,
 *   d_k = er*er + ei*ei;
 * for bit i of the symbol (the label's bits most significant first, kml_demap's
 * order: bit i of point k is (k >> (bits - 1 - i)) & 1)
 *   L = (min over k with bit_i(k) = 1 of d_k - min over k with bit_i(k) = 0 of d_k) * inv
 * at entry s*bits + i of the codeword, where kml_demap writes that bit's P0.
 * Positive means bit 0, as log(P0 / P1) does.  No clamp and no clip: the output
 * is the raw LLR.  kml_demap_llr works in any algorithm and on any code;
 * KML_E_UNSUP on a host-only context, KML_E_ARG for a NULL pointer, B < 0 or a
 * var that is not > 0.
 * LLR-in decode (kml_llr_decode): llr[B][cc_len] floats.  The two min-sum
 * contracts above with one change, the prior: L[v] = min(max(x, -256.0f),
 * 256.0f) of the caller's float (+-inf and +-1e30 are +-256; a punctured 5G
 * column has L = +0 as before).  A NaN is the caller's error: that codeword's
 * result is unspecified, no other codeword's is.  For any P0, decoding the
 * priors of the P0 contract through this entry equals kml_bp_decode of that P0
 * bit for bit (|L| <= 27.7 there: the clamp does nothing).  Schedule and alpha
 * are the context's; uu_hat, ret, cc_hat as in kml_bp_decode (any may be NULL).
 * llr_out[B][Ncol] (optional, punctured columns included) receives the
 * posteriors the returned decisions were taken from, as bit patterns (-0 and +0
 * differ): in the flooding schedule the T of the VN phase whose decisions are
 * returned, in the layered schedule T as the loop left it; iter_count = 0
 * leaves it as passed.  KML_E_UNSUP: a host-only context, a context not in
 * KML_ALG_NMS (so every code the min-sum mode refuses), and, for llr_out in the
 * flooding schedule only, a code whose N more floats of LDS do not fit.
 * The switch (kml_set_demapper).  KML_DEMAP_EXACT (the default, always
 * accepted): every path runs what it ran before.  KML_DEMAP_MAXLOG: in
 * kml_decode_frames, kml_decode_candidates, kml_sim_decode(_ex) and
 * kml_sim_point the final decode demaps with the max-log demapper and decodes
 * from its LLRs, on the known-channel and the blind path; for a 5G code the
 * candidate metric decodes run the context's min-sum decoder too (its alpha and
 * schedule, budget metric_iter) on the max-log LLRs of the candidates, the
 * metric being the unsatisfied checks of the decisions returned.  So under the
 * switch chosen and metrics of a 5G code are a min-sum receiver's, not the
 * reference's.  For a non-5G code the hard metric on the exact demapper's
 * output stays: chosen and metrics are bit-identical to the exact mode's and
 * only the final decode's priors change.  k-means (h_hat) is untouched on every
 * path; kml_demap and kml_bp_decode do not read the switch.
 * KML_DEMAP_MAXLOG returns KML_E_UNSUP, and the context keeps its value, on a
 * host-only context, on a context whose algorithm is not KML_ALG_NMS, and with
 * KML_BP_KERNEL=generic; an unknown value returns KML_E_ARG.
 * kml_set_algorithm(KML_ALG_SPA) returns the demapper to exact;
 * kml_set_algorithm(KML_ALG_NMS, alpha) and kml_set_schedule keep it.  The
 * min-sum mode's refusals (syn, the soft-syndrome metric,
 * kml_sim_decode_profile) hold as they are.  There is no fallback. */
#define KML_DEMAP_EXACT 0
#define KML_DEMAP_MAXLOG 1
int kml_set_demapper(kml_ctx *ctx, int demapper);
int kml_get_demapper(const kml_ctx *ctx);
int kml_demap_llr(kml_ctx *ctx, const double *y, const double *h, double var, int B, float *llr, int flags);
int kml_llr_decode(kml_ctx *ctx, const float *llr, int B, int iter_count, uint8_t *uu_hat, int32_t *ret,
                   uint8_t *cc_hat, float *llr_out, int flags);

/* The message format of the layered min-sum decoder, a fifth axis beside
 * precision, algorithm, schedule and demapper.  KML_MSG_F32 (the default,
 * always accepted): every path runs what it ran before.  KML_MSG_F16 sends
 * every layered min-sum decode of the context to bp_irregular_lnms_h16_kernel
 * (kmldpc_amd/csrc/bp_irregular_lnms_h16.hip), which keeps the decoder state in
 * IEEE binary16 and decodes two codewords in the two halves of every 32-bit
 * word.  It is held to tests/bp_h16_model.py, which the kernel equals bit for
 * bit.
 * The arithmetic contract is KML_SCHED_LAYERED's above with one change: every
 * value of the decoder state is IEEE binary16, denormals kept, no fma, each
 * operation rounded once to nearest-even.
 *   - Prior: the float L of the existing contract rounded once to binary16: in
 *     the P0 front end L = (float)(log q - log(1 - q)), in the LLR front end
 *     L = min(max(x, -256.0f), 256.0f); a punctured column has +0.
 *   - alpha: a16 = RN16((float)alpha), to float first and then to half (0.75,
 *     0.8125 and 1 are exact).
 *   - Sweep, the same four steps, each one binary16 operation:
 *     m_j = clamp(T[v_j] - c2v_j, -256, 256); the magnitudes compared as the
 *     unsigned integers their 15-bit patterns are; c2v_j = RN16(a16 * a_j) with
 *     its sign bit set to s_j; T[v_j] = m_j + c2v_j.
 *   - Decisions (T > 0 ? 0 : 1, a tie decides 1), the stop rule (a budget of k
 *     uses all k sweeps), ret = it + (it < max_iter) and iter_count = 0 (outputs
 *     as passed) are unchanged.
 *   - llr_out of kml_llr_decode is the binary16 T widened to float, which is
 *     exact; bit patterns, -0 and +0 differ.
 * A codeword's result does not depend on the codeword it shares its words with,
 * nor on the batch size or its place in the batch; ret, iters, the per-codeword
 * outputs and the counters are each codeword's own, as the f32 kernel reports
 * them.
 * Scope: that of kml_set_schedule plus the LLR entry: the final decode of
 * kml_bp_decode, kml_decode_frames, kml_decode_candidates, kml_sim_decode(_ex)
 * and kml_sim_point; kml_llr_decode with llr_out; under KML_DEMAP_MAXLOG a 5G
 * code's candidate metric decodes.  k-means, both demappers and the exact front
 * end's fp64 candidate metrics are untouched.
 * KML_MSG_F16 returns KML_E_UNSUP, and the context keeps its value, on a
 * host-only context, with KML_BP_KERNEL=generic, and on a context that is not in
 * KML_ALG_NMS and KML_SCHED_LAYERED (the flooding schedule has no binary16
 * kernel).  KML_E_ARG: an unknown value; KML_MSG_F16 when the context's alpha
 * rounds to +0 in binary16 (alpha <= 2^-25); and, in the F16 format,
 * kml_set_algorithm(KML_ALG_NMS, alpha) with such an alpha, the context left
 * unchanged.  kml_set_algorithm(KML_ALG_SPA) and
 * kml_set_schedule(KML_SCHED_FLOODING) return the format to F32;
 * kml_set_algorithm(KML_ALG_NMS, alpha), kml_set_schedule(KML_SCHED_LAYERED)
 * and kml_set_demapper keep it.  The min-sum mode's refusals (syn, the
 * soft-syndrome metric, kml_sim_decode_profile) hold as they are.  There is no
 * fallback. */
#define KML_MSG_F32 0
#define KML_MSG_F16 1
int kml_set_messages(kml_ctx *ctx, int fmt);
int kml_get_messages(const kml_ctx *ctx);

/* The offset correction of the min-sum check-node rule, a sixth axis beside
 * precision, algorithm, schedule, demapper and message format.  beta = 0 (the
 * default, always accepted, on host-only contexts too): every path runs what it
 * ran before, on the kernel instances it ran before.  beta > 0 sends every
 * min-sum decode of the context (flooding, layered, layered binary16) to the
 * offset instances of its kernel; kml_bp_kernel keeps naming the three families.
 * They are held to tests/bp_oms_model.py, which they equal bit for bit.
 * The arithmetic contract is that of the context's min-sum decoder with two
 * more operations in every check-node update.  Flooding and layered f32 (IEEE
 * binary32, denormals kept, no fma), b = (float)beta:
 *     c = RN(alpha * a_j);  c = RN(c - b), one rounding;  c = c > 0 ? c : +0;
 *     then the sign bit of c is set to s_j, exactly as without the offset.
 * Layered binary16: the same in binary16 with b16 = RN16((float)beta): a packed
 * multiply, a packed subtract, a packed max with +0.  No -0 reaches the max:
 * x - x is +0 in round-to-nearest and alpha * a_j is never negative, so the
 * operand of the max is positive, negative or +0.
 *   - A message of magnitude zero with its sign bit set (-0) is legal and is
 *     covered by the existing rules: -0 counts as negative in the sign XOR of
 *     m, and m + (-0) = m.
 *   - Priors, the +-256 clamp, the tie rule, the stop rule, ret and the counters
 *     are unchanged.
 * Scope: wherever the context's min-sum decoder runs, a 5G code's candidate
 * metric decodes under KML_DEMAP_MAXLOG included; under the exact demapper those
 * metric decodes stay fp64 sum-product.
 * KML_E_ARG: beta negative, NaN, infinite or > 256; a positive beta that rounds
 * to +0 in float; in the F16 format a positive beta that rounds to +0 in
 * binary16 (beta <= 2^-25), and kml_set_messages(KML_MSG_F16) when the
 * context's beta does.  beta > 0 returns KML_E_UNSUP, and the context keeps its
 * value, on a host-only context, on a context that is not in KML_ALG_NMS, and
 * with KML_BP_KERNEL=generic.  kml_set_algorithm(KML_ALG_SPA) returns the offset
 * to 0; kml_set_algorithm(KML_ALG_NMS, alpha), kml_set_schedule,
 * kml_set_demapper and kml_set_messages keep it.  The min-sum mode's refusals
 * (syn, the soft-syndrome metric, kml_sim_decode_profile) hold as they are.
 * There is no fallback.  KML_ABI_VERSION stays 2. */
int kml_set_nms_offset(kml_ctx *ctx, double beta);
int kml_get_nms_offset(const kml_ctx *ctx, double *beta);

int kml_dims(const kml_ctx *ctx, int32_t *dims /* [KML_DIM_COUNT] */);
/* Host-side code plan, for inspection and parity tests. */
int kml_code_perm(const kml_ctx *ctx, int32_t *perm /* [Ncol] */);
int kml_code_graph(const kml_ctx *ctx, int32_t *row_ptr /* [M+1] */, int32_t *row_col /* [E] */,
                   int32_t *col_ptr /* [Ncol+1] */, int32_t *col_slot /* [E] */);
int kml_constellation(const kml_ctx *ctx, double *points /* [2*Kc] */);
/* Host encoder (BinaryLDPCCodec::Encoder), uu[K] -> cc[cc_len], bytes. */
int kml_encode(const kml_ctx *ctx, const uint8_t *uu, uint8_t *cc, int B);

/* BinaryLDPCCodec::Decoder, batched.  p0[B][cc_len] = P(bit = 0) (the
 * reference's M2V).  Outputs (any may be NULL): uu_hat[B][K], ret[B] (the
 * reference return value iter + (iter < max_iter)), cc_hat[B][Ncol],
 * syn[B][M] (syndrom_soft; rows are only written when a CN phase runs, like
 * the reference's member array).  iter_count = 0 runs no iteration and, like
 * the reference (uu_hat is written inside its loop), leaves uu_hat and cc_hat
 * as the caller passed them. */
int kml_bp_decode(kml_ctx *ctx, const double *p0, int B, int iter_count, uint8_t *uu_hat, int32_t *ret,
                  uint8_t *cc_hat, double *syn, int flags);

/* ModemLinearSystem::DeMapping with bitLin = 0.5 and one channel estimate per
 * codeword: y[B][S][2], h[B][2], var = 10^(-snr/10) -> p0[B][cc_len]. */
int kml_demap(kml_ctx *ctx, const double *y, const double *h, double var, int B, double *p0, int flags);

/* KMeans(y, constellation, iters).Run(); h_hat = clusters[0]/c[0];
 * h4[j] = h_hat * exp(i*kPi/2*j).  h_hat[B][2], h4[B][4][2] (either may be NULL). */
int kml_kmeans(kml_ctx *ctx, const double *y, int B, int iters, double *h_hat, double *h4, int flags);

/* The same Run, then KMeans::clusters() = c[k] * hatH -> clusters[B][Kc][2] and
 * KMeans::idx() (the closing assignment, first minimum of glibc hypot,
 * kmeans.cc:76-83) -> idx[B][S].  Either output may be NULL. */
int kml_kmeans_state(kml_ctx *ctx, const double *y, int B, int iters, double *clusters, int32_t *idx, int flags);

/* KMeans::DumpToMat(filename, append) of ONE codeword (host only, no context):
 * a MAT-file level 5 with the reference's variables, each an n x 1 column,
 * uncompressed as lab::Mat writes them (lib/lab/src/mat.cc): data[S] complex,
 * cluster[Kc] complex, idx[S] int32, constellations[Kc] complex, hHats =
 * append[0..3] complex, realH = append[4] (1 x 1 complex).  Complex inputs
 * are interleaved (re, im); append holds 5 complex values.  Returns 0,
 * KML_E_ARG or KML_E_IO. */
int kml_kmeans_dump_mat(const char *path, const double *data, int S, const double *clusters, const int32_t *idx,
                        const double *constellations, int Kc, const double *append);

/* KmCodec::Decoder for B codewords at Es/N0 = snr dB.  true_h[B][2] selects
 * the known-channel path ([decoder] true_h_arg = true); true_h == NULL runs the
 * blind path (k-means, 4 candidates, syndrome metric).  Optional outputs:
 * chosen[B], metrics[B][4], ret[B], h_hat[B][2]. */
int kml_decode_frames(kml_ctx *ctx, const double *y, const double *true_h, double snr, int B, uint8_t *uu_hat,
                      int32_t *chosen, double *metrics, int32_t *ret, double *h_hat, int flags);

/* KmCodec::Decoder(mls, h_hats, uu_hat) (include/kmcodec.h:23-25,
 * src/kmcodec.cc:54-72) with the caller's channel estimates h_hats[B][nc][2],
 * 1 <= nc <= 4: nc == 1 demaps with h_hats[b][0] and decodes (no metric);
 * nc > 1 computes every candidate's syndrome metric (hard PEG count, 5G
 * metric_iter BP count, or the soft metric, as configured), takes the first
 * minimum, demaps with it and decodes.  chosen[B], metrics[B][4] (entries
 * >= nc are 0), ret[B] may be NULL.  KML_HISTOGRAM: metrics only
 * (KmCodec::GetHistogramData, kmcodec.cc:75-79), for nc == 1 too: the single
 * candidate's metric, no final decode, ret zeroed. */
int kml_decode_candidates(kml_ctx *ctx, const double *y, const double *h_hats, int nc, double snr, int B,
                          uint8_t *uu_hat, int32_t *chosen, double *metrics, int32_t *ret, int flags);

/* SourceSink::CntErr over B codewords; counters[4] += {err_bit, err_blk, tot_bit, tot_blk}. */
int kml_count_errors(kml_ctx *ctx, const uint8_t *uu, const uint8_t *uu_hat, int B, uint64_t *counters, int flags);

/* --- throughput driver (GPU-resident frames) ----------------------------- */
/* Generate B frames for codeword indices [first_cw, first_cw + B) at Es/N0 =
 * snr into the context's resident buffers (Philox stream keyed by seed). */
int kml_sim_generate(kml_ctx *ctx, double snr, uint64_t seed, uint64_t first_cw, int B);
/* Receive the resident batch (blind or known-H) and accumulate the counters.
 * counters[8] (may be NULL) receives {err_bit, err_blk, tot_bit, tot_blk,
 * vn_phases, cn_phases, converged, redone} of this call (redone: codewords a
 * FAST kernel deferred mid-decode to the exact kernel.  Unproven FAST
 * quotients are settled in place (exact_div.hpp dd_fix), so this is 0 unless
 * KML_FORCE_REDO=1 forces the path; see DESIGN.md "Bit-exactness strategy").  If sync == 0 the call
 * returns after enqueueing the work (counters must then be NULL); use
 * kml_sync to wait. */
int kml_sim_decode(kml_ctx *ctx, double snr, int blind, uint64_t *counters, int sync);
int kml_sync(kml_ctx *ctx);
/* Synchronous form with the per-codeword view the simulator's stop rule needs:
 * cw_err[B] (may be NULL) = error bits of each resident codeword, metrics[B][4]
 * (may be NULL) = the candidate metrics.  histogram != 0 runs
 * KmCodec::GetHistogramData instead of Decoder (simulator.cc:154-162): metrics
 * only, no final decode, and the error count then sees the uu_hat the last
 * metric decode left (5G metric) or all-zero decisions (hard PEG metric, whose
 * reference buffer is uninitialised).  counters[8] as kml_sim_decode. */
int kml_sim_decode_ex(kml_ctx *ctx, double snr, int blind, int histogram, int32_t *cw_err, double *metrics,
                      uint64_t *counters);
/* The resident batch received once (as kml_sim_decode_ex does, blind or known-H) with the
 * context's max_iter = P; for every iteration budget k = 1..P what a context created with
 * [ldpc] max_iter = k would count on the same frames:
 *   prof[P][3]   = {err_bit, err_blk, converged} at budget k (row k-1); may be NULL
 *   cw_prof[B][P] = error bits of each codeword at budget k;            may be NULL
 *   counters[8]  as kml_sim_decode (row P-1 of prof equals its err_bit / err_blk / converged).
 * A codeword whose parity check first passes at iteration c returns, at budget k, the
 * decisions of iteration min(k-1, c), and counts as converged when c <= k-1; the kernels
 * count the info-bit errors of every iteration's decisions while they decode.  Only the
 * final decode is profiled: the blind path's candidate metrics run as in kml_sim_decode.
 * An empty resident batch zeroes the outputs and returns 0.
 * KML_E_UNSUP (kml_last_error names the reason): a host-only context; the f32 mode;
 * a context with the soft-syndrome metric (metric_type = 1); codes that take
 * bp_part_kernel (PEG8064) or the generic bp_kernel, KML_BP_KERNEL=generic included;
 * max_iter > 64.  KML_E_ARG: a NULL context, max_iter < 1.  Nothing is launched by a
 * refused call and there is no fallback to another kernel.  Profiles for the f32 and the
 * partitioned kernels are follow-ups; so is a profile truncated by the sweep driver's
 * stop rule (kml_sweep_point / kml_sim_point are unchanged). */
int kml_sim_decode_profile(kml_ctx *ctx, double snr, int blind, uint64_t *prof, int32_t *cw_prof, uint64_t *counters);

/* --- simulator driver (Simulator::Simulate / run / run_blocks) ------------ */
/* The parsed config.toml: f[3] = {minimum_snr, maximum_snr, step_snr};
 * n[10] = {maximum_error_number, maximum_block_number, thread_block_number,
 * true_h_arg, 5gldpc, metric_type, metric_iter, histogram.enable, max_iter,
 * active}. */
int kml_run_config(const kml_ctx *ctx, double *f, int64_t *n);

/* In-place sum of n counters over all ranks (RCCL / gloo / MPI in the caller). */
typedef int (*kml_allreduce_fn)(uint64_t *vals, int n, void *user);
/* Decode `count` frames with global codeword indices [first_cw, first_cw+count):
 * cw_err[count] error bits per codeword, metrics[count][4] (histogram mode). */
typedef int (*kml_batch_fn)(uint64_t first_cw, int count, int32_t *cw_err, double *metrics, void *user);
/* Progress: counters {err_bit, err_blk, tot_bit, tot_blk} (SourceSink::PrintResult). */
typedef void (*kml_report_fn)(const uint64_t *counters, void *user);

typedef struct {
  double snr;
  int rank, world;       /* this process's shard of the codeword index space */
  int batch;             /* codewords per rank per round */
  uint64_t max_blocks;   /* maximum_block_number */
  uint64_t max_err;      /* maximum_error_number */
  int K;                 /* info bits per codeword (tot_bit += K) */
  int ncand;             /* histogram: metrics per codeword (1 known-H, 4 blind) */
  const char *hist_path; /* histogram output file of this rank, NULL = none */
  int report_every;      /* PrintResult period in codewords (reference: 100) */
} kml_point_cfg;

/* One SNR point of Simulator::run with the stop rule of run_blocks
 * (simulator.cc:117): codewords are taken in global index order until
 * maximum_block_number are counted or maximum_error_number block errors
 * reached, exactly as a single sequential stream would, whatever world and
 * batch are.  Rank r decodes indices [t*world*batch + r*batch, ...) of round t;
 * per round the ranks exchange world + 4 counters through `reduce` (no
 * per-codeword data moves between ranks).  counters[4] = the point's totals
 * {err_bit, err_blk, tot_bit, tot_blk}. */
int kml_sweep_point(const kml_point_cfg *cfg, kml_batch_fn decode, void *decode_user, kml_allreduce_fn reduce,
                    void *reduce_user, kml_report_fn report, void *report_user, uint64_t *counters);
/* kml_sweep_point with the context's GPU frame generator (Philox keyed by
 * seed and global codeword index) and receive path ([decoder] true_h_arg,
 * [histogram] enable from the config). */
int kml_sim_point(kml_ctx *ctx, const kml_point_cfg *cfg, uint64_t seed, kml_allreduce_fn reduce, void *reduce_user,
                  kml_report_fn report, void *report_user, uint64_t *counters);
/* Load B host frames (uu[B][K] source-bit bytes, y[B][S][2], true h[B][2])
 * into the resident batch in place of kml_sim_generate, e.g. the reference's
 * own seed-17 stream from kml_ref_frames, so kml_sim_decode's counters can be
 * compared with SourceSink::CntErr's (sourcesink.cc:29-47) on identical frames. */
int kml_sim_load(kml_ctx *ctx, double snr, const uint8_t *uu, const double *y, const double *h, int B,
                 uint64_t first_cw);
/* Copy the resident frames out (for checks): uu[B][K] bytes, y[B][S][2], h[B][2]. */
int kml_sim_frames(kml_ctx *ctx, uint8_t *uu, double *y, double *h);

/* --- multi-GPU counter reduction: RCCL over xGMI ------------------------- */
/* The reference sums its worker threads' counters under a mutex
 * (lib/lab/src/threadsafe_sourcesink.cc); across GPUs that is one RCCL
 * all-reduce, issued by this library on the context's stream.  Rank 0 calls
 * kml_comm_unique_id, the caller distributes the 128 bytes (any CPU channel,
 * e.g. torch.distributed gloo), and every rank calls kml_comm_init (a
 * collective).  librccl.so.1 is loaded on first use. */
#define KML_COMM_ID_BYTES 128
int kml_comm_unique_id(uint8_t *id /* [KML_COMM_ID_BYTES] */);
int kml_comm_init(kml_ctx *ctx, const uint8_t *id, int world, int rank);
/* Ranks of the context's communicator (0 = none). */
int kml_comm_size(const kml_ctx *ctx);
/* In-place sum over the ranks of n host values (staged through the GPU;
 * synchronous). */
int kml_comm_allreduce_u64(kml_ctx *ctx, uint64_t *vals, int n);
int kml_comm_allreduce_f64(kml_ctx *ctx, double *vals, int n);

/* --- the reference's host random sources (parity runs) ------------------ */
/* lab::CLCRandNum (randnum.cc:4-92): Park-Miller minimal standard with
 * Schrage's method; *state = 17 is SetSeed(-1).  Normal(): polar method. */
double kml_lcg_uniform(int64_t *state);
void kml_lcg_normal(int64_t *state, double *nn, int len);
/* lab::CWHRandNum (randnum.cc:95-166): Wichmann-Hill; xyz = {13, 37, 91} is SetSeed(-1). */
double kml_wh_uniform(int32_t *xyz);
void kml_wh_normal(int32_t *xyz, double *nn, int len);
/* lab::SourceSink::GetBitStr / GetSymStr (sourcesink.cc:5-19) on a CLCRandNum state. */
void kml_get_bit_str(int64_t *state, uint8_t *uu, int len);
void kml_get_sym_str(int64_t *state, int32_t *uu, int qary, int len);
/* n frames of Simulator::run_blocks' sequential stream (simulator.cc:118-130)
 * from a CLCRandNum state (advanced in place): uu[n][K] bytes, true_h[n][2],
 * y[n][S][2].  Host-side; also works on a host-only context. */
int kml_ref_frames(const kml_ctx *ctx, int64_t *state, double snr, int n, uint8_t *uu, double *true_h, double *y);

/* --- profiling ----------------------------------------------------------- */
/* When enabled, every kernel launch of the context is bracketed by HIP events
 * on the context's stream.  kml_prof_read returns, for the named stage
 * ("bp", "demap", "kmeans", "metric", "framegen"), the number of launches,
 * their summed device time in ms and the summed algorithmic bytes
 * (SURVEY §8d accounting for "bp"). */
int kml_prof_enable(kml_ctx *ctx, int on);
int kml_prof_reset(kml_ctx *ctx);
int kml_prof_read(kml_ctx *ctx, const char *stage, int64_t *launches, double *total_ms, double *alg_bytes);
/* Summed algorithmic fp64 flops of the stage's launches ("bp" only). */
int kml_prof_read_flops(kml_ctx *ctx, const char *stage, double *alg_flops);

/* Device-side probe of the exact-math helpers: in[n][4] = (a, b, c, d) ->
 * out[n][4] = (hypot(a,b), re((a+ib)/(c+id)), im(...), exp(a)) with the
 * glibc-exact restatements the kernels use. */
int kml_math_probe(kml_ctx *ctx, const double *in, int n, double *out);
/* Device-side probe of the soft metric's log (kml_log, glibc-exact): out[i] = log(in[i]). */
int kml_log_probe(kml_ctx *ctx, const double *in, int n, double *out);
/* Device-side probe of the decoder's divisions (exact_div.hpp, bp_common.hpp):
 * in[n][3] = (n0, n1, s) -> out[n][12] = (FAST VN quotients n0/s, n1/s
 * (dd_quot), div_rn n0/s, n1/s (correctly rounded, any operands), the CN
 * phase's near-one quotients n0/s, n1/s, the near-one reciprocal formula of s,
 * hipcc's refined reciprocal of s, hipcc's '/' n0/s, n1/s, flags: bit 0 / 1 =
 * dd_check could not prove the FAST quotient of n0 / n1, bit 2 = div2's
 * suspect flag, |1 - s v_rcp_f64(s)|: the hardware reciprocal's error). */
int kml_div_probe(kml_ctx *ctx, const double *in, int n, double *out);
/* Test hook: after the nth (0-based) cooperative BP launch from now, set that
 * kernel's abort word as a timed-out group barrier would (nth < 0: off).  The
 * call that owns the launch must then fail with KML_E_HIP, even when later
 * launches of the same call (chunks of a host-buffer decode) follow it.
 * nth = -2: raise the abort after the next cooperative launch AND fail that
 * call at once, before its sync (the error-return path: the next call must
 * start clean, not inherit the abort). */
int kml_debug_inject_abort(kml_ctx *ctx, int nth);

#ifdef __cplusplus
}
#endif
#endif
