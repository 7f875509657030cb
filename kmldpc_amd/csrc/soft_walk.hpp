// soft_walk.hpp — the host walk of the soft syndrome metric (kmcodec.cc:145-156
// with metric_type = true), free of HIP so it runs on the CPU
// (tests/native/soft_walk_check.cpp).
//
// syndrom_soft is the reference codec's member array and is only rewritten when
// a CN phase runs, so a candidate whose decode stops at iteration 0 reads the
// array left by the most recent decode that did run one — an earlier candidate,
// the previous codeword's final decode, ... — a sequential dependency across
// the batch.  Only the sum of logs of that array matters, so the state is one
// scalar (-inf = the never-written, zero array).  The candidates' decodes and
// sums run batched on the GPU; this walk takes their iteration counts and log
// sums and resolves the stale reads in codeword order.  A codeword's final
// decode can be skipped in the walk whenever it provably repeats its chosen
// candidate's metric decode (same trajectory up to the shorter iteration cap);
// otherwise the walk stops at the first codeword whose choice needs it, hands
// out what is resolved so far (one round), and resumes once that final
// decode's (iters, L) is fed back: one extra round per such link.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace kml {

struct __attribute__((visibility("hidden"))) SoftWalk {  // internal to the library: not an exported type
  const int B, nc, metric_iter, max_iter;
  const int32_t *const itm;  // [B][nc] iterations of the candidates' metric decodes
  const double *const Lm;    // [B][nc] their sums of log(syndrom_soft)
  // Reset rule: in the simulator (sim) the reference's codec is copied per task
  // of thread_block_number codewords, so the state restarts at global indices
  // that are multiples of it (and at the batch start).
  const bool sim;
  const uint64_t first_cw, task;
  double state;                 // incoming; after the walk, the state the batch leaves
  std::vector<int32_t> chosen;  // [B]
  std::vector<double> met;      // [B][4], entries >= nc stay 0
  std::vector<int32_t> list;    // codewords whose choice is known, in decode order

  SoftWalk(int B_, int nc_, int metric_iter_, int max_iter_, const int32_t *itm_, const double *Lm_, double state_in,
           bool sim_, uint64_t first_cw_, long long thread_block_number)
      : B(B_), nc(nc_), metric_iter(metric_iter_), max_iter(max_iter_), itm(itm_), Lm(Lm_), sim(sim_),
        first_cw(first_cw_), task((uint64_t)(thread_block_number > 1 ? thread_block_number : 1)),
        state(sim_ ? -INFINITY : state_in), chosen(B_, 0), met((size_t)4 * B_, 0.0) {
    list.reserve(B_);
  }

  // GetHistogramData: metric decodes only, so no final decode ever sets the state.
  void metrics_only() {
    for (int b = 0; b < B; b++) {
      if (reset_at(b)) state = -INFINITY;
      state = metrics_of(b, state);
    }
  }

  bool done() const { return cursor >= B; }

  // One round: list[first, first + n) are the codewords to decode now.  feedback
  // >= 0 names the last of them: its final decode does not repeat its metric
  // decode, so feed() its (iters, L) before the next round (or before reading
  // `state`).
  struct Round {
    size_t first;
    int n, feedback;
  };
  Round next() {
    const size_t first = list.size();
    bool unknown = false;  // the state hangs on the final decode of `pend`
    int b = cursor;
    for (; b < B; b++) {
      if (reset_at(b)) {
        state = -INFINITY;
        unknown = false;
      }
      const bool stale_first = itm[(size_t)b * nc] <= 0;
      if (stale_first && unknown) break;  // needs the pending final decode
      const double cur = metrics_of(b, unknown ? 0.0 : state);
      list.push_back(b);
      const int mc = itm[(size_t)b * nc + chosen[b]];
      // the final decode repeats the chosen candidate's metric decode when
      // both stop at the same iteration: converged before both caps, or equal caps
      const bool same = (mc < metric_iter && mc <= max_iter) || metric_iter == max_iter;
      if (same) {
        state = mc > 0 ? Lm[(size_t)b * nc + chosen[b]] : cur;
        unknown = false;
      } else {
        unknown = true;
        pend = b;
        pend_cur = cur;
      }
    }
    cursor = b;
    return {first, (int)(list.size() - first), unknown ? pend : -1};
  }
  void feed(int32_t iters, double L) { state = iters > 0 ? L : pend_cur; }

 private:
  int cursor = 0, pend = -1;
  double pend_cur = 0.0;
  bool reset_at(int b) const { return sim && (b == 0 || (first_cw + (uint64_t)b) % task == 0); }
  // candidates of codeword b against the incoming state; returns the state after them
  double metrics_of(int b, double in) {
    double cur = in;
    for (int i = 0; i < nc; i++) {
      const size_t e = (size_t)b * nc + i;
      if (itm[e] > 0) cur = Lm[e];
      met[(size_t)b * 4 + i] = std::fabs(cur);
    }
    int best = 0;
    for (int i = 1; i < nc; i++)
      if (met[(size_t)b * 4 + i] < met[(size_t)b * 4 + best]) best = i;
    chosen[b] = best;
    return cur;
  }
};

}  // namespace kml
