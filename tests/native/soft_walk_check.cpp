// soft_walk_check.cpp — kml::SoftWalk (kmldpc_amd/csrc/soft_walk.hpp) against a
// naive model that walks the codewords one by one, the way KmCodec::Decoder
// does: every candidate's metric decode, the choice, then the final decode,
// with syndrom_soft_ (here: the sum of its logs) carried from decode to decode.
//
// The final decode is synthetic, final(b, chosen): whenever it provably repeats
// the chosen candidate's metric decode it returns exactly that candidate's
// (iters, L); otherwise an arbitrary pair drawn from the case's seed.  The walk
// sees a final decode only through feed(), the model sees all of them.
//
//   soft_walk_check [cases]     prints "soft_walk_errors=<n>", exit status 1 if n > 0
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "soft_walk.hpp"

namespace {

uint64_t mix(uint64_t x) {  // splitmix64
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

struct Rng {
  uint64_t s;
  uint64_t next() { return s = mix(s); }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

struct Case {
  int B, nc, mit, max_iter;
  bool sim;
  uint64_t first_cw;
  long long task;
  double state_in;
  uint64_t seed;
  std::vector<int32_t> itm;
  std::vector<double> Lm;
  int nvalues;  // distinct log sums to draw from (few = ties)

  double value(uint64_t r) const { return -0.5 - (double)(r % (uint64_t)nvalues) * 0.375; }
  bool repeats(int b, int ch) const {
    const int mc = itm[(size_t)b * nc + ch];
    return (mc < mit && mc <= max_iter) || mit == max_iter;
  }
  void final(int b, int ch, int32_t &iters, double &L) const {
    if (repeats(b, ch)) {
      iters = itm[(size_t)b * nc + ch];
      L = Lm[(size_t)b * nc + ch];
      return;
    }
    const uint64_t r = mix(seed ^ ((uint64_t)b * 4 + (uint64_t)ch + 1) * 0xD1B54A32D192ED03ull);
    iters = (r >> 40) % 3 == 0 ? 0 : 1 + (int32_t)((r >> 20) % (uint64_t)max_iter);
    L = value(r);
  }
};

Case make_case(uint64_t n) {
  Rng g{mix(n * 2 + 1)};
  Case c;
  c.seed = g.next();
  c.B = 1 + g.below(40);
  c.nc = 1 + g.below(4);
  c.max_iter = 2 + g.below(19);
  c.mit = g.below(2) ? c.max_iter : 1 + g.below(c.max_iter - 1);  // metric_iter == max_iter, or below it
  const int kind = g.below(3);  // sim / non-sim with a finite state / non-sim with -inf
  c.sim = kind == 0;
  static const long long tasks[] = {1, 3, 8};
  c.task = c.sim ? tasks[g.below(3)] : 1000;
  c.first_cw = c.sim ? 1 + (uint64_t)g.below(29) : 0;
  c.nvalues = g.below(2) ? 3 : 1000;
  c.state_in = kind == 1 ? c.value(g.next()) : -INFINITY;
  const int zero_pct = 40 + g.below(56);  // heavy on 0: stale reads chain across codewords
  c.itm.resize((size_t)c.B * c.nc);
  c.Lm.resize((size_t)c.B * c.nc);
  for (size_t e = 0; e < c.itm.size(); e++) {
    c.itm[e] = g.below(100) < zero_pct ? 0 : 1 + g.below(c.mit);
    c.Lm[e] = c.value(g.next());  // a decode that ran no CN phase leaves a sum nobody may read
    if (c.itm[e] == 0) c.Lm[e] = 1e300;
  }
  return c;
}

bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof(a)) == 0; }

int errors = 0;
long long total_feeds = 0, total_links = 0, total_rounds = 0;
#define EXPECT(cond, ...)                                  \
  do {                                                     \
    if (!(cond)) {                                         \
      if (errors++ < 20) {                                 \
        printf("case %" PRIu64 ": ", n);                   \
        printf(__VA_ARGS__);                               \
        printf("\n");                                      \
      }                                                    \
    }                                                      \
  } while (0)

void run_case(uint64_t n) {
  const Case c = make_case(n);
  // the naive model
  std::vector<int32_t> chosen(c.B, 0);
  std::vector<double> met((size_t)4 * c.B, 0.0), hist_met((size_t)4 * c.B, 0.0);
  std::vector<int32_t> hist_chosen(c.B, 0);
  double state = c.sim ? -INFINITY : c.state_in, hist_state = state;
  int links = 0;
  for (int b = 0; b < c.B; b++) {
    if (c.sim && (b == 0 || (c.first_cw + (uint64_t)b) % (uint64_t)c.task == 0)) state = hist_state = -INFINITY;
    for (int pass = 0; pass < 2; pass++) {  // 0: Decoder, 1: GetHistogramData (no final decode)
      double cur = pass ? hist_state : state;
      double *m = (pass ? hist_met : met).data() + (size_t)b * 4;
      for (int i = 0; i < c.nc; i++) {
        if (c.itm[(size_t)b * c.nc + i] > 0) cur = c.Lm[(size_t)b * c.nc + i];
        m[i] = std::fabs(cur);
      }
      int best = 0;
      for (int i = 1; i < c.nc; i++)
        if (m[i] < m[best]) best = i;
      if (pass) {
        hist_chosen[b] = best;
        hist_state = cur;
        continue;
      }
      chosen[b] = best;
      int32_t itf;
      double Lf;
      c.final(b, best, itf, Lf);
      state = itf > 0 ? Lf : cur;
      if (!c.repeats(b, best)) links++;
    }
  }

  // the unit, in rounds
  kml::SoftWalk w(c.B, c.nc, c.mit, c.max_iter, c.itm.data(), c.Lm.data(), c.state_in, c.sim, c.first_cw, c.task);
  int feeds = 0, rounds = 0;
  while (!w.done()) {
    const kml::SoftWalk::Round r = w.next();
    EXPECT(++rounds <= c.B, "the walk does not advance");
    if (rounds > c.B) return;
    EXPECT(r.n >= 1 && r.first + (size_t)r.n == w.list.size(), "round [%zu, +%d) of a list of %zu", r.first, r.n,
           w.list.size());
    for (size_t k = r.first; k < w.list.size(); k++)  // listed only once the choice is final
      EXPECT(w.chosen[w.list[k]] == chosen[w.list[k]], "codeword %d listed with choice %d, final choice %d",
             w.list[k], w.chosen[w.list[k]], chosen[w.list[k]]);
    if (r.feedback >= 0) {
      EXPECT(r.feedback == w.list.back(), "feedback %d is not the round's last codeword %d", r.feedback, w.list.back());
      EXPECT(!c.repeats(r.feedback, w.chosen[r.feedback]), "feedback asked for a repeating final decode (%d)",
             r.feedback);
      int32_t itf;
      double Lf;
      c.final(r.feedback, w.chosen[r.feedback], itf, Lf);
      w.feed(itf, Lf);
      feeds++;
    }
  }
  total_feeds += feeds, total_links += links, total_rounds += rounds;
  EXPECT((int)w.list.size() == c.B, "%zu codewords listed of %d", w.list.size(), c.B);
  for (size_t k = 0; k < w.list.size(); k++) EXPECT(w.list[k] == (int)k, "list[%zu] = %d", k, w.list[k]);
  EXPECT(feeds <= links, "%d feed-backs for %d non-repeating final decodes", feeds, links);
  EXPECT(same_bits(w.state, state), "final state %a, model %a", w.state, state);
  for (int b = 0; b < c.B; b++) {
    EXPECT(w.chosen[b] == chosen[b], "chosen[%d] = %d, model %d", b, w.chosen[b], chosen[b]);
    for (int i = 0; i < 4; i++)
      EXPECT(same_bits(w.met[(size_t)b * 4 + i], met[(size_t)b * 4 + i]), "met[%d][%d] = %a, model %a", b, i,
             w.met[(size_t)b * 4 + i], met[(size_t)b * 4 + i]);
  }

  // the same object without rounds: histogram mode
  kml::SoftWalk h(c.B, c.nc, c.mit, c.max_iter, c.itm.data(), c.Lm.data(), c.state_in, c.sim, c.first_cw, c.task);
  h.metrics_only();
  EXPECT(same_bits(h.state, hist_state), "histogram: final state %a, model %a", h.state, hist_state);
  EXPECT(h.chosen == hist_chosen, "histogram: chosen differs");
  EXPECT(h.met.size() == hist_met.size() && memcmp(h.met.data(), hist_met.data(), 8 * hist_met.size()) == 0,
         "histogram: metrics differ");
}

}  // namespace

int main(int argc, char **argv) {
  const uint64_t cases = argc > 1 ? strtoull(argv[1], nullptr, 10) : 4000;
  for (uint64_t n = 0; n < cases; n++) run_case(n);
  printf("rounds=%lld feed_backs=%lld non_repeating_finals=%lld\n", total_rounds, total_feeds, total_links);
  printf("cases=%" PRIu64 " soft_walk_errors=%d\n", cases, errors);
  return errors ? 1 : 0;
}
