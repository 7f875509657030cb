// layout.cpp — see layout.hpp.  Sections: shared pieces (RNG, plan cache, the VN
// bank-model annealer), RegularLayout, PartitionPlan, IrregularPlan.
#include "layout.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <tuple>
#include <utility>

namespace kml {

// ------------------------------------------------------------ shared pieces
namespace {

struct Xorshift {
  uint64_t s;
  uint64_t next() {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
  }
  double uniform() { return (double)(next() >> 11) * 0x1p-53; }
};

// A plan is a pure function of its key; contexts on the same code (tests, one
// context per rank) reuse it instead of re-running the annealing (seconds).
// The oldest entry leaves when `cap` are held.  The lock is held while
// planning, so contexts created at once on one code plan it once.
template <class Key, class Plan>
class PlanMemo {
 public:
  explicit PlanMemo(size_t cap) : cap_(cap) {}
  template <class Make>
  Plan get(const Key &key, Make make) {
    std::lock_guard<std::mutex> g(mu_);
    for (const auto &e : entries_)
      if (e.first == key) return e.second;
    Plan plan = make();
    if (entries_.size() >= cap_) entries_.erase(entries_.begin());
    entries_.emplace_back(key, std::move(plan));
    return entries_.back().second;
  }

 private:
  const size_t cap_;
  std::mutex mu_;
  std::vector<std::pair<Key, Plan>> entries_;
};

// The VN phase's LDS bank model (bp_regular's, and bp_part's per member):
// position p's column stores its k-th v2c slot with ds_write_b128 (8-lane
// groups: 8 bins of 16 B mod 128 B, bin wb) and reads its k-th c2v with
// ds_read_b64 (32-lane halves: 32 bins of 8 B mod 256 B, bin rb).  Anneals the
// column order ord[lo, hi) against the summed excess group maxima.  Positions
// are grouped by wave (64 consecutive positions) whatever the workgroup size.
// Returns (initial cost, final cost).
std::pair<long long, long long> anneal_vn_order(std::vector<int32_t> &ord, int lo, int hi, int dv,
                                                const std::vector<int32_t> &col_ptr, const std::vector<uint8_t> &wb,
                                                const std::vector<uint8_t> &rb, uint64_t seed, long long iters) {
  const int n = hi - lo;
  const int nW = (n + 7) / 8, nR = (n + 31) / 32;
  std::vector<uint16_t> wc((size_t)nW * dv * 8, 0), rc((size_t)nR * dv * 32, 0);
  std::vector<int> wmax((size_t)nW * dv, 0), rmax((size_t)nR * dv, 0);
  auto wcnt = [&](int g, int k) { return &wc[((size_t)g * dv + k) * 8]; };
  auto rcnt = [&](int g, int k) { return &rc[((size_t)g * dv + k) * 32]; };
  auto gmax = [](const uint16_t *c, int m) {
    int x = 0;
    for (int i = 0; i < m; i++) x = std::max(x, (int)c[i]);
    return x;
  };
  for (int p = 0; p < n; p++)
    for (int k = 0; k < dv; k++) {
      wcnt(p / 8, k)[wb[(size_t)ord[lo + p] * dv + k]]++;
      rcnt(p / 32, k)[rb[(size_t)ord[lo + p] * dv + k]]++;
    }
  long long cost = 0;
  for (int g = 0; g < nW; g++)
    for (int k = 0; k < dv; k++) cost += (wmax[(size_t)g * dv + k] = gmax(wcnt(g, k), 8)) - 1;
  for (int g = 0; g < nR; g++)
    for (int k = 0; k < dv; k++) cost += (rmax[(size_t)g * dv + k] = gmax(rcnt(g, k), 32)) - 1;
  const long long c0 = cost;
  Xorshift rng{seed};
  double temp = 1.0;
  const double cool = std::pow(0.05, 1.0 / (double)std::max(iters, 1LL));
  auto move = [&](int p, int col, int sign) {
    for (int k = 0; k < dv; k++) {
      wcnt(p / 8, k)[wb[(size_t)col * dv + k]] += sign;
      rcnt(p / 32, k)[rb[(size_t)col * dv + k]] += sign;
    }
  };
  auto group_delta = [&](int a, int b, bool commit) {
    long long d = 0;
    for (int k = 0; k < dv; k++) {
      const int ga = a / 8, gb = b / 8;
      int m = gmax(wcnt(ga, k), 8);
      d += m - wmax[(size_t)ga * dv + k];
      if (commit) wmax[(size_t)ga * dv + k] = m;
      if (gb != ga) {
        m = gmax(wcnt(gb, k), 8);
        d += m - wmax[(size_t)gb * dv + k];
        if (commit) wmax[(size_t)gb * dv + k] = m;
      }
      const int ra = a / 32, rb2 = b / 32;
      m = gmax(rcnt(ra, k), 32);
      d += m - rmax[(size_t)ra * dv + k];
      if (commit) rmax[(size_t)ra * dv + k] = m;
      if (rb2 != ra) {
        m = gmax(rcnt(rb2, k), 32);
        d += m - rmax[(size_t)rb2 * dv + k];
        if (commit) rmax[(size_t)rb2 * dv + k] = m;
      }
    }
    return d;
  };
  for (long long it = 0; it < iters; it++, temp *= cool) {
    const int a = (int)(rng.next() % (uint64_t)n), b = (int)(rng.next() % (uint64_t)n);
    if (a / 8 == b / 8) continue;
    const int ca = ord[lo + a], cb = ord[lo + b];
    // swaps only between columns of equal degree (the kernel assigns columns to
    // positions in degree order); vacuous for the partition planner, whose
    // codes are regular, and for bp_regular's one degree
    if (col_ptr[ca + 1] - col_ptr[ca] != col_ptr[cb + 1] - col_ptr[cb]) continue;
    move(a, ca, -1);
    move(b, cb, -1);
    move(a, cb, +1);
    move(b, ca, +1);
    const long long d = group_delta(a, b, false);
    if (d <= 0 || rng.uniform() < std::exp(-(double)d / temp)) {
      group_delta(a, b, true);
      std::swap(ord[lo + a], ord[lo + b]);
      cost += d;
    } else {
      move(a, cb, -1);
      move(b, ca, -1);
      move(a, ca, +1);
      move(b, cb, +1);
    }
  }
  return {c0, cost};
}

}  // namespace

// ------------------------------------------------- RegularLayout (bp_regular)
static RegularLayout plan_regular_uncached(const LdpcCode &L) {
  RegularLayout out;
  const int N = L.N, dv = L.dv_max;
  // CN position of each row -> half bit h(row) = (position >> 2) & 1
  std::vector<int> row_pos(L.M);
  for (int i = 0; i < L.M; i++) row_pos[L.cn_order[i]] = i;
  // Physical slot of the j-th edge of a row (row_ptr order): rows are stored in
  // CN position order, and within a row the edges the even lane reads
  // (j < dc/2, ascending) and the odd lane reads (j >= dc/2, descending)
  // alternate, so at step st the pair reads slots 2st and 2st+1 of its row
  // (slots 2(dc-1-st)+1 and 2(dc-1-st) once st >= dc/2): per-lane base registers
  // plus immediate offsets, and conflict-free ds_read_b128 / ds_write_b64 groups
  // (consecutive positions).
  const int dc = L.dc_max;
  std::vector<int> slot_h(L.E), phys(L.E);
  for (int i = 0; i < L.M; i++)
    for (int e = L.row_ptr[i]; e < L.row_ptr[i + 1]; e++) {
      const int j = e - L.row_ptr[i];
      slot_h[e] = (row_pos[i] >> 2) & 1;
      phys[e] = row_pos[i] * dc + (j < dc / 2 ? 2 * j : 2 * (dc - 1 - j) + 1);
    }
  out.c2v_addr.resize(L.E);
  for (int e = 0; e < L.E; e++) out.c2v_addr[e] = phys[L.col_slot[e]] * 16 + 8 * slot_h[L.col_slot[e]];

  // bank bins per (column, k): see anneal_vn_order
  std::vector<uint8_t> wb((size_t)N * dv), rb((size_t)N * dv);
  for (int j = 0; j < N; j++)
    for (int k = 0; k < dv; k++) {
      const int e = L.col_ptr[j] + std::min(k, L.col_ptr[j + 1] - L.col_ptr[j] - 1);
      const int a = out.c2v_addr[e];
      wb[(size_t)j * dv + k] = (uint8_t)((a >> 4) & 7);
      rb[(size_t)j * dv + k] = (uint8_t)((a >> 3) & 31);
    }
  out.order.assign(L.vn_order.begin(), L.vn_order.end());
  std::tie(out.cost_initial, out.cost_final) =
      anneal_vn_order(out.order, 0, N, dv, L.col_ptr, wb, rb, 0x9E3779B97F4A7C15ull, 1000LL * N * dv);
  out.pos.assign(N, 0);
  for (int p = 0; p < N; p++) out.pos[out.order[p]] = p;
  return out;
}

void plan_regular_layout(const LdpcCode &L, RegularLayout &out) {
  using Key = std::tuple<std::vector<int32_t>, std::vector<int32_t>, std::vector<int32_t>>;
  static PlanMemo<Key, RegularLayout> memo(8);
  out = memo.get(Key(L.row_col, L.col_slot, L.cn_order), [&] { return plan_regular_uncached(L); });
}

// -------------------------------------------- PartitionPlan (bp_part_kernel)
namespace {

// Capacity-bounded majority assignment: every item goes to the part holding
// most of its neighbours, strongest preferences first, each part taking at
// most `cap` items (ties broken by a seeded random key).
void assign_majority(const std::vector<int32_t> &ptr, const std::vector<int32_t> &nbr,
                     const std::vector<int32_t> &nbr_part, int G, int cap, Xorshift &rng,
                     std::vector<int32_t> &part) {
  const int n = (int)ptr.size() - 1;
  struct Cand {
    int cnt;
    uint32_t key;
    int item, g;
  };
  std::vector<Cand> cand;
  cand.reserve((size_t)n * G);
  std::vector<int> cnt(G);
  for (int i = 0; i < n; i++) {
    std::fill(cnt.begin(), cnt.end(), 0);
    for (int e = ptr[i]; e < ptr[i + 1]; e++) cnt[nbr_part[nbr[e]]]++;
    for (int g = 0; g < G; g++) cand.push_back({cnt[g], (uint32_t)rng.next(), i, g});
  }
  std::sort(cand.begin(), cand.end(), [](const Cand &a, const Cand &b) {
    return a.cnt != b.cnt ? a.cnt > b.cnt : a.key < b.key;
  });
  part.assign(n, -1);
  std::vector<int> load(G, 0);
  for (const Cand &c : cand)
    if (part[c.item] < 0 && load[c.g] < cap) {
      part[c.item] = c.g;
      load[c.g]++;
    }
}

// One side of the Tanner graph in PartRefiner::run: the rows, or the columns.
struct Side {
  const std::vector<int32_t> &ptr, &nbr;  // node x's neighbours (nodes of the other side): nbr[ptr[x], ptr[x + 1])
  std::vector<int32_t> &part;             // member of each node
  const int G, n, cap;                    // members; nodes; nodes per member at exact balance
  std::vector<int> cnt, load;             // cnt[x * G + g]: x's neighbours in member g; load[g]: nodes of member g
  Side(const std::vector<int32_t> &ptr_, const std::vector<int32_t> &nbr_, std::vector<int32_t> &part_,
       const std::vector<int32_t> &other_part, int G_, int cap_)
      : ptr(ptr_), nbr(nbr_), part(part_), G(G_), n((int)ptr_.size() - 1), cap(cap_), cnt((size_t)n * G, 0),
        load(G, 0) {
    for (int x = 0; x < n; x++) {
      load[part[x]]++;
      for (int e = ptr[x]; e < ptr[x + 1]; e++) cnt[(size_t)x * G + other_part[nbr[e]]]++;
    }
  }
  // cut edges gained by moving x from member a to member b
  int delta(int x, int a, int b) const { return cnt[(size_t)x * G + a] - cnt[(size_t)x * G + b]; }
  // moves x from a to b; its neighbours' counts live on the other side
  void move(Side &other, int x, int a, int b) {
    for (int e = ptr[x]; e < ptr[x + 1]; e++) {
      other.cnt[(size_t)nbr[e] * G + a]--;
      other.cnt[(size_t)nbr[e] * G + b]++;
    }
    part[x] = b;
    load[a]--;
    load[b]++;
  }
};

}  // namespace

// Cut refinement of the balanced G-way partition (rows and columns of the
// Tanner graph; a cut edge is one whose row and column sit in different
// members, i.e. one mailbox entry of bp_part_kernel).  The BFS seeding and
// majority relabelling below reach a local optimum of "relabel one side given
// the other"; this escapes it by simulated annealing over single-node moves (a
// row or column to a member one of its neighbours is in), with member sizes
// kept within +-kSlack of MG / NG, then a repair to exact balance (the
// cheapest moves) and a greedy same-type swap polish.  kChains chains with
// fixed seeds run in parallel threads and the lowest cut wins (ties: the
// lowest chain), so the plan does not depend on timing or the host.
// PEG8064 at G = 4: 6,602 -> ~5,480 cut edges (27.3 % -> 22.7 % of 24,192).
// Every step is written once for a Side; an odd draw takes the rows, an even
// one the columns.
struct PartRefiner {
  const std::vector<int32_t> &row_ptr, &row_cols, &col_ptr, &col_rows;
  int G, MG, NG;
  long long run(std::vector<int32_t> &R, std::vector<int32_t> &C, long long iters, uint64_t seed) const {
    constexpr int kSlack = 16;
    Side side[2] = {{col_ptr, col_rows, C, R, G, NG}, {row_ptr, row_cols, R, C, G, MG}};  // indexed by r & 1
    long long cut = 0;
    for (int j = 0; j < side[0].n; j++)
      for (int e = col_ptr[j]; e < col_ptr[j + 1]; e++) cut += R[col_rows[e]] != C[j];
    Xorshift rng{seed};
    const double lT0 = std::log(1.0), lT1 = std::log(0.15);
    double acc[64];
    for (long long t = 0; t < iters; t++) {
      if ((t & 1023) == 0) {
        const double T = std::exp(lT0 + (lT1 - lT0) * (double)t / (double)iters);
        for (int d = 0; d < 64; d++) acc[d] = std::exp(-d / T);
      }
      const uint64_t r = rng.next();
      Side &s = side[r & 1], &o = side[~r & 1];
      const int x = (int)((r >> 1) % (uint64_t)s.n), a = s.part[x];
      const int b = o.part[s.nbr[s.ptr[x] + (int)((r >> 33) % (uint64_t)(s.ptr[x + 1] - s.ptr[x]))]];
      if (b == a || s.load[b] >= s.cap + kSlack || s.load[a] <= s.cap - kSlack) continue;
      const int d = s.delta(x, a, b);
      if (d <= 0 || rng.uniform() < acc[std::min(d, 63)]) {
        s.move(o, x, a, b);
        cut += d;
      }
    }
    // exact balance, rows first: the cheapest move from an overfull member to an underfull one
    for (int k = 1; k >= 0; k--) {
      Side &s = side[k], &o = side[1 - k];
      for (;;) {
        int over = -1, under = -1;
        for (int g = 0; g < G; g++) {
          if (s.load[g] > s.cap) over = g;
          if (s.load[g] < s.cap) under = g;
        }
        if (over < 0) break;
        int bx = -1, bd = 1 << 30;
        for (int x = 0; x < s.n; x++) {
          if (s.part[x] != over) continue;
          const int d = s.delta(x, over, under);
          if (d < bd) {
            bd = d;
            bx = x;
          }
        }
        s.move(o, bx, over, under);
        cut += bd;
      }
    }
    // greedy polish: improving swaps of two rows (or two columns) of different
    // members; rows are not adjacent to rows, so the two moves' gains add
    for (int pass = 0; pass < 4; pass++) {
      const long long before = cut;
      for (long long t = 0; t < 4 * (long long)(side[1].n + side[0].n) * G; t++) {
        const uint64_t r = rng.next();
        Side &s = side[r & 1], &o = side[~r & 1];
        const int x = (int)((r >> 1) % (uint64_t)s.n), y = (int)((r >> 32) % (uint64_t)s.n);
        const int a = s.part[x], b = s.part[y];
        if (a == b) continue;
        const int d = s.delta(x, a, b) + s.delta(y, b, a);
        if (d < 0) {
          s.move(o, x, a, b);
          s.move(o, y, b, a);
          cut += d;
        }
      }
      if (cut == before) break;
    }
    return cut;
  }
};

namespace {

// The refinement's schedule: KML_PART_REFINE=0 keeps the relabelling's plan
// (A/B), KML_PART_REFINE_ITERS sets the annealing steps per chain.
struct RefineSchedule {
  bool on = true;
  long long iters = 150000000LL;
};

RefineSchedule refine_schedule_from_env() {
  RefineSchedule s;
  const char *on = getenv("KML_PART_REFINE");
  s.on = !(on && on[0] == '0');
  if (const char *e = getenv("KML_PART_REFINE_ITERS")) s.iters = std::max(0LL, atoll(e));
  if (!s.on) s.iters = 0;  // one cache key for "off"
  return s;
}

// What the steps of plan_partition_uncached hand on.
struct PartWork {
  std::vector<int32_t> slot_row;            // row-order slot -> row
  std::vector<int32_t> col_rows, row_cols;  // adjacency, aligned with col_ptr / row_ptr
  std::vector<int32_t> rpart, cpart;        // member of each row / column
  std::vector<int32_t> row_at;              // row -> index into the plan's cn
  // A cut edge: the members owning its row (R) and its column (S), its row
  // slot in plan order, its column and edge number there, and its mirror slot
  // among S's mirrors.
  struct Cut {
    int R, S, slot, col, k, mirror;
  };
  std::vector<Cut> cuts;            // sorted by (R, slot): the index is the mailbox index x
  std::vector<int32_t> caddr, cvx;  // [j * dv + k], edge k of column j: LDS byte offset; mailbox index or -1
};

bool partitionable(const LdpcCode &L, int G) {
  if (G <= 0 || L.M % G || L.N % G || !L.dv_max || !L.dc_max) return false;
  for (int j = 0; j < L.N; j++)
    if (L.col_ptr[j + 1] - L.col_ptr[j] != L.dv_max) return false;
  for (int i = 0; i < L.M; i++)
    if (L.row_ptr[i + 1] - L.row_ptr[i] != L.dc_max) return false;
  return true;
}

void build_adjacency(const LdpcCode &L, PartWork &w) {
  w.slot_row.resize(L.E);
  for (int i = 0; i < L.M; i++)
    for (int e = L.row_ptr[i]; e < L.row_ptr[i + 1]; e++) w.slot_row[e] = i;
  w.row_cols.assign(L.row_col.begin(), L.row_col.end());
  w.col_rows.resize(L.E);
  for (int e = 0; e < L.E; e++) w.col_rows[e] = w.slot_row[L.col_slot[e]];
}

// initial row parts: breadth-first order over the Tanner graph, cut in G runs
void seed_rows_bfs(const LdpcCode &L, int G, PartWork &w) {
  const int M = L.M;
  std::vector<int32_t> order;
  order.reserve(M);
  std::vector<char> seen_r(M, 0), seen_c(L.N, 0);
  for (int s = 0; s < M; s++) {
    if (seen_r[s]) continue;
    size_t head = order.size();
    order.push_back(s);
    seen_r[s] = 1;
    while (head < order.size()) {
      const int r = order[head++];
      for (int e = L.row_ptr[r]; e < L.row_ptr[r + 1]; e++) {
        const int c = w.row_cols[e];
        if (seen_c[c]) continue;
        seen_c[c] = 1;
        for (int f = L.col_ptr[c]; f < L.col_ptr[c + 1]; f++) {
          const int r2 = w.col_rows[f];
          if (!seen_r[r2]) {
            seen_r[r2] = 1;
            order.push_back(r2);
          }
        }
      }
    }
  }
  w.rpart.assign(M, -1);
  for (int k = 0; k < M; k++) w.rpart[order[k]] = (int32_t)((long long)k * G / M);
}

// 40 rounds of "columns by majority given the rows, rows given the columns";
// leaves the labels of the lowest cut in w and returns that cut
long long relabel_by_majority(const LdpcCode &L, int G, PartWork &w) {
  auto cut_of = [&](const std::vector<int32_t> &rp, const std::vector<int32_t> &cp) {
    long long n = 0;
    for (int j = 0; j < L.N; j++)
      for (int e = L.col_ptr[j]; e < L.col_ptr[j + 1]; e++) n += rp[w.col_rows[e]] != cp[j];
    return n;
  };
  Xorshift rng{0xC2B2AE3D27D4EB4Full};
  long long best = -1;
  std::vector<int32_t> rpart = w.rpart, cpart;
  for (int it = 0; it < 40; it++) {
    assign_majority(L.col_ptr, w.col_rows, rpart, G, L.N / G, rng, cpart);
    const long long cc = cut_of(rpart, cpart);
    if (best < 0 || cc < best) {
      best = cc;
      w.rpart = rpart;
      w.cpart = cpart;
    }
    assign_majority(L.row_ptr, w.row_cols, cpart, G, L.M / G, rng, rpart);
  }
  return best;
}

// PartRefiner's chains, one thread each; w keeps the labels of the lowest cut
void refine_in_threads(const LdpcCode &L, int G, long long iters, long long best, PartWork &w) {
  constexpr int kChains = 4;
  const PartRefiner pr{L.row_ptr, w.row_cols, L.col_ptr, w.col_rows, G, L.M / G, L.N / G};
  std::vector<std::vector<int32_t>> rs(kChains, w.rpart), cs(kChains, w.cpart);
  std::vector<long long> cut(kChains, -1);
  std::vector<std::thread> th;
  for (int k = 0; k < kChains; k++)
    th.emplace_back([&, k] { cut[k] = pr.run(rs[k], cs[k], iters, 0x243F6A8885A308D3ull * (uint64_t)(k + 1)); });
  for (auto &t : th) t.join();
  for (int k = 0; k < kChains; k++)
    if (cut[k] < best) {
      best = cut[k];
      w.rpart = rs[k];
      w.cpart = cs[k];
    }
}

// Member orders (rows and columns by index; the columns are annealed later),
// the cut edges sorted by (row owner, partitioned row slot), and the members'
// exchange lists.  False when the cut does not fit the packed entries.
bool build_exchange_lists(const LdpcCode &L, PartWork &w, PartitionPlan &out) {
  const int M = L.M, N = L.N, G = out.G, dc = L.dc_max, EG = out.MG * dc;
  out.vn.clear();
  out.cn.clear();
  for (int g = 0; g < G; g++) {
    for (int j = 0; j < N; j++)
      if (w.cpart[j] == g) out.vn.push_back(j);
    for (int i = 0; i < M; i++)
      if (w.rpart[i] == g) out.cn.push_back(i);
  }
  w.row_at.resize(M);
  for (int p = 0; p < M; p++) w.row_at[out.cn[p]] = p;

  std::vector<PartWork::Cut> &cuts = w.cuts;
  for (int p = 0; p < N; p++) {
    const int j = out.vn[p];
    for (int e = L.col_ptr[j], k = 0; e < L.col_ptr[j + 1]; e++, k++) {
      const int s = L.col_slot[e], r = w.slot_row[s];
      if (w.rpart[r] != w.cpart[j])
        cuts.push_back({w.rpart[r], w.cpart[j], w.row_at[r] * dc + (s - L.row_ptr[r]), j, k, 0});
    }
  }
  std::sort(cuts.begin(), cuts.end(), [](const PartWork::Cut &a, const PartWork::Cut &b) {
    return a.R != b.R ? a.R < b.R : a.slot < b.slot;
  });
  out.ncut = (int)cuts.size();
  std::vector<char> pair((size_t)G * G, 0);
  for (const PartWork::Cut &c : cuts) pair[(size_t)c.R * G + c.S] = 1;
  out.all_pairs = true;
  for (int r = 0; r < G; r++)
    for (int q = 0; q < G; q++)
      if (r != q && !pair[(size_t)r * G + q]) out.all_pairs = false;
  if (out.ncut >= (1 << 15)) return false;  // packed (x << 16) entries

  std::vector<std::vector<int32_t>> xr(G), xc(G);
  for (size_t x = 0; x < cuts.size(); x++) {
    PartWork::Cut &c = cuts[x];
    xr[c.R].push_back((int32_t)((x << 16) | (uint32_t)(c.slot - c.R * EG)));
    c.mirror = (int)xc[c.S].size();
    xc[c.S].push_back((int32_t)((x << 16) | (uint32_t)(EG + c.mirror)));
  }
  out.mirror_max = 0;
  out.xr.clear();
  out.xc.clear();
  out.xr_ptr.assign(1, 0);
  out.xc_ptr.assign(1, 0);
  for (int g = 0; g < G; g++) {
    out.mirror_max = std::max(out.mirror_max, (int)xc[g].size());
    if (EG + (int)xc[g].size() >= (1 << 16)) return false;
    out.xr.insert(out.xr.end(), xr[g].begin(), xr[g].end());
    out.xc.insert(out.xc.end(), xc[g].begin(), xc[g].end());
    out.xr_ptr.push_back((int32_t)out.xr.size());
    out.xc_ptr.push_back((int32_t)out.xc.size());
  }
  return true;
}

// per-edge LDS addresses of the VN phase, per column: own row slot, or the
// mirror slot
void address_column_edges(const LdpcCode &L, const PartitionPlan &out, PartWork &w) {
  const int dv = L.dv_max, dc = L.dc_max, EG = out.MG * dc;
  w.caddr.assign((size_t)L.N * dv, 0);
  w.cvx.assign((size_t)L.N * dv, -1);
  for (int j = 0; j < L.N; j++) {
    const int g = w.cpart[j];
    for (int e = L.col_ptr[j], k = 0; e < L.col_ptr[j + 1]; e++, k++) {
      const int s = L.col_slot[e], r = w.slot_row[s];
      if (w.rpart[r] == g) w.caddr[(size_t)j * dv + k] = ((w.row_at[r] - g * out.MG) * dc + (s - L.row_ptr[r])) * 16;
    }
  }
  for (size_t x = 0; x < w.cuts.size(); x++) {
    const PartWork::Cut &c = w.cuts[x];
    w.caddr[(size_t)c.col * dv + c.k] = (EG + c.mirror) * 16;
    w.cvx[(size_t)c.col * dv + c.k] = (int32_t)x;
  }
}

// The columns' lane positions within each member: annealed against the VN
// phase's bank conflicts (write bins of the slot, read bins of the c2v half:
// bp_coop.hip part_c2v_half — bit 2 of the row for row slots, of the slot
// index for mirror slots).
// Each member's INTERIOR columns (every edge's row its own) last, so the
// boundary columns, whose v2c the partners wait for, are stored first; the
// annealing keeps the two runs apart (a VN phase split around the c2v
// receive, interior columns first, measured slower: 8.75 vs 8.20 ms per 4096
// PEG8064 codewords, profiles/r05_ab2_summary.txt)
void order_member_columns(const LdpcCode &L, const PartWork &w, PartitionPlan &out) {
  const int N = L.N, G = out.G, NG = out.NG, dv = L.dv_max, dc = L.dc_max, EG = out.MG * dc;
  std::vector<int> nbound(G, NG);
  out.interior = 0;
  for (int g = 0; g < G; g++) {
    auto interior = [&](int j) {
      for (int e = L.col_ptr[j]; e < L.col_ptr[j + 1]; e++)
        if (w.rpart[w.col_rows[e]] != g) return false;
      return true;
    };
    auto first = out.vn.begin() + (size_t)g * NG, last = first + NG;
    nbound[g] = (int)(std::stable_partition(first, last, [&](int j) { return !interior(j); }) - first);
    out.interior += NG - nbound[g];
  }
  std::vector<uint8_t> wb((size_t)N * dv), rb((size_t)N * dv);
  for (int j = 0; j < N; j++)
    for (int k = 0; k < dv; k++) {
      const int a = w.caddr[(size_t)j * dv + k], sl = a >> 4;
      const int half = sl < EG ? ((sl / dc) >> 2) & 1 : (sl >> 2) & 1;
      wb[(size_t)j * dv + k] = (uint8_t)((a >> 4) & 7);
      rb[(size_t)j * dv + k] = (uint8_t)(((a + 8 * half) >> 3) & 31);
    }
  out.anneal_initial = out.anneal_final = 0;
  for (int g = 0; g < G; g++)
    for (int part = 0; part < 2; part++) {
      const int lo = g * NG + (part ? nbound[g] : 0), hi = part ? (g + 1) * NG : g * NG + nbound[g];
      if (hi - lo < 2) continue;
      const auto c = anneal_vn_order(out.vn, lo, hi, dv, L.col_ptr, wb, rb,
                                     0x9E3779B97F4A7C15ull + (uint64_t)(2 * g + part), 300LL * (hi - lo) * dv);
      out.anneal_initial += c.first;
      out.anneal_final += c.second;
    }
}

// the tables indexed by lane position (pos, vaddr, vx) and by plan row (rx)
void fill_lane_tables(const LdpcCode &L, const PartWork &w, PartitionPlan &out) {
  const int N = L.N, dv = L.dv_max, dc = L.dc_max;
  out.pos.assign(N, 0);
  for (int p = 0; p < N; p++) out.pos[out.vn[p]] = p;
  out.vaddr.assign((size_t)N * dv, 0);
  out.vx.assign((size_t)N * dv, -1);
  for (int p = 0; p < N; p++)
    for (int k = 0; k < dv; k++) {
      out.vaddr[(size_t)p * dv + k] = w.caddr[(size_t)out.vn[p] * dv + k];
      out.vx[(size_t)p * dv + k] = w.cvx[(size_t)out.vn[p] * dv + k];
    }
  out.rx.assign(L.M, 0);
  for (size_t x = 0; x < w.cuts.size(); x++) {
    const int P = w.cuts[x].slot / dc, e = w.cuts[x].slot % dc;  // plan row index, edge position in the row
    if (!(out.rx[P] & 0xFF)) out.rx[P] = (int32_t)(x << 8);
    out.rx[P] |= 1 << e;
  }
}

struct PartitionResult {
  bool ok = false;
  PartitionPlan plan;
};

PartitionResult plan_partition_uncached(const LdpcCode &L, int G, const RefineSchedule &sched) {
  PartitionResult res;
  if (!partitionable(L, G)) return res;
  PartitionPlan &out = res.plan;
  PartWork w;
  build_adjacency(L, w);
  seed_rows_bfs(L, G, w);
  const long long best = relabel_by_majority(L, G, w);
  if (sched.on) refine_in_threads(L, G, sched.iters, best, w);
  out.G = G;
  out.MG = L.M / G;
  out.NG = L.N / G;
  if (!build_exchange_lists(L, w, out)) return res;
  address_column_edges(L, out, w);
  order_member_columns(L, w, out);
  fill_lane_tables(L, w, out);
  res.ok = true;
  return res;
}

}  // namespace

bool plan_partition(const LdpcCode &L, int G, PartitionPlan &out) {
  using Key = std::tuple<std::vector<int32_t>, std::vector<int32_t>, int, bool, long long>;
  static PlanMemo<Key, PartitionResult> memo(4);
  const RefineSchedule sched = refine_schedule_from_env();
  const PartitionResult res = memo.get(Key(L.row_col, L.col_slot, G, sched.on, sched.iters),
                                       [&] { return plan_partition_uncached(L, G, sched); });
  out = res.plan;
  return res.ok;
}

// -------------------------------------------- IrregularPlan (bp_irregular)
namespace {

// One wave's worth of items (64 columns, or 32 rows) for one round.
struct WaveItems {
  std::vector<int32_t> a, b;  // a: the (first) items; b: the second items of a pair wave
  double cost = 0;
};

// items[d] = the items of degree d.  cost(d) models one item's VALU work.
// Returns false when the items do not fit W pair waves + W single waves.
bool plan_rounds(std::vector<std::vector<int32_t>> items, int per_wave, int W, int pair_max, double (*cost)(int),
                 std::vector<WaveItems> &pairs, std::vector<WaveItems> &singles) {
  const int dmax = (int)items.size() - 1;
  pairs.clear();
  singles.clear();
  // pair waves from the highest degrees (up to pair_max): 2 * per_wave items of one degree
  for (int d = std::min(dmax, pair_max); d >= 0 && (int)pairs.size() < W; --d)
    while ((int)items[d].size() >= 2 * per_wave && (int)pairs.size() < W) {
      WaveItems w;
      w.a.assign(items[d].begin(), items[d].begin() + per_wave);
      w.b.assign(items[d].begin() + per_wave, items[d].begin() + 2 * per_wave);
      items[d].erase(items[d].begin(), items[d].begin() + 2 * per_wave);
      w.cost = 2 * per_wave * cost(d);
      pairs.push_back(std::move(w));
    }
  // leftover pair slots take a partial pair wave of one degree (at least half
  // a wave of pairs, lowest degrees first), so that fewer single waves mix
  // two degrees (a mixed wave runs both degrees' code paths)
  for (int d = 0; d <= std::min(dmax, pair_max) && (int)pairs.size() < W; ++d) {
    const int np = (int)items[d].size() / 2;
    if (np < per_wave / 2 || np >= per_wave) continue;
    WaveItems w;
    w.a.assign(items[d].begin(), items[d].begin() + np);
    w.b.assign(items[d].begin() + np, items[d].begin() + 2 * np);
    items[d].erase(items[d].begin(), items[d].begin() + 2 * np);
    w.cost = 2 * np * cost(d);
    pairs.push_back(std::move(w));
  }
  // the rest as single waves, highest degree first; a partial wave is topped up
  // with the next degree's items (a mixed wave)
  WaveItems cur;
  for (int d = dmax; d >= 0; --d)
    for (int32_t it : items[d]) {
      cur.a.push_back(it);
      cur.cost += cost(d);
      if ((int)cur.a.size() == per_wave) {
        singles.push_back(std::move(cur));
        cur = WaveItems();
      }
    }
  if (!cur.a.empty()) singles.push_back(std::move(cur));
  return (int)singles.size() <= W;
}

// Place pair waves and single waves on lane waves 0..W-1 so that the SIMD
// totals (wave w on SIMD w % 4) are balanced: longest-processing-time first,
// each SIMD taking W/4 pair waves and W/4 single waves.
void place_waves(const std::vector<WaveItems> &pairs, const std::vector<WaveItems> &singles, int W,
                 std::vector<int> &pair_of, std::vector<int> &single_of) {
  const int per = W / 4;
  std::vector<double> load(4, 0.0);
  std::vector<std::vector<int>> simd_waves(4);
  for (int w = 0; w < W; ++w) simd_waves[w % 4].push_back(w);
  pair_of.assign(W, -1);
  single_of.assign(W, -1);
  auto lpt = [&](const std::vector<WaveItems> &v, std::vector<int> &of) {
    std::vector<int> idx(v.size());
    for (size_t i = 0; i < v.size(); ++i) idx[i] = (int)i;
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return v[x].cost > v[y].cost; });
    std::vector<int> used(4, 0);
    for (int i : idx) {
      int best = -1;
      for (int s = 0; s < 4; ++s)
        if (used[s] < per && (best < 0 || load[s] < load[best])) best = s;
      of[simd_waves[best][used[best]++]] = i;
      load[best] += v[i].cost;
    }
  };
  lpt(pairs, pair_of);
  lpt(singles, single_of);
}

// div2 steps of a column (forward d-1, backward 2d-1); a degree-1 column's
// FAST v2c needs none (bp_irregular.hip vn_cols), only its hard decision
double vn_cost(int d) { return d == 1 ? 2.0 : 3.0 * d - 1.0; }
double cn_cost(int d) { return 1.5 * d; }        // per half-row: advances + half the c2v outputs

// slot blocks (kIrrCnStride), one per wave and round, in plan order; false
// when a row of the code is not in out.cn
bool place_slot_blocks(const LdpcCode &L, int T, IrregularPlan &out) {
  std::vector<int32_t> slot_of(L.E, -1);
  out.cn_base.assign(3 * T / 2, -1);
  int next = 0;
  for (int r = 0; r < 3; ++r)
    for (int w = 0; w < T / 64; ++w) {
      const int p0 = r * (T / 2) + w * 32;
      int dw = 0;
      for (int pi = 0; pi < 32; ++pi) {
        const int row = out.cn[p0 + pi];
        if (row >= 0) dw = std::max(dw, L.row_ptr[row + 1] - L.row_ptr[row]);
      }
      for (int pi = 0; pi < 32; ++pi) {
        const int row = out.cn[p0 + pi];
        if (row < 0) continue;
        out.cn_base[p0 + pi] = next + pi;
        for (int e = L.row_ptr[row]; e < L.row_ptr[row + 1]; ++e)
          slot_of[e] = next + pi + (e - L.row_ptr[row]) * kIrrCnStride;
      }
      next += dw * kIrrCnStride;
    }
  for (int32_t s : slot_of)
    if (s < 0) return false;
  out.n_slots = next;
  out.col_slot.resize(L.E);
  for (int e = 0; e < L.E; ++e) out.col_slot[e] = slot_of[L.col_slot[e]];
  return true;
}

}  // namespace

bool plan_irregular(const LdpcCode &L, int T, int vn_pair_max, int cn_pair_max, IrregularPlan &out) {
  if (T % 256) return false;
  const int W = T / 64;
  std::vector<std::vector<int32_t>> cols(L.dv_max + 1), rows(L.dc_max + 1);
  for (int32_t v : L.vn_order) cols[L.col_ptr[v + 1] - L.col_ptr[v]].push_back(v);
  for (int32_t r : L.cn_order) rows[L.row_ptr[r + 1] - L.row_ptr[r]].push_back(r);
  std::vector<WaveItems> vp, vs, cp, cs;
  if (!plan_rounds(cols, 64, W, vn_pair_max, vn_cost, vp, vs) ||
      !plan_rounds(rows, 32, W, cn_pair_max, cn_cost, cp, cs))
    return false;
  std::vector<int> vp_of, vs_of, cp_of, cs_of;
  place_waves(vp, vs, W, vp_of, vs_of);
  place_waves(cp, cs, W, cp_of, cs_of);
  out.vn.assign(3 * T, -1);
  out.cn.assign(3 * T / 2, -1);
  for (int w = 0; w < W; ++w) {
    if (vp_of[w] >= 0)
      for (size_t l = 0; l < vp[vp_of[w]].a.size(); ++l) {  // (a partial pair wave leaves lanes idle)
        out.vn[w * 64 + l] = vp[vp_of[w]].a[l];
        out.vn[T + w * 64 + l] = vp[vp_of[w]].b[l];
      }
    if (vs_of[w] >= 0)
      for (size_t l = 0; l < vs[vs_of[w]].a.size(); ++l) out.vn[2 * T + w * 64 + l] = vs[vs_of[w]].a[l];
    if (cp_of[w] >= 0)
      for (size_t l = 0; l < cp[cp_of[w]].a.size(); ++l) {
        out.cn[w * 32 + l] = cp[cp_of[w]].a[l];
        out.cn[T / 2 + w * 32 + l] = cp[cp_of[w]].b[l];
      }
    if (cs_of[w] >= 0)
      for (size_t l = 0; l < cs[cs_of[w]].a.size(); ++l) out.cn[T + w * 32 + l] = cs[cs_of[w]].a[l];
  }
  return place_slot_blocks(L, T, out);
}

// ---------------------------------------- LayeredPlan (bp_irregular_lnms)
void plan_layered(const LdpcCode &L, LayeredPlan &out) {
  out.layer_ptr.assign(1, 0);
  out.pass.clear();
  std::vector<int32_t> open_at(L.N, -1);  // column -> first row of the layer that last touched it
  int first = 0;
  auto close = [&](int end) {  // the layer [first, end) in passes
    for (int r = first; r < end; r += kLayRowsPerPass) {
      const int n = std::min(kLayRowsPerPass, end - r);
      out.pass.push_back(r | n << 16 | (r + n == end ? 1 : 0) << 24);
    }
  };
  for (int r = 0; r < L.M; ++r) {
    bool shared = false;
    for (int e = L.row_ptr[r]; e < L.row_ptr[r + 1]; ++e) shared |= open_at[L.row_col[e]] == first;
    if (shared && r > first) {
      close(r);
      out.layer_ptr.push_back(r);
      first = r;
    }
    for (int e = L.row_ptr[r]; e < L.row_ptr[r + 1]; ++e) open_at[L.row_col[e]] = first;
  }
  close(L.M);
  out.layer_ptr.push_back(L.M);
}

bool layered_items(const LdpcCode &L, const LayeredPlan &plan, std::vector<uint32_t> &out) {
  out.clear();
  if (L.E > 65535 || L.N >= 65535 || L.M > 65535) return false;  // (the pass words hold 16 bits of the first row)
  out.assign(plan.pass.size() * (size_t)kIrrThreads * 2, 0);
  for (size_t p = 0; p < plan.pass.size(); ++p) {
    const int first = plan.pass[p] & 0xFFFF, nrows = (plan.pass[p] >> 16) & 0xFF;
    for (int t = 0; t < kIrrThreads; ++t) {
      uint32_t *w = &out[(p * kIrrThreads + t) * 2];
      const int g = t / kLayLanesPerRow, l = t % kLayLanesPerRow;
      w[0] = ~0u;
      if (g >= nrows) continue;
      const int b = L.row_ptr[first + g], d = L.row_ptr[first + g + 1] - b;
      if (d > 2 * kLayLanesPerRow) return false;
      if (l >= d) continue;
      w[0] = (uint32_t)L.row_col[b + l] | (l + kLayLanesPerRow < d ? (uint32_t)L.row_col[b + l + kLayLanesPerRow] : 0xFFFFu) << 16;
      w[1] = (uint32_t)(b + l);
    }
  }
  return true;
}

}  // namespace kml
