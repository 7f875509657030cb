// Host checks of the kernels' placement plans (layout.cpp) on the reference's
// H files: every plan is a valid assignment of columns / rows / slots to lanes
// with the properties the kernels rely on.  Prints "plan_errors=0" on success.
//   plan_check <PEG2304 H> <BG2 H> <PEG8064 H> [--regular F | --irregular F | --partition F | --none F]...
// The extra (non-5G) H files are checked in the named role: the regular plan
// of another PEG2304-class code, the irregular plan (with a census line of
// what its waves hold), the partition plan, or neither plan being made (the
// code decodes on the generic bp_kernel).
// After each plan's checks one line pins the plan itself:
//   digest <regular|irregular|partition> <H file name> <16 hex digits>
// (tests/golden/host/plan_digests.json holds the recorded lines), and a
// --partition file is also planned under three refinement schedules in this
// one process (check_schedules).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "code.hpp"
#include "layout.hpp"

using namespace kml;

static int errors = 0;
#define CHECK(c, ...)                 \
  do {                                \
    if (!(c)) {                       \
      ++errors;                       \
      if (errors < 20) {              \
        printf("FAIL %s: ", #c);      \
        printf(__VA_ARGS__);          \
        printf("\n");                 \
      }                               \
    }                                 \
  } while (0)

static bool load(LdpcCode &L, const char *path, bool is5g) {
  std::string err;
  if (!L.load(path, is5g, true, false, err)) {
    printf("load %s: %s\n", path, err.c_str());
    return false;
  }
  return true;
}

static const char *base_name(const char *path) { return strrchr(path, '/') ? strrchr(path, '/') + 1 : path; }

// 64-bit FNV-1a over a plan: every array (its elements as int64, then its
// length) and every scalar (as int64), bytes least significant first.
struct Digest {
  uint64_t h = 0xcbf29ce484222325ull;
  Digest &add(long long v) {
    for (int b = 0; b < 8; b++) {
      h ^= ((uint64_t)v >> (8 * b)) & 0xFF;
      h *= 0x100000001b3ull;
    }
    return *this;
  }
  Digest &add(const std::vector<int32_t> &a) {
    for (int32_t x : a) add((long long)x);
    return add((long long)a.size());
  }
  void print(const char *plan, const char *name) const {
    printf("digest %s %s %016llx\n", plan, name, (unsigned long long)h);
  }
};

static int col_deg(const LdpcCode &L, int v) { return L.col_ptr[v + 1] - L.col_ptr[v]; }
static int row_deg(const LdpcCode &L, int r) { return L.row_ptr[r + 1] - L.row_ptr[r]; }

// bp_regular.hip: rows in CN-position order with the lane pair's edges
// interleaved; each edge's c2v byte address names its own slot and half.
static void check_regular(const LdpcCode &L, const char *name) {
  RegularLayout P;
  plan_regular_layout(L, P);
  CHECK((int)P.order.size() == L.N, "order size %zu", P.order.size());
  std::vector<int> seen(L.N, 0);
  for (int v : P.order) seen[v]++;
  for (int v = 0; v < L.N; v++) CHECK(seen[v] == 1, "column %d placed %d times", v, seen[v]);
  for (int p = 0; p < L.N; p++) CHECK(P.pos[P.order[p]] == p, "pos of position %d", p);
  std::vector<int> row_pos(L.M);
  for (int i = 0; i < L.M; i++) row_pos[L.cn_order[i]] = i;
  std::set<int> slots;
  for (int e = 0; e < L.E; e++) {  // e: a column-order edge; col_slot[e] = its row-order slot
    const int s = L.col_slot[e];
    int row = 0;
    while (L.row_ptr[row + 1] <= s) row++;
    const int j = s - L.row_ptr[row], dc = row_deg(L, row);
    const int phys = row_pos[row] * dc + (j < dc / 2 ? 2 * j : 2 * (dc - 1 - j) + 1);
    const int a = P.c2v_addr[e];
    CHECK(a / 16 == phys, "edge %d slot %d != %d", e, a / 16, phys);
    CHECK((a & 8) == 8 * ((row_pos[row] >> 2) & 1), "edge %d half", e);
    slots.insert(a / 16);
  }
  CHECK((int)slots.size() == L.E, "distinct slots %zu", slots.size());
  printf("regular: bank-conflict cost %lld -> %lld\n", P.cost_initial, P.cost_final);
  Digest().add(P.order).add(P.pos).add(P.c2v_addr).add(P.cost_initial).add(P.cost_final).print("regular", name);
}

static std::string set_str(const std::set<int> &s) {
  std::string o = "{";
  for (int d : s) o += (o.size() > 1 ? "," : "") + std::to_string(d);
  return o + "}";
}

// What the waves of an irregular plan hold, per phase: the degrees that occur
// paired (rounds 0-1: a lane's two columns, a lane pair's two rows) and single
// (round 2), and the number of waves that mix degrees, that are idle (a pair
// wave without a pair, a single wave without a node) and of partly filled pair
// waves.  One line per phase:
//   census <name> <vn|cn>: paired {..} single {..} mixed A idle B partial_pair C
static void irregular_census(const LdpcCode &L, const IrregularPlan &P, int T, const char *name) {
  for (int phase = 0; phase < 2; phase++) {
    const int per_wave = phase ? 32 : 64, n = phase ? T / 2 : T;  // positions per wave / per round
    const std::vector<int32_t> &a = phase ? P.cn : P.vn;
    auto deg = [&](int x) { return phase ? row_deg(L, x) : col_deg(L, x); };
    std::set<int> paired, single;
    int mixed = 0, idle = 0, partial = 0;
    for (int w = 0; w < n / per_wave; w++) {
      std::set<int> dp, ds;
      int np = 0;
      for (int i = w * per_wave; i < (w + 1) * per_wave; i++) {
        if (a[i] >= 0) dp.insert(deg(a[i])), np++;
        if (a[n + i] >= 0) dp.insert(deg(a[n + i]));
        if (a[2 * n + i] >= 0) ds.insert(deg(a[2 * n + i]));
      }
      paired.insert(dp.begin(), dp.end());
      single.insert(ds.begin(), ds.end());
      mixed += (dp.size() > 1) + (ds.size() > 1);
      idle += dp.empty() + ds.empty();
      partial += np > 0 && np < per_wave;
    }
    printf("census %s %s: paired %s single %s mixed %d idle %d partial_pair %d\n", name, phase ? "cn" : "vn",
           set_str(paired).c_str(), set_str(single).c_str(), mixed, idle, partial);
  }
}

// bp_irregular.hip: three rounds, pairs of equal degree (up to the limits) in
// rounds 0-1, every column / row exactly once, one degree per paired wave.
// census: print the census of the plan too.
static void check_irregular(const LdpcCode &L, const char *name, bool census = false) {
  const int T = kIrrThreads;
  IrregularPlan P;
  CHECK(plan_irregular(L, T, kIrrVnPairMax, kIrrCnPairMax, P), "plan_irregular failed");
  if (P.vn.empty()) return;
  CHECK((int)P.vn.size() == 3 * T && (int)P.cn.size() == 3 * T / 2, "sizes");
  std::vector<int> cs(L.N, 0), rs(L.M, 0);
  for (int v : P.vn)
    if (v >= 0) cs[v]++;
  for (int r : P.cn)
    if (r >= 0) rs[r]++;
  for (int v = 0; v < L.N; v++) CHECK(cs[v] == 1, "column %d placed %d times", v, cs[v]);
  for (int r = 0; r < L.M; r++) CHECK(rs[r] == 1, "row %d placed %d times", r, rs[r]);
  for (int t = 0; t < T; t++) {
    const int a = P.vn[t], b = P.vn[T + t];
    CHECK((a < 0) == (b < 0), "lane %d half-empty pair", t);
    if (a >= 0) {
      CHECK(col_deg(L, a) == col_deg(L, b), "lane %d pair degrees", t);
      CHECK(col_deg(L, a) <= kIrrVnPairMax, "lane %d pair degree %d", t, col_deg(L, a));
      CHECK(col_deg(L, a) == col_deg(L, P.vn[(t & ~63)]) || P.vn[t & ~63] < 0, "wave of lane %d mixes degrees", t);
    }
  }
  for (int q = 0; q < T / 2; q++) {
    const int a = P.cn[q], b = P.cn[T / 2 + q];
    CHECK((a < 0) == (b < 0), "pair %d half-empty", q);
    if (a >= 0) {
      CHECK(row_deg(L, a) == row_deg(L, b), "pair %d row degrees", q);
      CHECK(row_deg(L, a) <= kIrrCnPairMax, "pair %d row degree %d", q, row_deg(L, a));
    }
  }
  // slot blocks: edge e of the row at a lane pair sits at cn_base + e * kIrrCnStride,
  // every edge has its own slot, and the column-ordered table points at the same slots
  CHECK((int)P.cn_base.size() == 3 * T / 2 && (int)P.col_slot.size() == L.E, "slot table sizes");
  std::vector<int> owner(P.n_slots, -1), slot_of(L.E, -1);
  for (int q = 0; q < 3 * T / 2; q++) {
    const int r = P.cn[q];
    CHECK((r < 0) == (P.cn_base[q] < 0), "pair position %d base", q);
    if (r < 0) continue;
    for (int e = L.row_ptr[r]; e < L.row_ptr[r + 1]; e++) {
      const int s = P.cn_base[q] + (e - L.row_ptr[r]) * kIrrCnStride;
      CHECK(s >= 0 && s < P.n_slots && owner[s] < 0, "edge %d slot %d", e, s);
      if (s >= 0 && s < P.n_slots) owner[s] = e;
      slot_of[e] = s;
    }
  }
  for (int e = 0; e < L.E; e++) CHECK(P.col_slot[e] == slot_of[L.col_slot[e]], "column edge %d slot", e);
  printf("irregular: plan ok for T=%d, %d slots for %d edges\n", T, P.n_slots, L.E);
  if (census) irregular_census(L, P, T, name);
  Digest().add(P.vn).add(P.cn).add(P.cn_base).add(P.col_slot).add(P.n_slots).print("irregular", name);
}

static Digest digest_partition(const PartitionPlan &P) {
  Digest d;
  d.add(P.G).add(P.MG).add(P.NG).add(P.ncut).add(P.mirror_max).add(P.vn).add(P.cn).add(P.pos).add(P.vaddr);
  d.add(P.xr).add(P.xr_ptr).add(P.xc).add(P.xc_ptr).add(P.vx).add(P.rx).add(P.anneal_initial).add(P.anneal_final);
  return d.add(P.interior).add(P.all_pairs);
}

// bp_part_kernel: members own whole column / row blocks; every edge's LDS
// address of the column side is a row slot of the owner or one of its mirrors.
static void check_partition(const LdpcCode &L, const char *name, bool peg8064 = true) {
  PartitionPlan P;
  CHECK(plan_partition(L, 4, P), "plan_partition failed");
  if (P.vn.empty()) return;
  std::vector<int> cs(L.N, 0), rs(L.M, 0);
  for (int v : P.vn) cs[v]++;
  for (int r : P.cn) rs[r]++;
  for (int v = 0; v < L.N; v++) CHECK(cs[v] == 1, "column %d placed %d times", v, cs[v]);
  for (int r = 0; r < L.M; r++) CHECK(rs[r] == 1, "row %d placed %d times", r, rs[r]);
  const int nslots = P.MG * L.dc_max + P.mirror_max;
  for (size_t i = 0; i < P.vaddr.size(); i++)
    CHECK(P.vaddr[i] >= 0 && P.vaddr[i] < nslots * 16, "vaddr %zu = %d", i, P.vaddr[i]);
  // tagged exchange: a row's cut edges have consecutive mailbox indices from
  // rx's first index, in row order; vx names the same index from the column side
  std::vector<int> seen_x(P.ncut, 0);
  const int EG = P.MG * L.dc_max;
  for (int m = 0; m < P.G; m++)
    for (int q = P.xr_ptr[m]; q < P.xr_ptr[m + 1]; q++) {
      const int x = P.xr[q] >> 16, slot = P.xr[q] & 0xFFFF;  // member-local row slot
      const int Pr = m * P.MG + slot / L.dc_max, e = slot % L.dc_max;
      const int mask = P.rx[Pr] & 0xFF;
      CHECK((mask >> e) & 1, "row %d edge %d not in its cut mask", Pr, e);
      const int want = (P.rx[Pr] >> 8) + __builtin_popcount(mask & ((1 << e) - 1));
      CHECK(x == want, "row %d edge %d: x %d, rx gives %d", Pr, e, x, want);
      seen_x[x]++;
    }
  long long nvx = 0;
  for (size_t i = 0; i < P.vx.size(); i++)
    if (P.vx[i] >= 0) {
      ++nvx;
      CHECK(P.vx[i] < P.ncut, "vx %zu = %d", i, P.vx[i]);
      CHECK(P.vaddr[i] >= EG * 16, "cut edge %zu addressed to a row slot", i);
    }
  CHECK(nvx == P.ncut, "vx names %lld cut edges of %d", nvx, P.ncut);
  // exact balance (member m owns vn[m NG, (m+1) NG) and cn[m MG, (m+1) MG)):
  // every uncut edge of a column addresses a row slot of its own member whose
  // row holds that column
  const int NG = P.NG, dv = L.dv_max, dc = L.dc_max;
  CHECK(NG * P.G == L.N && P.MG * P.G == L.M, "member sizes %d %d", NG, P.MG);
  for (int p = 0; p < L.N; p++)
    for (int k = 0; k < dv; k++) {
      if (P.vx[(size_t)p * dv + k] >= 0) continue;
      const int sl = P.vaddr[(size_t)p * dv + k] / 16, r = P.cn[(p / NG) * P.MG + sl / dc];
      bool has = false;
      for (int e = L.row_ptr[r]; e < L.row_ptr[r + 1]; e++) has |= L.row_col[e] == P.vn[p];
      CHECK(has, "column position %d edge %d: row %d of member %d does not hold it", p, k, r, p / NG);
    }
  // the refined cut (layout.cpp PartRefiner; the relabelling alone: 6,602)
  if (peg8064 && (!getenv("KML_PART_REFINE") || getenv("KML_PART_REFINE")[0] != '0'))
    CHECK(P.ncut <= (getenv("KML_PART_REFINE_ITERS") ? 6602 : 5700), "cut %d edges", P.ncut);
  for (int x = 0; x < P.ncut; x++) CHECK(seen_x[x] == 1, "mailbox index %d received %d times", x, seen_x[x]);
  // the plan fits the kernel (bp_coop.hip part_plan_fits: LDS with 7 dummy
  // slots, at most 2/3 of the edges cut, 2 x 1024 exchange entries per member)
  int xmax = 0;
  for (int m = 0; m < P.G; m++)
    xmax = std::max(xmax, std::max(P.xr_ptr[m + 1] - P.xr_ptr[m], P.xc_ptr[m + 1] - P.xc_ptr[m]));
  CHECK(((long long)P.MG * 6 + P.mirror_max + 7) * 16 + L.N <= 160 * 1024, "LDS: mirror_max %d", P.mirror_max);
  CHECK(3LL * P.ncut <= 2LL * L.E && xmax <= 2 * 1024, "cut %d, exchange list %d", P.ncut, xmax);
  printf("partition: %d of %d edges cut, mirror_max %d, interior %d, bank-conflict cost %lld -> %lld\n", P.ncut, L.E,
         P.mirror_max, P.interior, P.anneal_initial, P.anneal_final);
  digest_partition(P).print("partition", name);
}

// The partition plan depends on the refinement's schedule (KML_PART_REFINE,
// KML_PART_REFINE_ITERS), so the planner's cache is keyed on it: one process
// asks for the same code under its own schedule, a short one, none, and its own
// again, and gets each schedule's plan, not the first one made.  Prints
//   schedules <name>: ncut <own> <3000000 steps> <unrefined>
static void check_schedules(const LdpcCode &L, const char *name) {
  const char *vars[2] = {"KML_PART_REFINE", "KML_PART_REFINE_ITERS"};
  std::string own[2];
  bool own_set[2];
  for (int v = 0; v < 2; v++)
    if ((own_set[v] = getenv(vars[v]) != nullptr)) own[v] = getenv(vars[v]);
  auto plan_under = [&](const char *refine, const char *iters) {  // nullptr: the process's own value
    const char *val[2] = {refine, iters};
    for (int v = 0; v < 2; v++)
      if (val[v] || own_set[v])
        setenv(vars[v], val[v] ? val[v] : own[v].c_str(), 1);
      else
        unsetenv(vars[v]);
    PartitionPlan P;
    CHECK(plan_partition(L, 4, P), "plan_partition failed");
    return P;
  };
  const PartitionPlan a = plan_under(nullptr, nullptr), b = plan_under("1", "3000000"), c = plan_under("0", nullptr),
                      a2 = plan_under(nullptr, nullptr);
  CHECK(digest_partition(a2).h == digest_partition(a).h, "%s: the own schedule's plan changed", name);
  CHECK(digest_partition(b).h != digest_partition(c).h, "%s: refined and unrefined plans equal", name);
  CHECK(b.ncut < c.ncut, "%s: refined cut %d, unrefined %d", name, b.ncut, c.ncut);
  printf("schedules %s: ncut %d %d %d\n", name, a.ncut, b.ncut, c.ncut);
}

// A code that takes neither specialised plan: a regular code gets no irregular
// plan (the library makes one for non-regular codes only) and must not be a
// (3,6) code whose quarters tile the partitioned kernel ((N / 4) % 16 == 0
// beyond LDS); a non-regular one must be declined by plan_irregular or hold a
// degree the irregular kernel has no instance for (columns 1..9, rows 2..10).
// Whatever plan_irregular returns for it, it returns without a fault.
static void check_none(const LdpcCode &L, const char *name) {
  bool regular = true, in_range = true;
  for (int v = 0; v < L.N; v++) {
    regular &= col_deg(L, v) == L.dv_max;
    in_range &= col_deg(L, v) >= 1 && col_deg(L, v) <= 9;
  }
  for (int r = 0; r < L.M; r++) {
    regular &= row_deg(L, r) == L.dc_max;
    in_range &= row_deg(L, r) >= 2 && row_deg(L, r) <= 10;
  }
  IrregularPlan P;
  const bool irr = plan_irregular(L, kIrrThreads, kIrrVnPairMax, kIrrCnPairMax, P);
  if (regular) {
    const bool lds = (long long)L.E * 16 + 16 + L.N <= 160 * 1024;
    CHECK(L.N != 2304, "%s is a PEG2304-class code", name);
    CHECK(lds || L.dv_max != 3 || L.dc_max != 6 || L.N % 4 || L.M % 4 || (L.N / 4) % 16,
          "%s tiles the partitioned kernel", name);
  } else {
    CHECK(!irr || !in_range, "%s has an irregular plan and degrees the irregular kernel holds", name);
  }
  printf("none %s: regular %d, dv_max %d, dc_max %d, plan_irregular %d\n", name, (int)regular, L.dv_max, L.dc_max,
         (int)irr);
}

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  LdpcCode a, b, c;
  if (!load(a, argv[1], false) || !load(b, argv[2], true) || !load(c, argv[3], false)) return 2;
  check_regular(a, base_name(argv[1]));
  check_irregular(b, base_name(argv[2]));
  check_partition(c, base_name(argv[3]));
  for (int i = 4; i + 1 < argc; i += 2) {
    LdpcCode x;
    if (!load(x, argv[i + 1], false)) return 2;
    const char *name = base_name(argv[i + 1]);
    if (!strcmp(argv[i], "--regular")) {
      CHECK(x.dv_max == 3 && x.dc_max == 6 && x.N == 2304 && x.M == 1152, "%s is not a PEG2304-class code", name);
      check_regular(x, name);
    } else if (!strcmp(argv[i], "--irregular")) {
      check_irregular(x, name, true);
    } else if (!strcmp(argv[i], "--partition")) {
      check_partition(x, name, false);
      check_schedules(x, name);
    } else if (!strcmp(argv[i], "--none")) {
      check_none(x, name);
    } else {
      return 2;
    }
  }
  printf("plan_errors=%d\n", errors);
  return errors ? 1 : 0;
}
