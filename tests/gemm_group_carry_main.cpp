// Stand-alone check of the grouped GEMM planner's carry mode (mkgp::plan_carry, macaw_llm_amd/csrc/gemm_group_plan.h): host code only.
// tests/test_gemm_group_carry_cpu.py builds and runs it (once more with -fsanitize=address,undefined).
//
//   gemm_group_carry_main            every check, prints "OK <launches checked>" or the first failures; exit status 1 on failure
//   gemm_group_carry_main dump CUS   32 cfg-3 layers at CUS planned CUs, carried and drained per layer, one line per launch
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../macaw_llm_amd/csrc/gemm_group_plan.h"

namespace {
int g_fail = 0, g_launches = 0;
#define CHECK(COND, ...)                                        \
  do {                                                          \
    if (!(COND)) {                                              \
      if (g_fail++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    }                                                           \
  } while (0)

enum Mode { BALANCE = 0, DRAIN = 1, CARRY = 2 };
struct Filler { int tiles, nk, done; std::vector<int> hits; };
struct Launch { int main_tiles, main_nk; std::vector<Filler> add; int mode; };
struct Stats { double heavy, light, t_max, idle; long taken, left; int live; mkgp::Plan plan; };

// plans one launch over the queue `q` (fillers with tiles left, in order), marks the tiles it takes, checks the plan's shape
// (gemm_group_plan_main.cpp's helper with the mode as a number, the launch's idle time and the count of live problems)
Stats run_launch(int n, const Launch& L, std::vector<Filler>& q, const char* what) {
  ++g_launches;
  for (const Filler& f : L.add) q.push_back(f);
  std::vector<Filler*> live;
  for (Filler& f : q) if (f.done < f.tiles) live.push_back(&f);
  Stats s{0, 1e30, 0, 0, 0, 0, (int)live.size(), {}};
  if ((int)live.size() > mkgp::MAX_FILL) live.resize(mkgp::MAX_FILL);
  int rem[mkgp::MAX_FILL], nk[mkgp::MAX_FILL];
  const int nf = (int)live.size();
  for (int i = 0; i < nf; ++i) { rem[i] = live[i]->tiles - live[i]->done; nk[i] = live[i]->nk; s.t_max = std::max(s.t_max, nk[i] + mkgp::TILE_C); }
  mkgp::Plan& p = s.plan;
  memset(&p, 0xee, sizeof p);
  const bool ok = L.mode == CARRY ? mkgp::plan_carry(n, L.main_tiles, L.main_nk, nf, rem, nk, p)
                                  : mkgp::plan(n, L.main_tiles, L.main_nk, nf, rem, nk, L.mode == DRAIN, p);
  CHECK(ok, "%s: plan refused", what);
  if (!ok) return s;
  // the taken tiles are a prefix of the queue
  long total = 0;
  bool partial = false;
  for (int i = 0; i < nf; ++i) {
    CHECK(p.taken[i] >= 0 && p.taken[i] <= rem[i], "%s: taken[%d] = %d of %d", what, i, p.taken[i], rem[i]);
    CHECK(!partial || p.taken[i] == 0, "%s: filler %d taken behind a partly taken one", what, i);
    if (p.taken[i] < rem[i]) partial = true;
    total += p.taken[i];
  }
  for (int i = nf; i < mkgp::MAX_FILL; ++i) CHECK(p.taken[i] == 0, "%s: taken[%d] set", what, i);
  CHECK(p.start[0] == 0 && p.start[n] == total, "%s: runs cover %d .. %d of %ld", what, p.start[0], p.start[n], total);
  // every workgroup: its main tiles b, b + n, ... and its filler tiles as wg_tile deals them; cost as the planner prices it
  long main_seen = 0;
  double sum = 0;
  std::vector<char> rank_seen(n, 0);
  for (int b = 0; b < n; ++b) {
    const int r = mkgp::wg_rank(b, n);
    CHECK(r >= 0 && r < n && !rank_seen[r] && mkgp::wg_of_rank(r, n) == b, "%s: rank of %d", what, b);
    if (r < 0 || r >= n) continue;
    rank_seen[r] = 1;
    const int mt = mkgp::main_tiles_of(b, n, L.main_tiles);
    main_seen += mt;
    double c = mt * (L.main_nk + mkgp::TILE_C);
    CHECK(p.start[r] <= p.start[r + 1], "%s: run of rank %d", what, r);
    for (int j = 0; j < p.start[r + 1] - p.start[r]; ++j) {
      const int x = mkgp::wg_tile(p.start, n, r, j);
      CHECK(x >= p.start[0] && x < p.start[n], "%s: tile %d of rank %d is index %d", what, j, r, x);
      int f = 0, at = x;
      while (f < nf && at >= p.taken[f]) at -= p.taken[f++];
      CHECK(f < nf, "%s: index %d past the taken tiles", what, x);
      if (f >= nf) break;
      live[f]->hits[live[f]->done + at]++;
      c += live[f]->nk + mkgp::TILE_C;
    }
    s.heavy = std::max(s.heavy, c);
    s.light = std::min(s.light, c);
    sum += c;
  }
  s.idle = s.heavy * n - sum;
  CHECK(main_seen == L.main_tiles, "%s: main tiles %ld of %d", what, main_seen, L.main_tiles);
  for (int i = 0; i < nf; ++i) { live[i]->done += p.taken[i]; s.left += live[i]->tiles - live[i]->done; }
  s.taken = total;
  if (L.mode == DRAIN && s.live == nf) CHECK(s.left == 0, "%s: drain left %ld tiles", what, s.left);
  return s;
}

Filler filler(int tiles, int nk) { return Filler{tiles, nk, 0, std::vector<int>(tiles, 0)}; }

void every_tile_once(const std::vector<Filler>& q, const char* what) {
  for (size_t i = 0; i < q.size(); ++i) {
    CHECK(q[i].done == q[i].tiles, "%s: filler %zu has %d of %d tiles", what, i, q[i].done, q[i].tiles);
    for (int t = 0; t < q[i].tiles; ++t) CHECK(q[i].hits[t] == 1, "%s: filler %zu tile %d run %d times", what, i, t, q[i].hits[t]);
  }
}

bool same_plan(const mkgp::Plan& a, const mkgp::Plan& b, int n) {
  return !memcmp(a.taken, b.taken, sizeof a.taken) && !memcmp(a.start, b.start, (n + 1) * sizeof a.start[0]);
}

// the backward of one cfg-3 decoder layer (gemm_group_plan_main.cpp); `last` is the mode of its dx(q|k|v) launch, the other
// three launches balance where that one drains and carry where it carries
std::vector<Launch> cfg3_layer(int last) {
  const int m = last == CARRY ? CARRY : BALANCE;
  return {{774, 64, {filler(688, 72)}, m}, {288, 344, {filler(1376, 72)}, m}, {288, 64, {filler(256, 72)}, m},
          {288, 192, {filler(768, 72)}, last}};
}

// 32 layers and a final flush; returns the sum over all launches of the heaviest workgroup's price
double cfg3_sequence(int n, int last, bool dump) {
  std::vector<Filler> q;
  double length = 0;
  for (int layer = 0; layer <= 32; ++layer) {
    const std::vector<Launch> ls = layer < 32 ? cfg3_layer(last) : std::vector<Launch>{{0, 0, {}, DRAIN}};
    int i = 0;
    for (const Launch& L : ls) {
      char what[64];
      snprintf(what, sizeof what, "cfg3 @%d %s layer %d launch %d", n, last == CARRY ? "carry" : "drain", layer, ++i);
      const Stats s = run_launch(n, L, q, what);
      length += s.heavy;
      if (dump) printf("%s: main %d x %d, took %ld, left %ld, live %d, heaviest %.1f idle %.0f (K-tiles)\n", what, L.main_tiles, L.main_nk, s.taken, s.left, s.live, s.heavy, s.idle);
      CHECK(s.live <= mkgp::MAX_FILL, "%s: %d live problems", what, s.live);
      if (L.mode == CARRY) {
        // never short of fillers: the launch is not the fallback (which uses the queue up), and it ends within one tile
        CHECK(s.left > 0, "%s: the queue ran dry", what);
        CHECK(s.heavy - s.light <= s.t_max + 1e-6, "%s: spread %.2f", what, s.heavy - s.light);
        CHECK(s.left <= 3 * n / 2, "%s: backlog %ld", what, s.left);
      }
    }
  }
  every_tile_once(q, "cfg3 sequence");
  return length;
}

void check_cfg3(int n, double bound, bool dump) {
  const double today = cfg3_sequence(n, DRAIN, dump), carry = cfg3_sequence(n, CARRY, dump);
  printf("cfg3 @%d: 32 layers drained per layer %.1f, carried %.1f K-tiles: ratio %.4f\n", n, today, carry, carry / today);
  CHECK(carry <= bound * today, "cfg3 @%d: carried %.1f against %.1f (ratio %.4f > %.3f)", n, carry, today, carry / today, bound);
}

uint32_t g_rng = 1;
int rnd(int lo, int hi) { g_rng = g_rng * 1664525u + 1013904223u; return lo + (int)((g_rng >> 8) % (uint32_t)(hi - lo + 1)); }

// least idle by brute force: a filler count per class of main cost (ka for the workgroups with the most main tiles, kb for
// the others), priced through wg_tile, over every pair whose heaviest workgroup lies in [lmain, lmain + t_max)
double brute_least_idle(int n, const Launch& L, const std::vector<Filler>& q, double t_max) {
  std::vector<double> tile_cost;          // the queue laid end to end
  for (const Filler& f : q) for (int t = f.done; t < f.tiles; ++t) tile_cost.push_back(f.nk + mkgp::TILE_C);
  std::vector<double> mc(n);
  double lmain = 0;
  for (int r = 0; r < n; ++r) { mc[r] = mkgp::main_tiles_of(mkgp::wg_of_rank(r, n), n, L.main_tiles) * (L.main_nk + mkgp::TILE_C); lmain = std::max(lmain, mc[r]); }
  double best = 1e300;
  for (int ka = 0; ka <= 12; ++ka)
    for (int kb = 0; kb <= 40; ++kb) {
      std::vector<uint16_t> start(n + 1, 0);
      for (int r = 0; r < n; ++r) start[r + 1] = (uint16_t)(start[r] + (mc[r] < lmain ? kb : ka));
      if (start[n] > tile_cost.size()) continue;
      double heavy = 0, sum = 0;
      for (int r = 0; r < n; ++r) {
        double c = mc[r];
        for (int j = 0; j < start[r + 1] - start[r]; ++j) c += tile_cost[mkgp::wg_tile(start.data(), n, r, j)];
        heavy = std::max(heavy, c);
        sum += c;
      }
      if (heavy < lmain - 1e-9 || heavy >= lmain + t_max - 1e-9) continue;
      best = std::min(best, heavy * n - sum);
    }
  return best;
}

void check_least_idle(uint32_t seed, bool one_k) {
  g_rng = seed * 2654435761u + 777u;
  const int n = 8, k_all = rnd(2, 12);
  Launch L{rnd(1, 40), rnd(2, 12), {}, CARRY};
  std::vector<Filler> q;
  double gaps = 0, heavy = 0, queued_cost = 0;
  for (int b = 0; b < n; ++b) heavy = std::max(heavy, mkgp::main_tiles_of(b, n, L.main_tiles) * (L.main_nk + mkgp::TILE_C));
  for (int b = 0; b < n; ++b) gaps += heavy - mkgp::main_tiles_of(b, n, L.main_tiles) * (L.main_nk + mkgp::TILE_C);
  const double t_most = 12 + mkgp::TILE_C;
  while ((int)q.size() < mkgp::MAX_FILL && (queued_cost < gaps + 2 * n * t_most || (int)q.size() < 2)) {
    q.push_back(filler(rnd(1, 60), one_k ? k_all : rnd(2, 12)));
    queued_cost += q.back().tiles * (q.back().nk + mkgp::TILE_C);
  }
  if (queued_cost < gaps + 2 * n * t_most) return;      // (eight short fillers: not the case under test)
  double t_max = 0;
  for (const Filler& f : q) t_max = std::max(t_max, f.nk + mkgp::TILE_C);
  const double least = brute_least_idle(n, L, q, t_max);
  char what[64];
  snprintf(what, sizeof what, "least idle, seed %u%s", seed, one_k ? " (one K)" : "");
  const Stats s = run_launch(n, L, q, what);
  CHECK(s.heavy >= heavy - 1e-9, "%s: level %.2f under the main's %.2f", what, s.heavy, heavy);
  if (one_k) CHECK(std::fabs(s.idle - least) < 1e-6, "%s: idle %.3f, least %.3f", what, s.idle, least);
  else CHECK(s.idle > least - 1e-6 && s.idle < least + t_max, "%s: idle %.3f, least %.3f, t_max %.2f", what, s.idle, least, t_max);
  // one K: the backlog is steered to within half a round of one tile per workgroup (the queue holds two rounds beyond the gaps)
  if (one_k) CHECK(s.left >= n / 2 && s.left <= 3 * n / 2, "%s: backlog %ld", what, s.left);
  run_launch(n, Launch{0, 0, {}, DRAIN}, q, what);
  every_tile_once(q, what);
}

// too little queued to lift the workgroups to the main's level: the plan of today's balance mode (which then drains)
void check_short_queue(uint32_t seed) {
  g_rng = seed * 2654435761u + 4242u;
  const int n = 8;
  Launch L{rnd(1, 7) + 8 * rnd(0, 3), rnd(6, 12), {}, CARRY};     // a partial last round
  const int missing = n - L.main_tiles % n;                       // workgroups one main tile short
  std::vector<Filler> q1, q2;
  const int tiles = rnd(0, std::max(0, missing / 2)), nk = rnd(2, 5);   // fewer tiles than gaps, each shorter than a main tile
  q1.push_back(filler(tiles, nk));
  q2.push_back(filler(tiles, nk));
  char what[64];
  snprintf(what, sizeof what, "short queue, seed %u", seed);
  const Stats a = run_launch(n, L, q1, what);
  L.mode = BALANCE;
  const Stats b = run_launch(n, L, q2, what);
  CHECK(same_plan(a.plan, b.plan, n) && a.left == 0, "%s: carry took %ld, balance %ld", what, a.taken, b.taken);
  every_tile_once(q1, what);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "dump")) { check_cfg3(atoi(argv[2]), 1.0, true); return g_fail != 0; }
  // 256: 1874.0 / 1934.1 = 0.969 per layer in steady state, the first layer and the final flush cost under 0.2 % of 32 layers
  check_cfg3(256, 0.975, false);
  check_cfg3(248, 1.0, false);
  check_cfg3(240, 1.0, false);
  {
    // no main problem: today's filler-only balance (whole rounds); whole rounds of main tiles: no idle time at any level,
    // so the launch only steers the backlog (29 queued, 8 workgroups: 3 tiles each leave 5, nearer 8 than 13 is)
    std::vector<Filler> q{filler(5, 12), filler(22, 12)};
    const Stats g = run_launch(8, Launch{0, 0, {}, CARRY}, q, "filler only");
    CHECK(g.taken == 24 && g.heavy == g.light, "filler only: took %ld", g.taken);
    q.push_back(filler(26, 12));
    const Stats w = run_launch(8, Launch{16, 3, {}, CARRY}, q, "whole rounds");
    CHECK(w.idle < 1e-9 && w.taken == 24 && w.left == 5, "whole rounds: took %ld, idle %.2f", w.taken, w.idle);
    // nothing queued, and idle workgroups with nothing queued
    std::vector<Filler> none;
    const Stats e = run_launch(8, Launch{3, 4, {}, CARRY}, none, "nothing queued");
    CHECK(e.taken == 0 && e.light == 0, "nothing queued: took %ld", e.taken);
    run_launch(8, Launch{0, 0, {}, DRAIN}, q, "flush");
    every_tile_once(q, "edge cases");
  }
  mkgp::Plan p;
  int rem[1] = {70000}, nk[1] = {4};
  CHECK(!mkgp::plan_carry(8, 9, 4, 1, rem, nk, p), "more tiles than a run index holds must be refused");
  CHECK(!mkgp::plan_carry(mkgp::MAX_WG + 1, 9, 4, 0, rem, nk, p), "too many workgroups must be refused");
  for (uint32_t seed = 1; seed <= 400; ++seed) { check_least_idle(seed, true); check_least_idle(seed, false); check_short_queue(seed); }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("OK %d\n", g_launches);
  return 0;
}
