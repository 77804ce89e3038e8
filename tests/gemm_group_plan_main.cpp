// Stand-alone check of the grouped GEMM launch planner (macaw_llm_amd/csrc/gemm_group_plan.h): host code only.
// tests/test_gemm_group_plan_cpu.py builds and runs it (once more with -fsanitize=address,undefined).
//
//   gemm_group_plan_main            every check, prints "OK <launches checked>" or the first failures; exit status 1 on failure
//   gemm_group_plan_main dump CUS   the plans of the cfg-3 layer sequence at CUS planned CUs, one line per launch
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

struct Filler { int tiles, nk, done; std::vector<int> hits; };
struct Launch { int main_tiles, main_nk; std::vector<Filler> add; bool drain; };
struct Stats { double heavy, light, t_max; long taken, left; };

// plans one launch over the queue `q` (fillers with tiles left, in order), marks the tiles it takes, checks the plan's shape
Stats run_launch(int n, const Launch& L, std::vector<Filler>& q, const char* what) {
  ++g_launches;
  for (const Filler& f : L.add) q.push_back(f);
  std::vector<Filler*> live;
  for (Filler& f : q) if (f.done < f.tiles) live.push_back(&f);
  if ((int)live.size() > mkgp::MAX_FILL) live.resize(mkgp::MAX_FILL);
  int rem[mkgp::MAX_FILL], nk[mkgp::MAX_FILL];
  const int nf = (int)live.size();
  Stats s{0, 1e30, 0, 0, 0};
  for (int i = 0; i < nf; ++i) { rem[i] = live[i]->tiles - live[i]->done; nk[i] = live[i]->nk; s.t_max = std::max(s.t_max, nk[i] + mkgp::TILE_C); }
  mkgp::Plan p;
  memset(&p, 0xee, sizeof p);
  const bool ok = mkgp::plan(n, L.main_tiles, L.main_nk, nf, rem, nk, L.drain, p);
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
  }
  CHECK(main_seen == L.main_tiles, "%s: main tiles %ld of %d", what, main_seen, L.main_tiles);
  for (int i = 0; i < nf; ++i) { live[i]->done += p.taken[i]; s.left += live[i]->tiles - live[i]->done; }
  s.taken = total;
  if (L.drain && (int)live.size() == nf) CHECK(s.left == 0, "%s: drain left %ld tiles", what, s.left);
  return s;
}

Filler filler(int tiles, int nk) { return Filler{tiles, nk, 0, std::vector<int>(tiles, 0)}; }

void every_tile_once(const std::vector<Filler>& q, const char* what) {
  for (size_t i = 0; i < q.size(); ++i) {
    CHECK(q[i].done == q[i].tiles, "%s: filler %zu has %d of %d tiles", what, i, q[i].done, q[i].tiles);
    for (int t = 0; t < q[i].tiles; ++t) CHECK(q[i].hits[t] == 1, "%s: filler %zu tile %d run %d times", what, i, t, q[i].hits[t]);
  }
}

// the backward of one cfg-3 decoder layer (B S = 4608, D = 4096, FF = 11008): dx(down) with dW(down) queued, dx(gate|up)
// with dW(gate|up), dx(o) with dW(o), dx(q|k|v) with dW(q|k|v) and drain
std::vector<Launch> cfg3_layer() {
  return {{774, 64, {filler(688, 72)}, false},
          {288, 344, {filler(1376, 72)}, false},
          {288, 64, {filler(256, 72)}, false},
          {288, 192, {filler(768, 72)}, true}};
}

void check_cfg3(int n, bool dump) {
  std::vector<Filler> q;
  int i = 0;
  for (const Launch& L : cfg3_layer()) {
    char what[64];
    snprintf(what, sizeof what, "cfg3 @%d launch %d", n, ++i);
    const Stats s = run_launch(n, L, q, what);
    if (dump) printf("%s: main %d x %d, took %ld, left %ld, heaviest %.1f lightest %.1f (K-tiles)\n", what, L.main_tiles, L.main_nk, s.taken, s.left, s.heavy, s.light);
    // enough is queued at every launch of this sequence: heaviest - lightest <= one filler tile
    CHECK(s.heavy - s.light <= s.t_max + 1e-6, "%s: spread %.2f > %.2f", what, s.heavy - s.light, s.t_max);
    if (!L.drain) CHECK(s.left > 0, "%s: a balancing launch used the queue up", what);
  }
  every_tile_once(q, "cfg3");
}

uint32_t g_rng = 1;
int rnd(int lo, int hi) { g_rng = g_rng * 1664525u + 1013904223u; return lo + (int)((g_rng >> 8) % (uint32_t)(hi - lo + 1)); }

void check_random(uint32_t seed, bool one_k) {
  g_rng = seed * 2654435761u + 12345u;
  const int n = 8, launches = rnd(1, 4), k_all = rnd(2, 12);
  std::vector<Filler> q;
  for (int i = 0; i < launches; ++i) {
    Launch L{rnd(0, 4) == 0 ? 0 : rnd(1, 40), rnd(2, 12), {}, i == launches - 1};
    const int adds = rnd(0, 2);
    for (int a = 0; a < adds; ++a) L.add.push_back(filler(rnd(0, 60), one_k ? k_all : rnd(2, 12)));
    long queued = 0;
    double gaps = 0, heavy = 0;
    for (const Filler& f : q) queued += f.tiles - f.done;
    for (const Filler& f : L.add) queued += f.tiles;
    for (int b = 0; b < n; ++b) heavy = std::max(heavy, mkgp::main_tiles_of(b, n, L.main_tiles) * (L.main_nk + mkgp::TILE_C));
    for (int b = 0; b < n; ++b) gaps += heavy - mkgp::main_tiles_of(b, n, L.main_tiles) * (L.main_nk + mkgp::TILE_C);
    double queued_cost = 0;
    for (const Filler& f : q) queued_cost += (f.tiles - f.done) * (f.nk + mkgp::TILE_C);
    for (const Filler& f : L.add) queued_cost += f.tiles * (f.nk + mkgp::TILE_C);
    char what[64];
    snprintf(what, sizeof what, "seed %u%s launch %d", seed, one_k ? " (one K)" : "", i);
    const Stats s = run_launch(n, L, q, what);
    // "enough fillers queued": the queue can lift every workgroup to the heaviest one's main cost and one tile beyond
    const bool enough = queued_cost >= gaps + n * s.t_max;
    if (enough && (L.drain || L.main_tiles > 0)) CHECK(s.heavy - s.light <= s.t_max + 1e-6, "%s: spread %.2f > %.2f", what, s.heavy - s.light, s.t_max);
    if (!L.drain && L.main_tiles > 0 && s.left > 0)   // a balancing launch never raises the launch's length by more than half a tile
      CHECK(s.heavy <= heavy + 0.5 * s.t_max + 1e-6, "%s: heaviest %.2f over main %.2f", what, s.heavy, heavy);
  }
  every_tile_once(q, "random");
}
}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "dump")) { check_cfg3(atoi(argv[2]), true); return g_fail != 0; }
  check_cfg3(256, false);
  check_cfg3(240, false);
  // workgroups without any work are legal: 3 main tiles on 8 workgroups, nothing queued; and nothing at all
  {
    std::vector<Filler> q;
    const Stats s = run_launch(8, Launch{3, 4, {}, false}, q, "idle workgroups");
    CHECK(s.taken == 0 && s.light == 0, "idle workgroups: took %ld", s.taken);
    run_launch(8, Launch{0, 4, {}, true}, q, "empty launch");
    // fewer fillers than idle workgroups: all taken, one each at the most
    q.push_back(filler(3, 12));
    const Stats f = run_launch(8, Launch{9, 3, {}, false}, q, "few fillers");
    CHECK(f.taken == 3 && f.left == 0 && f.heavy <= (3 + mkgp::TILE_C) + (12 + mkgp::TILE_C) + 1e-6, "few fillers: took %ld, heaviest %.1f", f.taken, f.heavy);
    // whole rounds of main tiles: a balancing launch takes nothing
    q.push_back(filler(5, 12));
    const Stats w = run_launch(8, Launch{16, 3, {}, false}, q, "whole rounds");
    CHECK(w.taken == 0 && w.left == 5, "whole rounds: took %ld", w.taken);
    // no main problem: whole rounds of the queue without drain, everything with it
    q.push_back(filler(22, 12));
    const Stats g = run_launch(8, Launch{0, 0, {}, false}, q, "filler only");
    CHECK(g.taken == 24 && g.heavy == g.light, "filler only: took %ld", g.taken);
    run_launch(8, Launch{0, 0, {}, true}, q, "filler only, drain");
    every_tile_once(q, "edge cases");
  }
  mkgp::Plan p;
  int rem[1] = {70000}, nk[1] = {4};
  CHECK(!mkgp::plan(8, 0, 0, 1, rem, nk, true, p), "more tiles than a run index holds must be refused");
  CHECK(!mkgp::plan(mkgp::MAX_WG + 1, 0, 0, 0, rem, nk, true, p), "too many workgroups must be refused");
  for (uint32_t seed = 1; seed <= 400; ++seed) { check_random(seed, true); check_random(seed, false); }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("OK %d\n", g_launches);
  return 0;
}
