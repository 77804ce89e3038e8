// Work plan of a grouped GEMM launch (mk_gemm_grouped): which filler tiles each persistent workgroup runs behind its main
// tiles.  Pure host code without HIP, so that it is tested on the CPU (tests/gemm_group_plan_main.cpp).
//
// One workgroup per planned CU.  Workgroup b runs the main tiles b, b + n, ... and then a number of filler tiles; the
// fillers' remaining tiles are laid end to end in queue order.  The map from workgroup to filler tile:
//   * the hardware sends workgroup b to XCD b % 8, so rank = (b % 8) * (n / 8) + b / 8 puts the workgroups of one XCD
//     side by side; they form a GROUP (n % 8 != 0: rank = b and groups of 64), and a group owns ONE contiguous span of
//     the laid-out tiles, as long as the sum of its members' counts;
//   * inside the group the span is dealt round by round: in round j the members that still have a j-th tile take the
//     next indices in rank order (wg_tile);
//   * a filler's tile order is tile_from_index with 8-row groups (no xcd_remap: the rank does that job).
// So the tiles that the workgroups of an XCD compute at the same time are up to n / 8 CONSECUTIVE tiles of a filler: a
// compact block 8 tile rows high whose operand panels the XCD's L2 holds once -- what xcd_remap + tile_from_index give
// an ordinary round.  (Measured, profiles/dw_fill_cfg3.txt: with one contiguous run per workgroup instead, concurrent
// tiles of an XCD lie a run length apart and share almost no panel; the draining launch ran 14 % over its price.)
//
// Cost of a tile: K-tiles + TILE_C, in units of one K-tile's time.  TILE_C = 9.4 / 1.38 is the fixed 9.4 us per tile
// over the 1.38 us per K-tile of the v9 loop (profiles/r06_gemm_v9_mfma16.txt; gemm_v9.hip header).
//
// Rule: a workgroup takes tiles while that brings its cost closer to the level L.
//   balance (no drain): L = the heaviest workgroup's main cost.  Whatever the queue still holds stays queued.  Without
//            a main problem L is the queue's cost per workgroup and a tile is taken only if it fits under L (whole rounds).
//   drain:   the highest L at which the queue is not used up (bisection), then the remaining tiles (fewer than one
//            per workgroup when all fillers share one K) go one each to the lightest workgroups.  With fillers of
//            different K the counts are then priced as dealt and single tiles moved from the heaviest to the lightest
//            workgroup while the two differ by more than a tile.
//   carry:   (plan_carry) the queue lives on behind the launch, so the level is free: the L >= lmain of least idle
//            time, moved by whole tiles per workgroup to keep about one tile per workgroup queued.
// Limitation: the level pass prices a workgroup as if it took its tiles in one run along the queue, while wg_tile deals
// a group's span round by round.  With one K for everything a launch takes (every decoder layer: K = tokens / 64) the
// two are the same; where a balancing launch's span crosses fillers of different K, a workgroup's real cost differs
// from the balanced one by at most (its tile count) x (the K difference).  Only the drain branch re-prices as dealt.
// A balance launch whose queue runs dry at its level is planned as a drain.  While the queue lasts every workgroup
// ends within half a filler tile of L, so the heaviest and the lightest differ by at most one filler tile's cost.
#pragma once
#include <algorithm>
#include <cstdint>

namespace mkgp {

constexpr int MAX_FILL = 8, MAX_WG = 320;
constexpr double TILE_C = 9.4 / 1.38;

struct Plan {
  int taken[MAX_FILL];            // tiles of each filler this launch runs (from its first remaining tile on)
  uint16_t start[MAX_WG + 1];     // by rank: the workgroup runs start[r + 1] - start[r] filler tiles (which ones: wg_tile)
};

inline int wg_rank(int b, int n) { return (n & 7) == 0 ? (b & 7) * (n >> 3) + (b >> 3) : b; }
inline int wg_of_rank(int r, int n) { return (n & 7) == 0 ? (r % (n >> 3)) * 8 + r / (n >> 3) : r; }
inline int main_tiles_of(int b, int n, int tiles) { return b < tiles ? (tiles - b + n - 1) / n : 0; }
inline int group_width(int n) { return (n & 7) == 0 ? n >> 3 : 64; }
// index, in the taken tiles laid end to end, of the j-th filler tile of the workgroup of rank r (-1: it has none)
inline int wg_tile(const uint16_t* start, int n, int r, int j) {
  const int W = group_width(n), g0 = r / W * W, g1 = std::min(n, g0 + W);
  if (j < 0 || j >= start[r + 1] - start[r]) return -1;
  int at = start[g0];
  for (int jj = 0; jj <= j; ++jj)
    for (int i = g0; i < (jj == j ? r : g1); ++i) at += start[i + 1] - start[i] > jj;
  return at;
}

namespace detail {
// one pass in rank order at level L; bias 0.5 = nearest, 0 = only what fits.  cnt / cost by rank.  Returns tiles taken.
inline long pass(int n, const double* main_cost, int n_fill, const int* rem, const int* nk, double L, double bias, int* cnt,
                 double* cost) {
  int f = 0, left = n_fill > 0 ? rem[0] : 0;
  long total = 0;
  for (int r = 0; r < n; ++r) {
    double c = main_cost[r];
    int k = 0;
    while (f < n_fill) {
      if (left == 0) { if (++f < n_fill) left = rem[f]; continue; }
      const double t = nk[f] + TILE_C;
      const double room = (L - c) / t + bias;
      int take = room <= 0 ? 0 : room >= left ? left : (int)room;
      c += take * t; k += take; left -= take;
      if (left > 0) break;
    }
    cnt[r] = k; cost[r] = c; total += k;
  }
  return total;
}
// cost by rank of cnt[r] filler tiles each, dealt as wg_tile deals them
inline void price(int n, const double* main_cost, int n_fill, const int* rem, const int* nk, const int* cnt, double* cost) {
  const int W = group_width(n);
  int f = 0, left = n_fill > 0 ? rem[0] : 0;
  for (int g0 = 0; g0 < n; g0 += W) {
    const int g1 = std::min(n, g0 + W);
    for (int r = g0; r < g1; ++r) cost[r] = main_cost[r];
    for (int j = 0, any = 1; any; ++j) {
      any = 0;
      for (int r = g0; r < g1; ++r) {
        if (cnt[r] <= j) continue;
        while (f < n_fill && left == 0) if (++f < n_fill) left = rem[f];
        if (f >= n_fill) return;
        cost[r] += nk[f] + TILE_C; --left; any = 1;
      }
    }
  }
}
// the plan of cnt[r] filler tiles for the workgroup of rank r: the runs, and the queue's prefix that they cover
inline void emit(int n_wg, int n_fill, const int* rem, const int* cnt, Plan& out) {
  long at = 0;
  for (int r = 0; r < n_wg; ++r) { out.start[r] = (uint16_t)at; at += cnt[r]; }
  for (int r = n_wg; r <= MAX_WG; ++r) out.start[r] = (uint16_t)at;
  long rest = at;
  for (int i = 0; i < MAX_FILL; ++i) {
    out.taken[i] = i < n_fill ? (int)std::min<long>(rest, rem[i]) : 0;
    rest -= out.taken[i];
  }
}
}  // namespace detail

// n_wg workgroups, a main problem of main_tiles tiles of main_nk K-tiles (0 tiles: none), fillers with rem[i] remaining
// tiles of nk[i] K-tiles.  False when the launch cannot be described (too many workgroups, fillers or tiles).
inline bool plan(int n_wg, int main_tiles, int main_nk, int n_fill, const int* rem, const int* nk, bool drain, Plan& out) {
  if (n_wg < 1 || n_wg > MAX_WG || n_fill < 0 || n_fill > MAX_FILL || main_tiles < 0) return false;
  long queued = 0;
  double queued_cost = 0, t_last = 0;
  for (int i = 0; i < n_fill; ++i) {
    if (rem[i] < 0 || nk[i] < 1) return false;
    queued += rem[i];
    queued_cost += rem[i] * (nk[i] + TILE_C);
    if (rem[i] > 0) t_last = nk[i] + TILE_C;
  }
  if (queued > 65535) return false;
  double main_cost[MAX_WG], cost[MAX_WG];
  int cnt[MAX_WG];
  double lmain = 0;
  for (int r = 0; r < n_wg; ++r) {
    main_cost[r] = main_tiles_of(wg_of_rank(r, n_wg), n_wg, main_tiles) * (main_nk + TILE_C);
    lmain = std::max(lmain, main_cost[r]);
  }
  long got = 0;
  bool level_plan = false;
  if (!drain) {
    got = main_tiles > 0 ? detail::pass(n_wg, main_cost, n_fill, rem, nk, lmain, 0.5, cnt, cost)
                         : detail::pass(n_wg, main_cost, n_fill, rem, nk, queued_cost / n_wg, 0.0, cnt, cost);
    level_plan = got < queued || main_tiles == 0;
  }
  if (!level_plan) {
    // drain: the highest level that does not use the queue up, then the rest one each to the lightest workgroups
    double lo = 0, hi = lmain + queued_cost + 1;
    for (int it = 0; it < 48 && queued > 0; ++it) {
      const double mid = 0.5 * (lo + hi);
      if (detail::pass(n_wg, main_cost, n_fill, rem, nk, mid, 0.5, cnt, cost) < queued) lo = mid; else hi = mid;
    }
    got = detail::pass(n_wg, main_cost, n_fill, rem, nk, lo, 0.5, cnt, cost);
    int order[MAX_WG];
    while (got < queued) {
      for (int r = 0; r < n_wg; ++r) order[r] = r;
      std::stable_sort(order, order + n_wg, [&](int a, int b) { return cost[a] < cost[b]; });
      for (int i = 0; i < n_wg && got < queued; ++i, ++got) { ++cnt[order[i]]; cost[order[i]] += t_last; }
    }
    // fillers of different K: handing out the rest moved every later run along the queue, so price the runs as they
    // are now and move single tiles from the heaviest to the lightest workgroup while that still helps
    double t_max = 0;
    for (int i = 0; i < n_fill; ++i) if (rem[i] > 0) t_max = std::max(t_max, nk[i] + TILE_C);
    for (int it = 0; it < 4 * n_wg; ++it) {
      detail::price(n_wg, main_cost, n_fill, rem, nk, cnt, cost);
      int h = -1, l = 0;
      for (int r = 0; r < n_wg; ++r) {
        if (cnt[r] > 0 && (h < 0 || cost[r] > cost[h])) h = r;
        if (cost[r] < cost[l]) l = r;
      }
      if (h < 0 || cost[h] - cost[l] <= t_max) break;
      --cnt[h]; ++cnt[l];
    }
  }
  detail::emit(n_wg, n_fill, rem, cnt, out);
  return true;
}

// Tiles that a carrying launch aims to leave queued: one per workgroup.  A level moves in steps of one tile per
// workgroup, so the backlog lands within n_wg / 2 of this wherever the queue allows it: between n_wg / 2 and 3 n_wg / 2
// tiles.  Why one: in the decoder every grad-input launch has its own grad-weight GEMM queued in front of it, and that
// one alone holds more tiles than the launch's least-idle level needs (cfg 3 at 256: 688 for 250, 1376 for 1120, 256
// for 224, 768 for 672), so no backlog at all would already do; one tile per workgroup is the margin for a launch
// whose own filler is short, and it ends the step with a single filler-only round.  It is far from the limits: at
// most 3 n_wg / 2 tiles lie in two or three problems of a decoder layer (MAX_FILL = 8 live ones, 65535 tiles), and the
// operands they keep alive are those of the layer just left (tests/gemm_group_carry_main.cpp walks 32 layers).
inline int carry_target(int n_wg) { return n_wg; }

// carry: the queue outlives the launch (it is shared by the layers of a backward pass), so the launch is free to end at any
// level L >= lmain and takes the one that costs the least idle time, sum over workgroups of (heaviest - cost), priced as
// dealt.  The workgroups come in at most two classes of main cost (q or q + 1 main tiles); a plan is a filler count per
// class, kA for the heavier and kB for the lighter one, and every pair whose level can lie in [lmain, lmain + t_max) is
// priced.  Fillers of one K (every decoder layer): kA = 0 and kB = floor or ceil of the gap in tiles, and adding s tiles
// to every workgroup leaves the idle time as it is, so s >= 0 is chosen to bring the backlog nearest carry_target().
// Fillers of different K: the pairs are priced as dealt and ties go to the backlog nearest the target; no shift (its
// price would depend on what lies further along the queue).
// Without a main problem, and where today's balance uses the queue up, the plan is that of plan(..., drain = false, ...).
inline bool plan_carry(int n_wg, int main_tiles, int main_nk, int n_fill, const int* rem, const int* nk, Plan& out) {
  if (!plan(n_wg, main_tiles, main_nk, n_fill, rem, nk, false, out)) return false;
  long queued = 0;
  double t_min = 1e30, t_max = 0;
  for (int i = 0; i < n_fill; ++i) {
    queued += rem[i];
    if (rem[i] > 0) { t_min = std::min(t_min, nk[i] + TILE_C); t_max = std::max(t_max, nk[i] + TILE_C); }
  }
  if (main_tiles == 0 || out.start[n_wg] >= queued) return true;
  double main_cost[MAX_WG], cost[MAX_WG];
  int cnt[MAX_WG];
  double lmain = 0, lmin = 1e30;
  for (int r = 0; r < n_wg; ++r) {
    main_cost[r] = main_tiles_of(wg_of_rank(r, n_wg), n_wg, main_tiles) * (main_nk + TILE_C);
    lmain = std::max(lmain, main_cost[r]);
    lmin = std::min(lmin, main_cost[r]);
  }
  int n_light = 0;
  for (int r = 0; r < n_wg; ++r) n_light += main_cost[r] < lmain;
  const int n_heavy = n_wg - n_light;
  const double gap = lmain - lmin, eps = 1e-9;
  const bool one_k = t_max - t_min < eps;
  const long target = carry_target(n_wg);
  const auto dist = [&](long taken) { const long d = queued - taken - target; return d < 0 ? -d : d; };
  double best = 1e300;
  long best_taken = 0;
  int best_a = 0, best_b = 0;
  for (int ka = 0; ka * t_min < t_max - eps; ++ka) {
    for (int kb = one_k ? (int)(gap / t_min + eps) : 0; lmin + kb * t_min < lmain + t_max - eps; ++kb) {
      if (n_light == 0 && kb > 0) break;
      const long taken = (long)ka * n_heavy + (long)kb * n_light;
      if (taken > queued) break;
      for (int r = 0; r < n_wg; ++r) cnt[r] = main_cost[r] < lmain ? kb : ka;
      detail::price(n_wg, main_cost, n_fill, rem, nk, cnt, cost);
      double heavy = 0, sum = 0;
      for (int r = 0; r < n_wg; ++r) { heavy = std::max(heavy, cost[r]); sum += cost[r]; }
      if (heavy >= lmain + t_max - eps) continue;
      const double idle = heavy * n_wg - sum;
      if (idle < best - 1e-6 || (idle < best + 1e-6 && dist(taken) < dist(best_taken))) {
        best = idle; best_taken = taken; best_a = ka; best_b = kb;
      }
    }
  }
  long shift = 0;
  if (one_k) {
    const long room = (queued - best_taken) / n_wg;
    shift = (queued - best_taken - target + n_wg / 2) / n_wg;      // (C++ division truncates towards zero: negative -> 0 below)
    shift = std::max(0L, std::min(shift, room));
  }
  for (int r = 0; r < n_wg; ++r) cnt[r] = (int)shift + (main_cost[r] < lmain ? best_b : best_a);
  detail::emit(n_wg, n_fill, rem, cnt, out);
  return true;
}

}  // namespace mkgp
