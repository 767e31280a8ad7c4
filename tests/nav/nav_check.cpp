// Host harness of the navigation-field arithmetic (stretch_mujoco_amd/csrc/smj_nav.h): the inline functions the HIP kernel calls,
// compiled for the host.  The predicate, the move cost, the diagonal rule, the neighbour order and the store's groups on their own;
// then an emulation of the kernel's phases -- weights, empty potential, goals, sweeps until one changes nothing, stores by 16-byte
// groups -- in both storage modes' indexing (the potential in an array of its own, as in LDS, or in the env's slice of the output
// buffer, relaxed in place) and in two orders: the runs of a sweep one after the other (smj_nav_walk_run, thread by thread), and in
// lock step (all 256 threads take step i of their runs before any takes step i + 1, as a wavefront does).  Each is held against the
// harness's own std::priority_queue Dijkstra and next-by-definition on seeded maps, the serpentine and maps full of ties.  Every
// cell must be stored exactly once.  Prints the sweep counts and "ok" at the end.
#include "smj_nav.h"
#include "host_check.h"

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <queue>
#include <random>
#include <utility>
#include <vector>

static const int THREADS = 256;   // NAV_THREADS of smj_nav.hip

struct Field { std::vector<int> pot, next; };
struct Map { int nx, ny, lethal, neutral; bool have_cost; std::vector<uint8_t> cost; std::vector<int> goals; };

// ---- long-hand: Dijkstra from the goals with 64-bit sums, next by its definition
static Field dijkstra(const Map& m) {
  const int nx = m.nx, ny = m.ny, n = nx * ny;
  std::vector<char> ok(n);
  std::vector<long> w(n);
  for (int c = 0; c < n; c++) { const int k = m.have_cost ? m.cost[c] : 0; ok[c] = k < m.lethal; w[c] = m.neutral + k; }
  auto moves = [&](int c, const std::function<void(int, long)>& f) {
    const int y = c / nx, x = c % nx;
    for (int dy = -1; dy <= 1; dy++)
      for (int dx = -1; dx <= 1; dx++) {   // ascending linear index
        if (!dy && !dx) continue;
        const int j = y + dy, i = x + dx;
        if (j < 0 || j >= ny || i < 0 || i >= nx || !ok[j * nx + i]) continue;
        if (dy && dx && !(ok[j * nx + x] && ok[y * nx + i])) continue;
        f(j * nx + i, (dy && dx ? 7 : 5) * (w[c] + w[j * nx + i]));
      }
  };
  std::vector<long> pot(n, SMJ_NAV_NONE);
  typedef std::pair<long, int> Item;
  std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
  for (int g : m.goals)
    if (g >= 0 && g < n && ok[g] && pot[g] != 0) { pot[g] = 0; heap.push(Item(0, g)); }
  while (!heap.empty()) {
    const Item it = heap.top();
    heap.pop();
    if (it.first > pot[it.second]) continue;
    moves(it.second, [&](int nb, long mv) {
      if (it.first + mv < pot[nb]) { pot[nb] = it.first + mv; heap.push(Item(pot[nb], nb)); }
    });
  }
  Field f{std::vector<int>(n), std::vector<int>(n, -1)};
  for (int c = 0; c < n; c++) {
    CHECK(pot[c] <= SMJ_NAV_NONE, "potential %ld above NONE", pot[c]);
    f.pot[c] = (int)pot[c];
    if (pot[c] >= SMJ_NAV_NONE) continue;
    if (pot[c] == 0) { f.next[c] = c; continue; }
    long best = -1;
    moves(c, [&](int nb, long mv) {
      if (pot[nb] < SMJ_NAV_NONE && (best < 0 || pot[nb] + mv < best)) { best = pot[nb] + mv; f.next[c] = nb; }
    });
    CHECK(best == pot[c], "cell %d: the best move gives %ld, potential %ld", c, best, pot[c]);
  }
  return f;
}

// ---- the kernel, on the host
struct HostPot {
  int* p;
  int get(int c) const { return p[c]; }
  void set(int c, int v) { p[c] = v; }
};

template <class F>
static void store_groups(std::vector<int>& out, long e0, int ncell, int base_words, std::vector<int>& written, int* wide, F value) {
  const int al = (int)((base_words + e0) & 3);
  for (int k = 0; k < smj_grid_groups(ncell); k++) {
    const int first = smj_grid_group_first(k, al);
    if (first >= ncell) continue;
    if (first >= 0 && first + 4 <= ncell) {
      CHECK(((base_words + e0 + first) & 3) == 0, "a whole group off its 16-byte boundary");
      ++*wide;
    }
    for (int i = 0; i < 4; i++) {
      const int c = first + i;
      if (c >= 0 && c < ncell) { out[e0 + c] = value(c); written[c]++; }
    }
  }
}

// lds: the potential in an array of its own, copied out at the end; otherwise relaxed in the env's slice of the output (env 1 of 2:
// env 0's slice must stay untouched).  lockstep: the order of the walk.  base_words: where the outputs' first word sits relative to
// a 16-byte boundary.
static Field emulate(const Map& m, bool lds, bool lockstep, int base_words, int* sweeps_out) {
  const int nx = m.nx, ny = m.ny, ncell = nx * ny;
  const long e0 = ncell;
  std::vector<uint16_t> w(ncell);
  std::vector<int> lpot(lds ? ncell : 0), gpot(2 * (size_t)ncell, -7), gnext(2 * (size_t)ncell, -7);
  HostPot pot{lds ? lpot.data() : gpot.data() + e0};
  for (int c = 0; c < ncell; c++) {
    w[c] = smj_nav_weight(m.have_cost ? m.cost[c] : 0, m.lethal, m.neutral);
    pot.set(c, SMJ_NAV_NONE);
  }
  for (int g : m.goals)
    if (smj_nav_goal_used(g, ncell, w.data())) pot.set(g, 0);
  const int smax = smj_nav_max_sweeps(nx, ny);
  int s = 0;
  for (; s < smax; s++) {
    bool changed = false;
    const int runs = smj_nav_runs(nx, ny, s, THREADS), items = smj_nav_lines(nx, ny, s) * runs;
    if (!lockstep) {
      for (int t = 0; t < THREADS; t++)
        for (int r = t; r < items; r += THREADS) {
          int l, i0, i1;
          smj_nav_run(nx, ny, s, runs, r, &l, &i0, &i1);
          CHECK(i0 < i1 && i1 <= smj_nav_line_len(nx, ny, s), "run %d of sweep %d: [%d, %d)", r, s, i0, i1);
          changed |= smj_nav_walk_run(pot, w.data(), nx, ny, s, l, i0, i1);
        }
    } else {
      const int per = (smj_nav_line_len(nx, ny, s) + runs - 1) / runs;   // the longest run
      for (int r0 = 0; r0 < items; r0 += THREADS)
        for (int pass = 0; pass < 2; pass++)
          for (int j = 0; j < per; j++)   // step j of the forward walk, then step j of the backward walk
            for (int r = r0; r < r0 + THREADS && r < items; r++) {
              int l, i0, i1, y, x;
              smj_nav_run(nx, ny, s, runs, r, &l, &i0, &i1);
              const int i = pass ? i1 - 2 - j : i0 + j;
              if (i < i0 || i >= i1) continue;
              smj_nav_line_cell(s, l, i, &y, &x);
              changed |= smj_nav_relax(pot, w.data(), nx, ny, y, x);
            }
    }
    if (!changed) break;
  }
  CHECK(s < smax || ncell == 1, "%d x %d: the sweep bound %d was reached", nx, ny, smax);
  *sweeps_out = s + 1 < smax ? s + 1 : smax;   // the sweeps run, the one without a change included
  std::vector<int> written(ncell, 0), written_n(ncell, 0);
  int wide = 0;
  if (lds) store_groups(gpot, e0, ncell, base_words, written, &wide, [&](int c) { return lpot[c]; });
  store_groups(gnext, e0, ncell, base_words, written_n, &wide, [&](int c) { return smj_nav_next(pot, w.data(), nx, ny, c / nx, c % nx); });
  CHECK(ncell < 8 || wide > 0, "%d x %d: no whole group", nx, ny);
  Field f{std::vector<int>(ncell), std::vector<int>(ncell)};
  for (int c = 0; c < ncell; c++) {
    CHECK((!lds || written[c] == 1) && written_n[c] == 1, "cell %d of %d x %d stored %d / %d times", c, nx, ny, written[c], written_n[c]);
    CHECK(gpot[c] == -7 && gnext[c] == -7, "env 0 was written at cell %d", c);
    f.pot[c] = gpot[e0 + c];
    f.next[c] = gnext[e0 + c];
  }
  return f;
}

static long cells_checked = 0;

static void compare(const char* tag, const Map& m) {
  const Field want = dijkstra(m);
  int reach = 0;
  for (int v : want.pot) reach += v < SMJ_NAV_NONE;
  int sweeps[4] = {0, 0, 0, 0};
  for (int mode = 0; mode < 4; mode++) {
    const bool lds = mode & 1, lockstep = mode & 2;
    if (lds && m.nx * m.ny > SMJ_NAV_LDS_CELLS) continue;
    const Field got = emulate(m, lds, lockstep, mode == 0 ? 0 : mode, &sweeps[mode]);
    for (int c = 0; c < m.nx * m.ny; c++) {
      CHECK(got.pot[c] == want.pot[c] && got.next[c] == want.next[c], "%s %d x %d mode %d cell (%d, %d): potential %d next %d, want %d %d", tag, m.nx, m.ny,
            mode, c / m.nx, c % m.nx, got.pot[c], got.next[c], want.pot[c], want.next[c]);
      cells_checked++;
    }
  }
  CHECK(m.nx * m.ny > SMJ_NAV_LDS_CELLS || (sweeps[0] == sweeps[1] && sweeps[2] == sweeps[3]), "%s: the storage mode changed the sweep count", tag);
  printf("%-22s %4d x %-4d neutral %3d  reachable %6d  sweeps: line by line %4d, lock step %4d\n", tag, m.nx, m.ny, m.neutral, reach, sweeps[0], sweeps[2]);
}

static Map blank(int nx, int ny, int lethal = 253, int neutral = 50) {
  return Map{nx, ny, lethal, neutral, true, std::vector<uint8_t>((size_t)nx * ny, 0), {}};
}

static Map serpentine(int nx, int ny) {
  Map m = blank(nx, ny, 253, 1);
  int k = 0;
  for (int y = 1; y < ny; y += 2, k++)
    for (int x = 0; x < nx; x++) m.cost[y * nx + x] = x == (k % 2 == 0 ? nx - 1 : 0) ? 0 : 254;
  m.goals = {0};
  return m;
}

static void check_pieces() {
  CHECK(smj_nav_passable(252, 253) && !smj_nav_passable(253, 253) && smj_nav_passable(255, 256) && !smj_nav_passable(0, 0), "predicate");
  CHECK(smj_nav_weight(0, 253, 50) == 50 && smj_nav_weight(255, 256, 255) == 510 && smj_nav_weight(253, 253, 50) == 0, "weight");
  CHECK(smj_nav_move(1, 1, false) == 10 && smj_nav_move(1, 1, true) == 14 && smj_nav_move(510, 510, true) == 7140, "move cost");
  CHECK(65535L * smj_nav_move(510, 510, true) == 467919900L && 467919900L < SMJ_NAV_NONE, "the largest finite potential");
  CHECK(smj_nav_diagonal_open(1, 1) && !smj_nav_diagonal_open(0, 1) && !smj_nav_diagonal_open(1, 0), "diagonal rule");
  int prev = -2000;
  for (int k = 0; k < 8; k++) {   // ascending linear index, the centre left out
    const int lin = smj_nav_dy(k) * 1000 + smj_nav_dx(k);
    CHECK(lin > prev && lin != 0 && abs(smj_nav_dy(k)) <= 1 && abs(smj_nav_dx(k)) <= 1, "neighbour %d", k);
    prev = lin;
  }
  CHECK(smj_nav_lines(5, 9, 0) == 9 && smj_nav_line_len(5, 9, 0) == 5 && smj_nav_lines(5, 9, 1) == 5 && smj_nav_line_len(5, 9, 3) == 9, "lines of a sweep");
  CHECK(smj_nav_runs(128, 128, 0, 256) == 1 && smj_nav_runs(128, 128, 1, 256) == 1 && smj_nav_runs(256, 256, 0, 256) == 1 && smj_nav_runs(64, 64, 1, 256) == 1, "whole lines on the square grids");
  CHECK(smj_nav_runs(4, 4096, 1, 256) == 32 && smj_nav_runs(4, 4096, 0, 256) == 1 && smj_nav_runs(4096, 4, 0, 256) == 32 && smj_nav_runs(4096, 16, 0, 256) == 16, "runs of the long lines");
  for (int len : {1, 7, 128, 129, 300, 4095, 4096}) {   // the runs of a line cover it once
    const int runs = smj_nav_runs(len, 2, 0, 256);
    int covered = 0;
    for (int r = 0; r < runs; r++) {
      int l, i0, i1;
      smj_nav_run(len, 2, 0, runs, r, &l, &i0, &i1);
      CHECK(l == 0 && i0 == covered && i1 > i0, "run %d of a line of %d: [%d, %d)", r, len, i0, i1);
      covered = i1;
    }
    CHECK(covered == len, "the runs cover %d of %d", covered, len);
  }
  CHECK(smj_nav_max_sweeps(256, 256) == 65536 && SMJ_NAV_LDS_CELLS >= 16384 && SMJ_NAV_MAX_CELLS == 65536, "bounds");
  check_store_groups<70>(smj_grid_groups, smj_grid_group_first);
  {   // the 3 x 3 case by hand: goal (0, 0), lethal (0, 1), neutral 1
    Map m = blank(3, 3, 253, 1);
    m.cost[1] = 254;
    m.goals = {0};
    int sw;
    const Field f = emulate(m, true, false, 0, &sw);
    const int pot[9] = {0, SMJ_NAV_NONE, 40, 10, 20, 30, 20, 24, 34}, next[9] = {0, -1, 5, 0, 3, 4, 3, 3, 4};
    for (int c = 0; c < 9; c++) CHECK(f.pot[c] == pot[c] && f.next[c] == next[c], "3 x 3 cell %d: %d %d", c, f.pot[c], f.next[c]);
  }
}

int main() {
  check_pieces();
  std::mt19937 rng(20261019);
  const int shapes[][2] = {{1, 1}, {7, 1}, {1, 7}, {16, 12}, {61, 83}, {128, 128}, {129, 128}, {600, 5}, {4096, 4}, {4, 4096}};
  for (const auto& sh : shapes) {
    const int nx = sh[0], ny = sh[1], n = nx * ny;
    {   // free, zero cost: ties everywhere (every octile path of a cell costs the same); one goal, then three, one of them skipped
      Map m = blank(nx, ny, 253, 1);
      m.goals = {(ny / 2) * nx + nx / 2};
      compare("free, centre goal", m);
      m.neutral = 255;
      m.goals = {0, n - 1, -1, n, (ny / 3) * nx + (2 * nx) / 3};
      m.have_cost = false;
      m.lethal = 1;
      compare("null cost, four goals", m);
    }
    {   // all lethal
      Map m = blank(nx, ny);
      std::fill(m.cost.begin(), m.cost.end(), 253);
      m.goals = {0};
      compare("all lethal", m);
    }
    for (int rep = 0; rep < 2; rep++) {   // 30 % lethal, random costs; then a map of two cost values only (ties between unequal paths)
      Map m = blank(nx, ny, rep ? 256 : 253, rep ? 1 : 50);
      for (int c = 0; c < n; c++) m.cost[c] = rep ? (rng() % 4 == 0 ? 255 : 1 + 2 * (rng() % 2)) : (rng() % 10 < 3 ? 253 + rng() % 3 : rng() % 253);
      m.goals = {(int)(rng() % n), (int)(rng() % n), -1};
      for (int g : m.goals)
        if (g >= 0) m.cost[g] = 0;
      compare(rep ? "two costs, lethal 256" : "random 30 %", m);
    }
    compare("serpentine", serpentine(nx, ny));
    {   // checkerboard: only the diagonal rule decides
      Map m = blank(nx, ny, 253, 1);
      for (int c = 0; c < n; c++) m.cost[c] = ((c / nx) + (c % nx)) & 1 ? 254 : 0;
      m.goals = {0};
      compare("checkerboard", m);
    }
    if (nx >= 7 && ny >= 7) {   // a wall with one gap, and a closed pocket
      Map m = blank(nx, ny, 253, 3);
      for (int y = 0; y < ny; y++) m.cost[y * nx + nx / 2] = y == ny - 2 ? 0 : 255;
      for (int y = 1; y <= 5; y++)
        for (int x = 1; x <= 5; x++)
          if (y == 1 || y == 5 || x == 1 || x == 5) m.cost[y * nx + x] = 253;
      m.goals = {nx - 1};
      compare("wall, gap, pocket", m);
    }
  }
  printf("%ld cells compared, %d failures\n", cells_checked, failures);
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
