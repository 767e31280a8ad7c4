// Host harness of the frontier arithmetic (stretch_mujoco_amd/csrc/smj_front.h): the inline functions the HIP kernel calls, compiled
// for the host.  The states, the codes of a root's slot, the order key and the representative's key on their own; then an emulation
// of the kernel's phases -- codes, frontier flags, labels, unions, jumps until a round changes nothing, the store by 16-byte groups,
// sizes in the roots' slots, the arg-max rows with per-thread bests, sums, representative, roots put back -- in both storage modes'
// indexing (the words in an array of their own, as in LDS, or in the env's slice of the output buffer, between guards) and in
// three orders of the union phase: round by round as the schedule hands the cells out, thread by thread, and shuffled.  Each is held
// against the harness's own flood fill and long-hand statistics on seeded maps, the serpentine, a spiral and maps full of ties.
// Prints the jump rounds and "ok" at the end.
#include "smj_front.h"
#include "host_check.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <queue>
#include <random>
#include <vector>

static const int THREADS = 256;   // FRONT_THREADS of smj_front.hip

struct Map { int nx, ny, min_hits, lethal, min_size, max_regions; bool have_cost; std::vector<int> hit, miss; std::vector<uint8_t> cost; };
struct Result { std::vector<int> label, goal, region; int count[2]; };

// ---- long-hand: states, mask, flood fill in ascending seeds, statistics with std::sort
static Result by_definition(const Map& m) {
  const int nx = m.nx, ny = m.ny, n = nx * ny;
  std::vector<int> st(n);
  for (int c = 0; c < n; c++) st[c] = m.hit[c] >= m.min_hits ? 1 : m.miss[c] > 0 ? 0 : -1;
  std::vector<char> fr(n, 0);
  for (int y = 0; y < ny; y++)
    for (int x = 0; x < nx; x++) {
      const int c = y * nx + x;
      if (st[c] != 0 || (m.have_cost && m.cost[c] >= m.lethal)) continue;
      fr[c] = (x > 0 && st[c - 1] < 0) || (x + 1 < nx && st[c + 1] < 0) || (y > 0 && st[c - nx] < 0) || (y + 1 < ny && st[c + nx] < 0);
    }
  Result r;
  r.label.assign(n, -1);
  struct Reg { long size, sx, sy; int label; std::vector<int> cells; };
  std::vector<Reg> regs;
  int nfront = 0;
  for (int seed = 0; seed < n; seed++) {
    if (!fr[seed] || r.label[seed] >= 0) continue;
    Reg g{0, 0, 0, seed, {}};
    std::queue<int> q;
    q.push(seed);
    r.label[seed] = seed;
    while (!q.empty()) {
      const int c = q.front(), y = c / nx, x = c % nx;
      q.pop();
      g.size++; g.sx += x; g.sy += y; g.cells.push_back(c);
      nfront++;
      for (int j = y - 1; j <= y + 1; j++)
        for (int i = x - 1; i <= x + 1; i++)
          if (j >= 0 && j < ny && i >= 0 && i < nx && fr[j * nx + i] && r.label[j * nx + i] < 0) { r.label[j * nx + i] = seed; q.push(j * nx + i); }
    }
    if (g.size >= m.min_size) regs.push_back(g);
  }
  std::sort(regs.begin(), regs.end(), [](const Reg& a, const Reg& b) { return a.size != b.size ? a.size > b.size : a.label < b.label; });
  const int G = m.max_regions;
  r.goal.assign(G, -1);
  r.region.assign(4 * G, 0);
  for (int k = 0; k < G; k++) r.region[4 * k] = -1;
  for (int k = 0; k < G && k < (int)regs.size(); k++) {
    const Reg& g = regs[k];
    long long best = -1;
    for (int c : g.cells) {   // ascending? the fill's order is not: compare the index too
      const long long dx = g.size * (c % nx) - g.sx, dy = g.size * (c / nx) - g.sy, d = dx * dx + dy * dy;
      if (best < 0 || d < best || (d == best && c < r.goal[k])) { best = d; r.goal[k] = c; }
    }
    r.region[4 * k] = g.label; r.region[4 * k + 1] = (int)g.size; r.region[4 * k + 2] = (int)g.sx; r.region[4 * k + 3] = (int)g.sy;
  }
  r.count[0] = (int)regs.size();
  r.count[1] = nfront;
  return r;
}

// ---- the kernel, on the host
struct HostLab {
  int* p;
  int get(int c) const { return p[c]; }
  void set(int c, int v) { p[c] = v; }
  int cas(int c, int expected, int v) { const int found = p[c]; if (found == expected) p[c] = v; return found; }
  int add(int c, int v) { const int found = p[c]; p[c] += v; return found; }
};

enum Order { BY_ROUND, BY_THREAD, SHUFFLED };
static int jump_rounds_seen = 0;

template <class F>
static void my_cells(int ncell, int t, F f) {
  for (int k = 0; k < smj_front_rounds(ncell, THREADS); k++) {
    const int c = smj_front_cell(t, k, THREADS);
    if (c < ncell) f(c);
  }
}
template <class F>
static void all_cells(int ncell, F f) {
  for (int t = 0; t < THREADS; t++) my_cells(ncell, t, f);
}

static Result emulate(const Map& m, bool lds, Order order, unsigned seed) {
  const int nx = m.nx, ny = m.ny, ncell = nx * ny, G = m.max_regions;
  const int pad = 5, GUARD = -12345;   // the env's slice starts 5 words into the buffer: no 16-byte alignment
  std::vector<int> out(pad + ncell + 7, GUARD), words(lds ? ncell : 0);
  HostLab lab{lds ? words.data() : out.data() + pad};
  std::vector<int> seen(ncell, 0);
  all_cells(ncell, [&](int c) { seen[c]++; });
  for (int c = 0; c < ncell; c++) CHECK(seen[c] == 1, "the schedule hands cell %d out %d times", c, seen[c]);

  all_cells(ncell, [&](int c) { lab.set(c, smj_front_code(m.hit[c], m.miss[c], m.have_cost ? m.cost[c] : 0, m.min_hits, m.lethal)); });
  all_cells(ncell, [&](int c) {
    const int code = lab.get(c);
    if (code != SMJ_FRONT_FREE) return;
    if (smj_front_is_frontier(lab, nx, ny, c / nx, c % nx)) lab.set(c, code | SMJ_FRONT_FLAG);
  });
  all_cells(ncell, [&](int c) { lab.set(c, lab.get(c) & SMJ_FRONT_FLAG ? c : -1); });
  // the unions
  const auto link = [&](int c) { if (lab.get(c) >= 0) smj_front_link(lab, nx, c / nx, c % nx); };
  if (order == BY_ROUND) {
    for (int k = 0; k < smj_front_rounds(ncell, THREADS); k++)
      for (int t = 0; t < THREADS; t++)
        if (smj_front_cell(t, k, THREADS) < ncell) link(smj_front_cell(t, k, THREADS));
  } else if (order == BY_THREAD) {
    all_cells(ncell, link);
  } else {
    std::vector<int> perm(ncell);
    std::iota(perm.begin(), perm.end(), 0);
    std::mt19937 g(seed);
    std::shuffle(perm.begin(), perm.end(), g);
    for (int c : perm) link(c);
  }
  for (int c = 0; c < ncell; c++) CHECK(lab.get(c) <= c && lab.get(c) >= -1, "cell %d holds %d after the unions", c, lab.get(c));
  // the jumps: every thread's cells in turn, in place
  int rounds = 0;
  for (;; rounds++) {
    CHECK(rounds < smj_front_max_jumps(), "more than %d jump rounds", smj_front_max_jumps());
    if (rounds >= smj_front_max_jumps()) break;
    bool changed = false;
    all_cells(ncell, [&](int c) { changed |= smj_front_jump(lab, c); });
    if (!changed) break;
  }
  if (rounds > jump_rounds_seen) jump_rounds_seen = rounds;
  Result r;
  if (lds) {
    const int al = pad & 3;
    std::vector<int> written(ncell, 0);
    for (int k = 0; k < smj_grid_groups(ncell); k++) {
      const int first = smj_grid_group_first(k, al);
      for (int i = 0; i < 4; i++)
        if (first + i >= 0 && first + i < ncell) { out[pad + first + i] = words[first + i]; written[first + i]++; }
      if (first >= 0 && first + 4 <= ncell) CHECK((pad + first) % 4 == 0, "group %d is stored wide off a 16-byte boundary", k);
    }
    for (int c = 0; c < ncell; c++) CHECK(written[c] == 1, "cell %d stored %d times", c, written[c]);
  }
  // sizes, counts
  r.count[0] = r.count[1] = 0;
  all_cells(ncell, [&](int c) {
    const int v = lab.get(c);
    r.count[1] += v >= 0;
    if (v == c) lab.set(c, smj_front_size_code(1));
  });
  all_cells(ncell, [&](int c) { const int v = lab.get(c); if (v >= 0) lab.add(v, -1); });
  std::vector<uint64_t> mine(THREADS);
  const auto best_of = [&](int t, bool count) {
    uint64_t best = 0;
    my_cells(ncell, t, [&](int c) {
      const int v = lab.get(c);
      if (!smj_front_is_size_code(v) || smj_front_code_size(v) < m.min_size) return;
      if (count) r.count[0]++;
      best = std::max(best, smj_front_order_key(smj_front_code_size(v), c));
    });
    return best;
  };
  for (int t = 0; t < THREADS; t++) mine[t] = best_of(t, true);
  std::vector<int> s_label(G, -1), s_size(G, 0), s_sx(G, 0), s_sy(G, 0), s_goal(G, 0x7fffffff);
  std::vector<uint64_t> s_rep(G, ~0ull);
  int nrows = 0;
  for (int k = 0; k < G; k++) {
    const uint64_t best = *std::max_element(mine.begin(), mine.end());
    if (!best) break;
    nrows = k + 1;
    int owners = 0;
    for (int t = 0; t < THREADS; t++) {
      if (mine[t] != best) continue;
      owners++;
      const int root = smj_front_key_label(best);
      CHECK(root % THREADS == t, "root %d chosen by thread %d", root, t);
      s_label[k] = root;
      s_size[k] = smj_front_key_size(best);
      lab.set(root, smj_front_row_code(k));
      mine[t] = best_of(t, false);
    }
    CHECK(owners == 1, "row %d has %d owners", k, owners);
  }
  all_cells(ncell, [&](int c) {
    const int row = smj_front_row_of(lab, lab.get(c));
    if (row >= 0) { s_sx[row] += c % nx; s_sy[row] += c / nx; }
  });
  all_cells(ncell, [&](int c) {
    const int row = smj_front_row_of(lab, lab.get(c));
    if (row >= 0) s_rep[row] = std::min(s_rep[row], smj_front_rep_key(s_size[row], s_sx[row], s_sy[row], c / nx, c % nx));
  });
  all_cells(ncell, [&](int c) {
    const int row = smj_front_row_of(lab, lab.get(c));
    if (row >= 0 && smj_front_rep_key(s_size[row], s_sx[row], s_sy[row], c / nx, c % nx) == s_rep[row]) s_goal[row] = std::min(s_goal[row], c);
  });
  r.goal.assign(G, -1);
  r.region.assign(4 * G, 0);
  for (int k = 0; k < G; k++) {
    if (k < nrows) r.goal[k] = s_goal[k];
    r.region[4 * k] = s_label[k]; r.region[4 * k + 1] = s_size[k]; r.region[4 * k + 2] = s_sx[k]; r.region[4 * k + 3] = s_sy[k];
  }
  if (!lds) all_cells(ncell, [&](int c) { if (lab.get(c) < -1) lab.set(c, c); });
  for (int i = 0; i < pad; i++) CHECK(out[i] == GUARD, "guard word %d before the env written", i);
  for (int i = pad + ncell; i < (int)out.size(); i++) CHECK(out[i] == GUARD, "guard word %d behind the env written", i);
  r.label.assign(out.begin() + pad, out.begin() + pad + ncell);
  return r;
}

static void compare(const char* tag, const Map& m) {
  const Result want = by_definition(m);
  for (int lds = 0; lds < 2; lds++) {
    if (lds && m.nx * m.ny > SMJ_FRONT_LDS_CELLS) continue;
    for (int order = 0; order < 3; order++) {
      const Result got = emulate(m, lds != 0, (Order)order, 17u * m.nx + m.ny);
      int bad = 0;
      for (size_t c = 0; c < want.label.size(); c++) bad += got.label[c] != want.label[c];
      CHECK(bad == 0, "%s %d x %d lds %d order %d: %d labels differ", tag, m.nx, m.ny, lds, order, bad);
      CHECK(got.goal == want.goal, "%s %d x %d lds %d order %d: goals differ (first %d, want %d)", tag, m.nx, m.ny, lds, order, got.goal[0], want.goal[0]);
      CHECK(got.region == want.region, "%s %d x %d lds %d order %d: regions differ", tag, m.nx, m.ny, lds, order);
      CHECK(got.count[0] == want.count[0] && got.count[1] == want.count[1], "%s %d x %d lds %d order %d: counts %d %d, want %d %d", tag, m.nx, m.ny, lds,
            order, got.count[0], got.count[1], want.count[0], want.count[1]);
    }
  }
}

// ---- maps: states 1 occupied, 0 free, -1 unknown
static Map from_states(int nx, int ny, const std::vector<int>& st) {
  Map m{nx, ny, 1, 253, 1, 16, false, std::vector<int>(nx * ny), std::vector<int>(nx * ny), {}};
  for (int c = 0; c < nx * ny; c++) { m.hit[c] = st[c] > 0; m.miss[c] = st[c] == 0; }
  return m;
}
static std::vector<int> serpentine(int nx, int ny) {
  std::vector<int> s(nx * ny, 0);
  for (int k = 0, y = 1; y < ny; y += 2, k++) {
    for (int x = 0; x < nx; x++) s[y * nx + x] = -1;
    s[y * nx + (k % 2 == 0 ? nx - 1 : 0)] = 0;
  }
  return s;
}
static std::vector<int> spiral(int nx, int ny) {
  std::vector<int> s(nx * ny, -1);
  int y = 0, x = 0, dy = 0, dx = 1, turns = 0;
  s[0] = 0;
  const auto in = [&](int j, int i) { return j >= 0 && j < ny && i >= 0 && i < nx; };
  while (turns < 2) {
    const int y1 = y + dy, x1 = x + dx, y2 = y + 2 * dy, x2 = x + 2 * dx;
    if (in(y1, x1) && s[y1 * nx + x1] != 0 && !(in(y2, x2) && s[y2 * nx + x2] == 0)) { y = y1; x = x1; s[y * nx + x] = 0; turns = 0; }
    else { const int t = dy; dy = dx; dx = -t; turns++; }
  }
  return s;
}

int main() {
  // the pieces
  CHECK(smj_front_state(0, 0, 1) == SMJ_FRONT_UNKNOWN && smj_front_state(0, 1, 1) == SMJ_FRONT_FREE && smj_front_state(1, 5, 1) == SMJ_FRONT_OCCUPIED, "states");
  CHECK(smj_front_state(1, 0, 2) == SMJ_FRONT_UNKNOWN && smj_front_state(1, 1, 2) == SMJ_FRONT_FREE && smj_front_state(2, 0, 2) == SMJ_FRONT_OCCUPIED, "min_hits 2");
  CHECK(smj_front_code(0, 1, 253, 1, 253) == SMJ_FRONT_BLOCKED && smj_front_code(0, 1, 252, 1, 253) == SMJ_FRONT_FREE && smj_front_code(0, 1, 255, 1, 256) == SMJ_FRONT_FREE, "cost");
  CHECK(smj_front_code(0, 0, 255, 1, 253) == SMJ_FRONT_UNKNOWN && smj_front_code(3, 0, 255, 1, 253) == SMJ_FRONT_OCCUPIED, "cost touches free cells only");
  for (int size : {1, 2, 65535, 65536}) {
    const int v = smj_front_size_code(size);
    CHECK(v <= -2 && smj_front_is_size_code(v) && !smj_front_is_row_code(v) && smj_front_code_size(v) == size, "size code %d", size);
  }
  for (int k = 0; k < SMJ_FRONT_MAX_REGIONS; k++) {
    const int v = smj_front_row_code(k);
    CHECK(!smj_front_is_size_code(v) && smj_front_is_row_code(v) && smj_front_code_row(v) == k, "row code %d", k);
  }
  CHECK(smj_front_order_key(65536, 0) > smj_front_order_key(65535, 0) && smj_front_order_key(5, 3) > smj_front_order_key(5, 4) && smj_front_order_key(1, 65535) > 0, "order");
  CHECK(smj_front_key_size(smj_front_order_key(65536, 0)) == 65536 && smj_front_key_label(smj_front_order_key(7, 65535)) == 65535, "order decoded");
  CHECK(smj_front_rep_key(65536, 0, 0, 15, 4095) == (uint64_t)65536 * 65536 * (4095ull * 4095 + 15 * 15), "the largest key");
  CHECK(smj_front_rep_key(3, 2, 20, 7, 0) == 4 + 1, "key of (0, 7) against sums (2, 20) of 3 cells");
  check_store_groups<40>(smj_grid_groups, smj_grid_group_first);

  // the phases against the definitions
  const int shapes[][2] = {{1, 1}, {2, 1}, {7, 1}, {1, 7}, {5, 5}, {16, 12}, {61, 83}, {128, 128}, {129, 128}, {4096, 4}, {4, 4096}, {256, 256}};
  for (const auto& sh : shapes) {
    const int nx = sh[0], ny = sh[1], n = nx * ny;
    std::mt19937 g(1000 * nx + ny);
    std::vector<int> st(n);
    for (int& v : st) v = (int)(g() % 3) - 1;
    Map thirds = from_states(nx, ny, st);
    thirds.max_regions = 64;
    compare("random thirds", thirds);
    Map counts = thirds;
    for (int c = 0; c < n; c++) { counts.hit[c] = (int)(g() % 4); counts.miss[c] = (int)(g() % 4); }
    counts.min_hits = 2;
    counts.min_size = 2;
    compare("counts 0 .. 3", counts);
    Map costed = thirds;
    costed.have_cost = true;
    costed.cost.resize(n);
    for (uint8_t& v : costed.cost) v = g() % 10 < 3 ? 253 + g() % 3 : g() % 253;
    compare("random cost", costed);
    costed.lethal = 256;
    costed.max_regions = 1;
    compare("lethal 256", costed);
    // mostly free with a few unknown cells: long frontier rings, few regions
    for (int& v : st) v = g() % 50 == 0 ? -1 : 0;
    Map holes = from_states(nx, ny, st);
    holes.min_size = 5;
    compare("holes", holes);
    compare("serpentine", from_states(nx, ny, serpentine(nx, ny)));
    compare("spiral", from_states(nx, ny, spiral(nx, ny)));
    // ties: isolated free cells (every region of size 1), and full rows of frontier (equal sizes, symmetric keys)
    for (int c = 0; c < n; c++) st[c] = (c / nx) % 2 == 0 && (c % nx) % 2 == 0 ? 0 : -1;
    Map iso = from_states(nx, ny, st);
    iso.max_regions = 64;
    compare("isolated", iso);
    for (int c = 0; c < n; c++) st[c] = (c / nx) % 4 == 0 ? 0 : (c / nx) % 4 == 2 ? -1 : 1;
    for (int c = 0; c < n; c++)
      if ((c / nx) % 4 == 1) st[c] = (c % nx) % 2 ? -1 : 1;   // free rows under a comb of unknown cells: one region per row, all equal
    Map rows = from_states(nx, ny, st);
    rows.max_regions = 3;
    compare("equal rows", rows);
    Map none = thirds;
    none.min_size = n + 1;
    compare("nothing kept", none);
  }
  printf("jump rounds: at most %d of %d\n", jump_rounds_seen, smj_front_max_jumps());
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
