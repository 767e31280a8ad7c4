// Host harness of the distance-field arithmetic (stretch_mujoco_amd/csrc/smj_edt.h): the inline functions the HIP kernel calls,
// compiled for the host.  The obstacle predicate, the bit searches, the cut into strips and the store's groups on their own; then a
// serial emulation of the kernel's three phases -- mask of the whole grid, row offsets and row range per strip, column search per
// 16-byte group -- for every strip of a grid, including strips whose nearest obstacle lies outside them, held against a brute force
// over all obstacle cells with the key (dist2, index), on seeded grids and on grids full of ties, with and without R.  Every cell
// must be written exactly once.  Prints "ok" at the end.
#include "smj_edt.h"
#include "host_check.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

struct Field { std::vector<int> dist2, nearest; };

// long-hand: every obstacle cell for every cell
static Field brute(const std::vector<int>& hit, const std::vector<int>* miss, int nx, int ny, int min_hits, int unknown, int R) {
  std::vector<int> obs;
  for (int c = 0; c < nx * ny; c++)
    if (hit[c] >= min_hits || (unknown && miss && hit[c] == 0 && (*miss)[c] == 0)) obs.push_back(c);
  Field f{std::vector<int>(nx * ny, SMJ_EDT_NONE), std::vector<int>(nx * ny, -1)};
  for (int y = 0; y < ny; y++)
    for (int x = 0; x < nx; x++) {
      long best = SMJ_EDT_NONE;
      int at = -1;
      for (int c : obs) {   // ascending index: '<' keeps the smallest index among equals
        const long dy = y - c / nx, dx = x - c % nx, d = dy * dy + dx * dx;
        if (d < best) { best = d; at = c; }
      }
      if (R > 0 && best > (long)R * R) { best = SMJ_EDT_NONE; at = -1; }
      f.dist2[y * nx + x] = (int)best;
      f.nearest[y * nx + x] = at;
    }
  return f;
}

// the kernel, serially; base_words: where the output's first cell sits relative to a 16-byte boundary
static Field emulate(const std::vector<int>& hit, const std::vector<int>* miss, int nx, int ny, int min_hits, int unknown, int R, int base_words,
                     int* wide_groups) {
  const int ncell = nx * ny;
  std::vector<unsigned long long> mask((ncell + 63) / 64, 0ull);
  for (int c = 0; c < ncell; c++)
    if (smj_edt_obstacle(hit[c], miss && unknown ? (*miss)[c] : 1, miss != nullptr, min_hits, unknown)) mask[c >> 6] |= 1ull << (c & 63);
  Field f{std::vector<int>(ncell, -7), std::vector<int>(ncell, -7)};
  std::vector<int> written(ncell, 0);
  const int strips = smj_edt_strips(nx, ny);
  int covered = 0;
  for (int si = 0; si < strips; si++) {
    const smj_edt_strip_t s = smj_edt_strip(nx, ny, si);
    CHECK(s.w >= 1 && s.c0 == covered && ny * s.w <= SMJ_EDT_STRIP_CELLS, "strip %d of %d x %d: c0 %d w %d", si, nx, ny, s.c0, s.w);
    covered += s.w;
    std::vector<int16_t> off((size_t)ny * s.w);
    int jlo = ny, jhi = -1;
    for (int t = 0; t < ny * s.w; t++) {
      const int y = t / s.w, lx = t - y * s.w;
      const int o = smj_edt_row_offset(mask.data(), nx, y, s.c0 + lx, R);
      CHECK(o == SMJ_EDT_NO_OFF || (s.c0 + lx + o >= 0 && s.c0 + lx + o < nx), "offset %d leaves the row", o);
      off[t] = (int16_t)o;
      if (o != SMJ_EDT_NO_OFF) { jlo = y < jlo ? y : jlo; jhi = y > jhi ? y : jhi; }
    }
    const int gmax = smj_grid_groups(s.w);
    for (int t = 0; t < ny * gmax; t++) {
      const int y = t / gmax, k = t - y * gmax;
      const int g0 = y * nx + s.c0;
      const int al = (base_words + g0) & 3;
      const int l0 = smj_grid_group_first(k, al);
      if (l0 >= s.w) continue;
      if (l0 >= 0 && l0 + 4 <= s.w) {
        CHECK(((base_words + g0 + l0) & 3) == 0, "a whole group off its 16-byte boundary");
        ++*wide_groups;
      }
      for (int i = 0; i < 4; i++) {
        const int lx = l0 + i;
        if (lx < 0 || lx >= s.w) continue;
        int d, n;
        smj_edt_column(off.data() + lx, s.w, nx, y, s.c0 + lx, jlo, jhi, R, &d, &n);
        f.dist2[g0 + lx] = d;
        f.nearest[g0 + lx] = n;
        written[g0 + lx]++;
      }
    }
  }
  CHECK(covered == nx, "the strips cover %d of %d columns", covered, nx);
  for (int c = 0; c < ncell; c++) CHECK(written[c] == 1, "cell %d of %d x %d written %d times", c, nx, ny, written[c]);
  return f;
}

static long cells_checked = 0;

static void compare(const char* tag, const std::vector<int>& hit, const std::vector<int>* miss, int nx, int ny, int min_hits, int unknown) {
  for (int R : {0, 1, 3, 20}) {
    const Field want = brute(hit, miss, nx, ny, min_hits, unknown, R);
    for (int base : {0, 1, 3}) {
      int wide = 0;
      const Field got = emulate(hit, miss, nx, ny, min_hits, unknown, R, base, &wide);
      CHECK(nx < 8 || wide > 0, "%s %d x %d: no whole group", tag, nx, ny);
      for (int c = 0; c < nx * ny; c++) {
        CHECK(got.dist2[c] == want.dist2[c] && got.nearest[c] == want.nearest[c], "%s %d x %d R %d base %d cell (%d, %d): dist2 %d nearest %d, want %d %d",
              tag, nx, ny, R, base, c / nx, c % nx, got.dist2[c], got.nearest[c], want.dist2[c], want.nearest[c]);
        cells_checked++;
      }
    }
  }
}

static void check_pieces() {
  CHECK(smj_edt_obstacle(1, 0, 1, 1, 0) && !smj_edt_obstacle(0, 0, 1, 1, 0) && smj_edt_obstacle(0, 0, 1, 1, 1) && !smj_edt_obstacle(0, 2, 1, 1, 1), "predicate");
  CHECK(!smj_edt_obstacle(2, 0, 1, 3, 0) && smj_edt_obstacle(3, 5, 1, 3, 0) && !smj_edt_obstacle(0, 0, 0, 1, 1) && !smj_edt_obstacle(1, 0, 1, 2, 1), "predicate, min_hits");
  CHECK(smj_edt_strips(128, 128) == 1 && smj_edt_strips(256, 256) == 4 && smj_edt_strip(256, 256, 3).c0 == 192 && smj_edt_strip(256, 256, 3).w == 64, "strips of the square grids");
  CHECK(smj_edt_strips(16, 4096) == 4 && smj_edt_strip_width(16, 4096) == 4 && smj_edt_strips(4096, 16) == 4 && smj_edt_strip_width(4096, 16) == 1024, "strips of the extremes");
  CHECK(smj_edt_strips(1, 1) == 1 && smj_edt_strips(129, 127) == 1 && smj_edt_strips(131, 127) == 2 && smj_edt_strip(131, 127, 1).w == 65, "strips of odd grids");
  // the bit searches against a scan, over word boundaries
  std::mt19937 rng(7);
  std::vector<unsigned long long> m(5);
  for (int rep = 0; rep < 200; rep++) {
    for (auto& w : m) w = rep % 3 == 0 ? 0ull : (rng() % 4 ? (1ull << (rng() % 64)) : ((unsigned long long)rng() << 32 | rng()) & ((unsigned long long)rng() << 32 | rng()));
    const int a = rng() % 320, b = rng() % 320, lo = a < b ? a : b, hi = a < b ? b : a, pos = lo + rng() % (hi - lo + 1);
    int pw = -1, nw = -1;
    for (int c = lo; c <= pos; c++) if (m[c >> 6] >> (c & 63) & 1) pw = c;
    for (int c = hi; c >= pos; c--) if (m[c >> 6] >> (c & 63) & 1) nw = c;
    CHECK(smj_edt_prev(m.data(), lo, pos) == pw && smj_edt_next(m.data(), pos, hi) == nw, "bit search [%d, %d] from %d", lo, hi, pos);
  }
  check_store_groups<70>(smj_grid_groups, smj_grid_group_first);
}

int main() {
  check_pieces();
  std::mt19937 rng(20261019);
  const int shapes[][2] = {{1, 1}, {7, 1}, {1, 7}, {16, 12}, {61, 83}, {64, 64}, {131, 127}, {200, 100}, {1024, 16}, {16, 1024}, {4096, 4}, {4, 4096}};
  for (const auto& sh : shapes) {
    const int nx = sh[0], ny = sh[1], n = nx * ny;
    const bool big = n > 12000;
    std::vector<int> hit(n, 0), miss(n, 0);
    compare("empty", hit, nullptr, nx, ny, 1, 0);
    if (!big) {
      std::fill(hit.begin(), hit.end(), 1);
      compare("full", hit, nullptr, nx, ny, 1, 0);
    }
    for (int corner = 0; corner < 4; corner++) {
      std::fill(hit.begin(), hit.end(), 0);
      hit[(corner / 2 ? ny - 1 : 0) * nx + (corner % 2 ? nx - 1 : 0)] = 1;
      compare("corner", hit, nullptr, nx, ny, 1, 0);
    }
    for (double p : {0.01, 0.3}) {
      if (big && p > 0.1) continue;   // the brute force is obstacles x cells
      for (int c = 0; c < n; c++) { hit[c] = (rng() % 10000 < p * 10000) ? 1 + rng() % 5 : 0; miss[c] = rng() % 3; }
      compare("random", hit, nullptr, nx, ny, 1, 0);
      compare("random, min_hits 3", hit, nullptr, nx, ny, 3, 0);
      if (!big) compare("random, unknown", hit, &miss, nx, ny, 2, 1);
    }
    if (!big) {
      for (int c = 0; c < n; c++) hit[c] = ((c / nx) + (c % nx)) & 1;
      compare("checkerboard", hit, nullptr, nx, ny, 1, 0);
    }
    // the four-fold tie: obstacles at the middles of the four edges
    std::fill(hit.begin(), hit.end(), 0);
    hit[nx / 2] = hit[(ny - 1) * nx + nx / 2] = hit[(ny / 2) * nx] = hit[(ny / 2) * nx + nx - 1] = 1;
    compare("four-fold tie", hit, nullptr, nx, ny, 1, 0);
    // obstacles in the last strip alone: every other strip looks across its edge
    std::fill(hit.begin(), hit.end(), 0);
    const smj_edt_strip_t last = smj_edt_strip(nx, ny, smj_edt_strips(nx, ny) - 1);
    for (int y = 0; y < ny; y += 3) hit[y * nx + last.c0 + (y % last.w)] = 1;
    compare("last strip", hit, nullptr, nx, ny, 1, 0);
  }
  {   // the issue's example: 9 x 9, the centre takes the top obstacle
    std::vector<int> hit(81, 0);
    hit[4] = hit[8 * 9 + 4] = hit[4 * 9] = hit[4 * 9 + 8] = 1;
    int wide = 0;
    const Field f = emulate(hit, nullptr, 9, 9, 1, 0, 0, 0, &wide);
    CHECK(f.dist2[40] == 16 && f.nearest[40] == 4, "centre of the 9 x 9 tie grid: dist2 %d nearest %d", f.dist2[40], f.nearest[40]);
  }
  printf("%ld cells compared, %d failures\n", cells_checked, failures);
  if (failures) return 1;
  printf("ok\n");
  return 0;
}
