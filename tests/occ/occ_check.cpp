// Host harness of the occupancy arithmetic (stretch_mujoco_amd/csrc/smj_occ.h): the inline functions the HIP kernel calls, compiled
// for the host.  The classification table, the closed-form line against a long-hand iterative Bresenham (no cell twice, 8-connected,
// both ends), the guards on cell indices no int can hold, and a serial emulation of the kernel's scatter on a seeded scan against
// long-hand fp64 by the comparison rule of tests/occupancy_ref.py -- the same grid as one band and as several gives identical
// arrays, accumulate adds.  Prints "ok" at the end.
#include "smj_occ.h"
#include "host_check.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <set>
#include <utility>
#include <vector>

static void check_classify() {
  float len = -7.f;
  const float r_min = 0.2f, r_max = 5.f;
  struct { float r; int clears, want; float len; } cases[] = {
      {NaN, 1, SMJ_OCC_DROP, 0.f},     {0.f, 1, SMJ_OCC_DROP, 0.f},    {-0.f, 1, SMJ_OCC_DROP, 0.f},   {0.1f, 1, SMJ_OCC_DROP, 0.f},
      {std::nextafter(0.2f, 0.f), 1, SMJ_OCC_DROP, 0.f},               {0.2f, 1, SMJ_OCC_RETURN, 0.2f}, {1.f, 1, SMJ_OCC_RETURN, 1.f},
      {5.f, 1, SMJ_OCC_RETURN, 5.f},   {std::nextafter(5.f, INF), 1, SMJ_OCC_CLEAR, 5.f},              {INF, 1, SMJ_OCC_CLEAR, 5.f},
      {-1.f, 1, SMJ_OCC_CLEAR, 5.f},   {-INF, 1, SMJ_OCC_CLEAR, 5.f},  {-1e-30f, 1, SMJ_OCC_CLEAR, 5.f},
      {-1.f, 0, SMJ_OCC_DROP, 0.f},    {INF, 0, SMJ_OCC_DROP, 0.f},    {6.f, 0, SMJ_OCC_DROP, 0.f},    {1.f, 0, SMJ_OCC_RETURN, 1.f},
      {NaN, 0, SMJ_OCC_DROP, 0.f}};
  for (const auto& c : cases) {
    const int got = smj_occ_classify(c.r, r_min, r_max, c.clears, &len);
    CHECK(got == c.want && len == c.len, "classify(%g, clears %d) = %d length %g, want %d length %g", c.r, c.clears, got, len, c.want, c.len);
  }
  CHECK(smj_occ_classify(0.f, 0.f, 5.f, 0, &len) == SMJ_OCC_RETURN && smj_occ_classify(-0.f, 0.f, 5.f, 0, &len) == SMJ_OCC_RETURN, "r_min = 0: a zero range is a return");
  CHECK(smj_occ_classify(3.f, 3.f, 3.f, 0, &len) == SMJ_OCC_RETURN && len == 3.f, "r_min == r_max keeps that value");
}

// long-hand: a running error term, one step of the major axis at a time
static std::vector<std::pair<int, int>> bresenham(int ax, int ay, int bx, int by) {
  const int dx = std::abs(bx - ax), dy = std::abs(by - ay), sx = bx < ax ? -1 : 1, sy = by < ay ? -1 : 1;
  std::vector<std::pair<int, int>> out = {{ax, ay}};
  int x = ax, y = ay;
  if (dx >= dy) {
    long err = dx;
    for (int i = 0; i < dx; i++) {
      x += sx; err += 2L * dy;
      if (err >= 2L * dx) { err -= 2L * dx; y += sy; }
      out.push_back({x, y});
    }
  } else {
    long err = dy;
    for (int i = 0; i < dy; i++) {
      y += sy; err += 2L * dx;
      if (err >= 2L * dy) { err -= 2L * dy; x += sx; }
      out.push_back({x, y});
    }
  }
  return out;
}

static void check_one_line(int ax, int ay, int bx, int by) {
  const smj_occ_line_t L = {ax, ay, bx, by, SMJ_OCC_RETURN};
  const int n = smj_occ_steps(L);
  CHECK(n == std::max(std::abs(bx - ax), std::abs(by - ay)), "steps of (%d, %d) -> (%d, %d)", ax, ay, bx, by);
  const auto want = bresenham(ax, ay, bx, by);
  CHECK((int)want.size() == n + 1, "long-hand line has %zu cells, n = %d", want.size(), n);
  std::set<std::pair<int, int>> seen;
  int px = 0, py = 0;
  for (int i = 0; i <= n; i++) {
    int ix = -12345, iy = -12345;
    smj_occ_cell(L, n, i, &ix, &iy);
    CHECK(ix == want[(size_t)i].first && iy == want[(size_t)i].second, "(%d, %d) -> (%d, %d) cell %d: (%d, %d), long-hand (%d, %d)", ax, ay, bx, by, i, ix, iy,
          want[(size_t)i].first, want[(size_t)i].second);
    CHECK(seen.insert({ix, iy}).second, "(%d, %d) -> (%d, %d) visits (%d, %d) twice", ax, ay, bx, by, ix, iy);
    if (i) CHECK(std::abs(ix - px) <= 1 && std::abs(iy - py) <= 1, "(%d, %d) -> (%d, %d) jumps at %d", ax, ay, bx, by, i);
    CHECK(smj_occ_layer(L, n, i) == (i == n), "layer of cell %d of %d", i, n);
    px = ix; py = iy;
  }
  CHECK(px == bx && py == by, "the line (%d, %d) -> (%d, %d) ends in (%d, %d)", ax, ay, bx, by, px, py);
  smj_occ_line_t C = L;
  C.kind = SMJ_OCC_CLEAR;
  CHECK(smj_occ_layer(C, n, n) == 0 && smj_occ_layer(C, n, 0) == 0, "a clearing ray has no hit");
}

static void check_line() {
  for (int dx = -40; dx <= 40; dx++)
    for (int dy = -40; dy <= 40; dy++) check_one_line(7, -3, 7 + dx, -3 + dy);
  // the longest lines the guards admit, from the largest indices: 2 i d_min stays inside int32
  const int far = 1 << 20, reach = 2 * SMJ_OCC_MAX_STEPS;
  for (int sx : {-1, 1})
    for (int sy : {-1, 1}) {
      check_one_line(sx * far, sy * far, sx * far + sx * reach, sy * far + sy * reach);
      check_one_line(sx * far, sy * far, sx * far + sx * reach, sy * far + sy * (reach - 1));
      check_one_line(sx * far, sy * far, sx * far - sx * (reach - 1), sy * far + sy * reach);
      check_one_line(-sx * far, sy * far, -sx * far + sx * 8192, sy * far - sy * 5000);
    }
  std::mt19937 g(7);
  for (int t = 0; t < 2000; t++) {
    const int ax = (int)(g() % 4001) - 2000, ay = (int)(g() % 4001) - 2000;
    check_one_line(ax, ay, ax + (int)(g() % 601) - 300, ay + (int)(g() % 601) - 300);
  }
}

static void check_guards() {
  const float o[2] = {0.5f, 0.5f}, d[2] = {1.f, 0.f};
  smj_occ_line_t L = smj_occ_line(SMJ_OCC_RETURN, o, d, 3.f, 0.f, 0.f, 1.f);
  CHECK(L.kind == SMJ_OCC_RETURN && L.ax == 0 && L.ay == 0 && L.bx == 3 && L.by == 0, "a plain ray");
  CHECK(smj_occ_line(SMJ_OCC_DROP, o, d, 3.f, 0.f, 0.f, 1.f).kind == SMJ_OCC_DROP, "a dropped ray stays dropped");
  // origin exactly 2^20 cells out is kept, the next cell is dropped; so is everything no int can hold
  const float at[2] = {1048576.5f, 0.5f}, past[2] = {1048577.5f, 0.5f}, neg[2] = {-1048576.f, 0.5f}, negpast[2] = {-1048576.5f, 0.5f};
  CHECK(smj_occ_line(SMJ_OCC_RETURN, at, d, 3.f, 0.f, 0.f, 1.f).kind == SMJ_OCC_RETURN, "origin in cell 2^20 is kept");
  CHECK(smj_occ_line(SMJ_OCC_RETURN, past, d, 3.f, 0.f, 0.f, 1.f).kind == SMJ_OCC_DROP, "origin in cell 2^20 + 1 is dropped");
  L = smj_occ_line(SMJ_OCC_RETURN, neg, d, 3.f, 0.f, 0.f, 1.f);
  CHECK(L.kind == SMJ_OCC_RETURN && L.ax == -1048576 && L.bx == -1048573, "origin in cell -2^20 is kept");
  CHECK(smj_occ_line(SMJ_OCC_RETURN, negpast, d, 3.f, 0.f, 0.f, 1.f).kind == SMJ_OCC_DROP, "origin in cell -2^20 - 1 is dropped");
  for (float bad : {NaN, INF, -INF, 3e9f, -3e9f, 1e30f, -3e38f}) {
    const float ox[2] = {bad, 0.5f}, oy[2] = {0.5f, bad}, dd[2] = {bad, 0.f}, de[2] = {0.f, bad};
    CHECK(smj_occ_line(SMJ_OCC_RETURN, ox, d, 3.f, 0.f, 0.f, 1.f).kind == SMJ_OCC_DROP, "origin x = %g is kept", bad);
    CHECK(smj_occ_line(SMJ_OCC_RETURN, oy, d, 3.f, 0.f, 0.f, 1.f).kind == SMJ_OCC_DROP, "origin y = %g is kept", bad);
    CHECK(smj_occ_line(SMJ_OCC_CLEAR, o, dd, 3.f, 0.f, 0.f, 1.f).kind == SMJ_OCC_DROP, "direction x = %g is kept", bad);
    CHECK(smj_occ_line(SMJ_OCC_CLEAR, o, de, 3.f, 0.f, 0.f, 1.f).kind == SMJ_OCC_DROP, "direction y = %g is kept", bad);
    CHECK(smj_occ_line(SMJ_OCC_RETURN, o, d, 3.f, bad, 0.f, 1.f).kind == SMJ_OCC_DROP, "x0 = %g is kept", bad);
  }
  // the longest ray the entry admits (r_max / cell = 8192) along a unit direction is kept; a direction of more than twice the length is not
  const float diag[2] = {0.70710678f, -0.70710678f}, twice[2] = {2.01f, 0.f};
  L = smj_occ_line(SMJ_OCC_CLEAR, o, d, 8192.f, 0.f, 0.f, 1.f);
  CHECK(L.kind == SMJ_OCC_CLEAR && L.bx == 8192 && smj_occ_steps(L) == 8192, "a ray of 8192 cells");
  CHECK(smj_occ_line(SMJ_OCC_CLEAR, o, diag, 8192.f, 0.f, 0.f, 1.f).kind == SMJ_OCC_CLEAR, "a diagonal ray of 8192 cells");
  CHECK(smj_occ_line(SMJ_OCC_CLEAR, o, twice, 8192.f, 0.f, 0.f, 1.f).kind == SMJ_OCC_DROP, "a ray of 16466 cells is walked");
  // negatives just below the origin: floor, not truncation
  const float below[2] = {-1e-3f, -1e-3f};
  L = smj_occ_line(SMJ_OCC_RETURN, below, d, 0.5f, 0.f, 0.f, 1.f);
  CHECK(L.ax == -1 && L.ay == -1 && L.bx == 0 && L.by == -1, "a point just below the origin falls into cell 0 (truncation instead of floor)");
}

struct Grid { std::vector<int> hit, miss; };
struct Scan {
  Pose body, frame;
  std::vector<float> site_pos, lz, r;   // [K][3], [K][3], [K]
};

// what one launch does, serially: per band the two arrays, every ray walked, the band stored once
static void emulate(const Scan& s, int kind, float x0, float y0, float cell, int nx, int ny, float r_min, float r_max, int clears, int cap, int accumulate,
                    bool with_miss, Grid* out) {
  const float inv_cell = 1.f / cell;
  const int K = (int)s.r.size();
  for (int band = 0; band < smj_hmap_bands(nx, ny, cap); band++) {
    const smj_hmap_band_t b = smj_hmap_band(nx, ny, cap, band);
    const int ncell = b.rows * b.cols, g0 = b.r0 * nx + b.c0;
    std::vector<unsigned> hits((size_t)ncell), misses((size_t)ncell);   // exactly the band: the sanitizer sees any slot beyond it
    for (int c = 0; c < ncell; c++) {
      hits[(size_t)c] = accumulate ? (unsigned)out->hit[(size_t)(g0 + c)] : 0u;
      misses[(size_t)c] = accumulate && with_miss ? (unsigned)out->miss[(size_t)(g0 + c)] : 0u;
    }
    for (int k = 0; k < K; k++) {
      float o[2], d[2], len;
      smj_occ_ray(kind, s.body.p, s.body.m, &s.site_pos[3 * (size_t)k], &s.lz[3 * (size_t)k], s.frame.p, s.frame.m, o, d);
      const int cls = smj_occ_classify(s.r[(size_t)k], r_min, r_max, clears, &len);
      const smj_occ_line_t L = smj_occ_line(cls, o, d, len, x0, y0, inv_cell);
      if (L.kind == SMJ_OCC_DROP) continue;
      const int n = smj_occ_steps(L);
      for (int i = 0; i <= n; i++) {
        int ix, iy;
        smj_occ_cell(L, n, i, &ix, &iy);
        const int slot = smj_hmap_slot(b, ix, iy);
        if (slot < 0) continue;
        if (smj_occ_layer(L, n, i)) hits[(size_t)slot] += 1u;
        else misses[(size_t)slot] += 1u;
      }
    }
    for (int c = 0; c < ncell; c++) {
      out->hit[(size_t)(g0 + c)] = (int)hits[(size_t)c];
      if (with_miss) out->miss[(size_t)(g0 + c)] = (int)misses[(size_t)c];
    }
  }
}

static void box(double p, double m, double org, double cell, long* lo, long* hi) {
  *lo = (long)std::floor((p - m - org) / cell);
  *hi = (long)std::floor((p + m - org) / cell);
}

static void check_scatter(int kind, int nx, int ny, float cell, float x0, float y0, float r_min, float r_max, int clears, unsigned seed) {
  // a laser yawed on a body yawed 0.25 rad, in a room of four walls; the frame body yawed -0.6 rad elsewhere
  const int K = 360;
  Scan s;
  const double yb = 0.25, yf = -0.6;
  const double bm[9] = {std::cos(yb), -std::sin(yb), 0, std::sin(yb), std::cos(yb), 0, 0, 0, 1};
  const double fm[9] = {std::cos(yf), -std::sin(yf), 0, std::sin(yf), std::cos(yf), 0, 0, 0, 1};
  for (int k = 0; k < 9; k++) { s.body.m[k] = (float)bm[k]; s.frame.m[k] = (float)fm[k]; }
  s.body.p[0] = 0.11f; s.body.p[1] = -0.07f; s.body.p[2] = 0.1f;
  s.frame.p[0] = -0.2f; s.frame.p[1] = 0.3f; s.frame.p[2] = 0.f;
  s.site_pos.resize(3 * K); s.lz.resize(3 * K); s.r.resize(K);
  std::mt19937 g(seed);
  std::uniform_real_distribution<double> U(0, 1);
  const double walls[4][2] = {{0, -2.3}, {0, 3.1}, {1, -1.7}, {1, 2.4}};
  std::vector<double> O(2 * (size_t)K), D(2 * (size_t)K), SO(2 * (size_t)K), SD(2 * (size_t)K);
  for (int k = 0; k < K; k++) {
    const double ang = 0.15 + 2 * M_PI * k / K;
    const float sp[3] = {0.2f, -0.15f, 0.07f}, z[3] = {(float)std::cos(ang), (float)std::sin(ang), 0.f};
    for (int j = 0; j < 3; j++) { s.site_pos[3 * (size_t)k + j] = sp[j]; s.lz[3 * (size_t)k + j] = z[j]; }
    // fp64 ray from the same fp32 inputs, with the scale of every coordinate
    double ow[3], dw[3], so[3], sd[3];
    for (int i = 0; i < 3; i++) {
      ow[i] = s.body.p[i]; so[i] = std::fabs((double)s.body.p[i]); dw[i] = 0; sd[i] = 0;
      for (int j = 0; j < 3; j++) {
        ow[i] += (double)s.body.m[3 * i + j] * sp[j]; so[i] += std::fabs((double)s.body.m[3 * i + j] * sp[j]);
        dw[i] += (double)s.body.m[3 * i + j] * z[j];  sd[i] += std::fabs((double)s.body.m[3 * i + j] * z[j]);
      }
    }
    double t = 1e30;
    for (const auto& w : walls) {
      const int a = (int)w[0];
      const double tt = (w[1] - ow[a]) / dw[a];
      if (tt > 0 && tt < t) t = tt;
    }
    float r = (float)(t + 0.01 * (U(g) - 0.5));
    const double u = U(g);
    if (u < 0.05) r = -1.f;
    else if (u < 0.07) r = NaN;
    else if (u < 0.12) r = (float)(0.129 + 0.03 * U(g));   // the rays that end on the robot itself
    else if (u < 0.14) r = INF;
    else if (u < 0.16) r = 0.f;
    s.r[(size_t)k] = r;
    for (int i = 0; i < 2; i++) {
      if (kind == SMJ_OCC_WORLD) {
        O[2 * (size_t)k + i] = ow[i]; D[2 * (size_t)k + i] = dw[i]; SO[2 * (size_t)k + i] = so[i]; SD[2 * (size_t)k + i] = sd[i];
      } else {
        double oo = 0, dd = 0, soo = 0, sdd = 0;
        for (int j = 0; j < 3; j++) {
          const double f = s.frame.m[3 * j + i];
          oo += f * (ow[j] - s.frame.p[j]); soo += std::fabs(f) * (so[j] + std::fabs((double)s.frame.p[j]));
          dd += f * dw[j]; sdd += std::fabs(f) * sd[j];
        }
        O[2 * (size_t)k + i] = oo; D[2 * (size_t)k + i] = dd; SO[2 * (size_t)k + i] = soo; SD[2 * (size_t)k + i] = sdd;
      }
    }
  }
  const size_t nc = (size_t)nx * ny;
  Grid one{std::vector<int>(nc, 7), std::vector<int>(nc, 7)};
  emulate(s, kind, x0, y0, cell, nx, ny, r_min, r_max, clears, nx * ny, 0, true, &one);   // one band
  for (int cap : {(int)SMJ_OCC_BAND_CELLS, 1024, 3 * nx, nx, nx > 8 ? nx / 2 - 1 : 1, 1}) {
    Grid many{std::vector<int>(nc, 7), std::vector<int>(nc, 7)};
    emulate(s, kind, x0, y0, cell, nx, ny, r_min, r_max, clears, cap, 0, true, &many);
    CHECK(one.hit == many.hit && one.miss == many.miss, "%d x %d cut with %d cells per band differs from one band", nx, ny, cap);
  }
  Grid honly{std::vector<int>(nc, 7), std::vector<int>(nc, 7)};
  emulate(s, kind, x0, y0, cell, nx, ny, r_min, r_max, clears, 1024, 0, false, &honly);
  CHECK(honly.hit == one.hit && honly.miss == std::vector<int>(nc, 7), "without a miss layer the hits differ or the miss layer is touched");
  Grid twice = one;
  emulate(s, kind, x0, y0, cell, nx, ny, r_min, r_max, clears, 100, 1, true, &twice);
  for (size_t q = 0; q < nc; q++) CHECK(twice.hit[q] == 2 * one.hit[q] && twice.miss[q] == 2 * one.miss[q], "cell %zu: accumulate does not add", q);
  // long-hand fp64 with the comparison rule
  const double EPS = 32 * std::ldexp(1.0, -24);
  std::vector<long> hit_lo(nc, 0), hit_hi(nc, 0), miss_lo(nc, 0), miss_hi(nc, 0);
  long sure = 0, amb = 0, dropped = 0, returns = 0;
  for (int k = 0; k < K; k++) {
    const float r = s.r[(size_t)k];
    int cls;
    double len = 0;
    if (r != r) cls = 0;
    else if (r >= r_min && r <= r_max) { cls = 1; len = r; }
    else if (r >= 0.f && r < r_min) cls = 0;
    else if (clears) { cls = 2; len = r_max; }
    else cls = 0;
    if (!cls) { dropped++; continue; }
    returns += cls == 1;
    const double* o = &O[2 * (size_t)k];
    const double* d = &D[2 * (size_t)k];
    const double e[2] = {o[0] + len * d[0], o[1] + len * d[1]};
    const double so_spread = std::ldexp(1.0, -22) * (std::fabs(o[0] - x0) + std::fabs(o[1] - y0));
    const double se_spread = std::ldexp(1.0, -22) * (std::fabs(e[0] - x0) + std::fabs(e[1] - y0));
    long al[2], ah[2], bl[2], bh[2];
    const double org[2] = {x0, y0};
    for (int i = 0; i < 2; i++) {
      box(o[i], EPS * SO[2 * (size_t)k + i] + so_spread, org[i], cell, &al[i], &ah[i]);
      box(e[i], EPS * (SO[2 * (size_t)k + i] + std::fabs(len) * SD[2 * (size_t)k + i]) + se_spread, org[i], cell, &bl[i], &bh[i]);
    }
    const bool is_sure = al[0] == ah[0] && al[1] == ah[1] && bl[0] == bh[0] && bl[1] == bh[1];
    (is_sure ? sure : amb)++;
    std::set<size_t> ch, cm;
    for (long ax = al[0]; ax <= ah[0]; ax++)
      for (long ay = al[1]; ay <= ah[1]; ay++)
        for (long bx = bl[0]; bx <= bh[0]; bx++)
          for (long by = bl[1]; by <= bh[1]; by++) {
            const auto cells = bresenham((int)ax, (int)ay, (int)bx, (int)by);
            for (size_t i = 0; i < cells.size(); i++) {
              const int ix = cells[i].first, iy = cells[i].second;
              if (ix < 0 || ix >= nx || iy < 0 || iy >= ny) continue;
              (cls == 1 && i + 1 == cells.size() ? ch : cm).insert((size_t)iy * nx + ix);
            }
          }
    for (size_t q : ch) { hit_hi[q]++; if (is_sure) hit_lo[q]++; }
    for (size_t q : cm) { miss_hi[q]++; if (is_sure) miss_lo[q]++; }
  }
  long seen = 0, occupied = 0;
  for (size_t q = 0; q < nc; q++) {
    seen += one.hit[q] > 0 || one.miss[q] > 0;
    occupied += one.hit[q] > 0;
    CHECK(hit_lo[q] <= one.hit[q] && one.hit[q] <= hit_hi[q], "cell %zu: hit %d outside [%ld, %ld]", q, one.hit[q], hit_lo[q], hit_hi[q]);
    CHECK(miss_lo[q] <= one.miss[q] && one.miss[q] <= miss_hi[q], "cell %zu: miss %d outside [%ld, %ld]", q, one.miss[q], miss_lo[q], miss_hi[q]);
    CHECK(one.hit[q] + one.miss[q] <= K, "cell %zu: more counts than rays", q);
  }
  printf("%s frame, grid %d x %d cell %g, r_max %g clears %d: returns %ld, dropped %ld, sure %ld, ambiguous %ld, cells seen %ld, occupied %ld\n",
         kind == SMJ_OCC_WORLD ? "world" : "body", nx, ny, cell, r_max, clears, returns, dropped, sure, amb, seen, occupied);
  CHECK(amb <= 7, "more than 2 %% ambiguous rays");
  CHECK(returns > 30 && seen * 20 >= (long)nc, "the scan misses the grid: %ld of %zu cells seen", seen, nc);
}

int main() {
  check_classify();
  check_line();
  check_guards();
  check_scatter(SMJ_OCC_WORLD, 64, 64, 0.05f, -1.613f, -1.587f, 0.2f, 5.f, 1, 1);
  check_scatter(SMJ_OCC_BODY, 64, 64, 0.05f, -1.613f, -1.587f, 0.2f, 9.5f, 1, 2);
  check_scatter(SMJ_OCC_WORLD, 128, 128, 0.05f, -3.213f, -3.187f, 0.2f, 9.5f, 0, 3);
  check_scatter(SMJ_OCC_BODY, 61, 83, 0.0625f, -1.913f, -2.587f, 0.2f, 2.f, 1, 4);
  check_scatter(SMJ_OCC_WORLD, 16, 12, 0.05f, 0.087f, -0.513f, 0.2f, 2.f, 0, 5);
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
