// Host harness of the height-map arithmetic (stretch_mujoco_amd/csrc/smj_hmap.h): the inline functions the HIP kernel calls,
// compiled for the host.  The order-preserving key (strictly monotone, round trip, key 0 never produced), the cell rule at and
// around boundaries and on values no int can hold, the cut into bands, the split of a band store, and a serial emulation of the kernel's scatter on a seeded
// image against long-hand fp64 by the comparison rule of tests/height_map_ref.py -- the same grid as one band and as several gives
// identical arrays.  Prints "ok" at the end.
#include "smj_hmap.h"
#include "host_check.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

static void check_key() {
  std::vector<float> v = {0.f, -0.f, from_bits(1u), from_bits(0x007fffffu), from_bits(0x00800000u), from_bits(0x7f7fffffu),
                          -from_bits(1u), -from_bits(0x007fffffu), -from_bits(0x00800000u), -from_bits(0x7f7fffffu), INF, -INF, 1.f, -1.f};
  std::mt19937 g(2024);
  while (v.size() < 100014) {
    const float f = from_bits((uint32_t)g());
    if (f == f) v.push_back(f);
  }
  // total order of the sweep: by value, -0 before +0
  std::sort(v.begin(), v.end(), [](float a, float b) { return a < b || (a == b && std::signbit(a) && !std::signbit(b)); });
  for (size_t i = 0; i < v.size(); i++) {
    const uint32_t k = smj_hmap_key(v[i]);
    CHECK(k != 0u, "key 0 produced by %.9g", v[i]);
    CHECK(to_bits(smj_hmap_unkey(k)) == to_bits(v[i]), "round trip of %.9g (bits %08x)", v[i], to_bits(v[i]));
    if (i) {
      const uint32_t kp = smj_hmap_key(v[i - 1]);
      if (to_bits(v[i]) == to_bits(v[i - 1])) CHECK(k == kp, "equal floats, different keys");
      else CHECK(kp < k, "not strictly monotone: %.9g (%08x) -> %08x, %.9g (%08x) -> %08x", v[i - 1], to_bits(v[i - 1]), kp, v[i], to_bits(v[i]), k);
    }
  }
  CHECK(smj_hmap_key(-0.f) < smj_hmap_key(0.f), "-0 sorts below +0");
  CHECK(std::isnan(smj_hmap_unkey(0u)), "key 0 decodes to NaN");
  CHECK(smj_hmap_key_of_stored(std::numeric_limits<float>::quiet_NaN()) == 0u && smj_hmap_key_of_stored(-std::numeric_limits<float>::quiet_NaN()) == 0u,
        "a stored NaN of either sign is empty");
  CHECK(smj_hmap_key_of_stored(-2.5f) == smj_hmap_key(-2.5f) && smj_hmap_key_of_stored(-INF) == smj_hmap_key(-INF), "stored numbers keep their key");
}

static bool cell_of(float x, float y, float z, float x0, float y0, float cell, int nx, int ny, float zl, float zh, int* ix, int* iy) {
  *ix = *iy = -12345;
  return smj_hmap_cell(x, y, z, x0, y0, 1.f / cell, nx, ny, zl, zh, ix, iy);
}

static void check_cell_rule() {
  int ix, iy;
  // a grid whose edges are exact in fp32: origin -2, cell 0.25 (inv_cell 4), 16 x 8
  const float x0 = -2.f, y0 = -1.f, c = 0.25f;
  const int nx = 16, ny = 8;
  for (int k = -2; k <= nx + 1; k++) {
    const float edge = x0 + k * c;
    bool in = cell_of(edge, 0.f, 0.f, x0, y0, c, nx, ny, -1.f, 1.f, &ix, &iy);
    CHECK(in == (k >= 0 && k < nx) && (!in || (ix == k && iy == 4)), "x at edge %d: in %d ix %d iy %d", k, in, ix, iy);
    // the neighbours of an edge, on a grid from 0 (x - x0 is then exact; from -2 the subtraction rounds a neighbour back onto the edge)
    const float e0 = k * c, below = std::nextafter(e0, -INF), above = std::nextafter(e0, INF);
    in = cell_of(below, 0.f, 0.f, 0.f, y0, c, nx, ny, -1.f, 1.f, &ix, &iy);
    CHECK(in == (k >= 1 && k <= nx) && (!in || ix == k - 1), "x just below edge %d: in %d ix %d", k, in, ix);
    in = cell_of(above, 0.f, 0.f, 0.f, y0, c, nx, ny, -1.f, 1.f, &ix, &iy);
    CHECK(in == (k >= 0 && k < nx) && (!in || ix == k), "x just above edge %d: in %d ix %d", k, in, ix);
  }
  for (int k = -2; k <= ny + 1; k++) {
    const float edge = y0 + k * c, below = std::nextafter(k * c, -INF);
    bool in = cell_of(0.f, edge, 0.f, x0, y0, c, nx, ny, -1.f, 1.f, &ix, &iy);
    CHECK(in == (k >= 0 && k < ny) && (!in || (iy == k && ix == 8)), "y at edge %d: in %d ix %d iy %d", k, in, ix, iy);
    in = cell_of(0.f, below, 0.f, x0, 0.f, c, nx, ny, -1.f, 1.f, &ix, &iy);
    CHECK(in == (k >= 1 && k <= ny) && (!in || iy == k - 1), "y just below edge %d: in %d iy %d", k, in, iy);
  }
  // the z band is closed on both sides
  CHECK(cell_of(0.f, 0.f, -1.f, x0, y0, c, nx, ny, -1.f, 1.f, &ix, &iy) && cell_of(0.f, 0.f, 1.f, x0, y0, c, nx, ny, -1.f, 1.f, &ix, &iy), "z at the limits is kept");
  CHECK(!cell_of(0.f, 0.f, std::nextafter(-1.f, -INF), x0, y0, c, nx, ny, -1.f, 1.f, &ix, &iy) &&
        !cell_of(0.f, 0.f, std::nextafter(1.f, INF), x0, y0, c, nx, ny, -1.f, 1.f, &ix, &iy), "z just outside the limits is dropped");
  CHECK(cell_of(0.f, 0.f, 3e38f, x0, y0, c, nx, ny, -INF, INF, &ix, &iy) && cell_of(0.f, 0.f, -3e38f, x0, y0, c, nx, ny, -INF, INF, &ix, &iy), "an open band keeps every z");
  CHECK(cell_of(0.f, 0.f, 0.5f, x0, y0, c, nx, ny, 0.5f, 0.5f, &ix, &iy), "z_lo == z_hi keeps that value");
  // NaN, infinities, values beyond the int range: dropped by a float compare, the outputs are not touched
  for (float bad : {NaN, INF, -INF, 3e9f, -3e9f, 1e30f, -1e30f, 3e38f, -3e38f}) {
    CHECK(!cell_of(bad, 0.f, 0.f, x0, y0, c, nx, ny, -1.f, 1.f, &ix, &iy) && ix == -12345 && iy == -12345, "x = %g is kept", bad);
    CHECK(!cell_of(0.f, bad, 0.f, x0, y0, c, nx, ny, -1.f, 1.f, &ix, &iy) && ix == -12345 && iy == -12345, "y = %g is kept", bad);
  }
  for (float bad : {NaN, INF, -INF}) CHECK(!cell_of(0.f, 0.f, bad, x0, y0, c, nx, ny, -1.f, 1.f, &ix, &iy), "z = %g is kept", bad);
  CHECK(!cell_of(0.f, 0.f, NaN, x0, y0, c, nx, ny, -INF, INF, &ix, &iy), "a NaN z passes an open band");
  // negatives just below the origin: floor, not truncation
  CHECK(!cell_of(x0 - 1e-3f, 0.f, 0.f, x0, y0, c, nx, ny, -1.f, 1.f, &ix, &iy) && !cell_of(0.f, y0 - 1e-3f, 0.f, x0, y0, c, nx, ny, -1.f, 1.f, &ix, &iy),
        "a point just below the origin falls into cell 0 (truncation instead of floor)");
  // the largest grid side and a huge cell
  CHECK(cell_of(1e6f, -1e6f, 0.f, -1e30f, -1e30f, 3e38f, 1, 1, -INF, INF, &ix, &iy) && ix == 0 && iy == 0, "one huge cell");
  CHECK(cell_of(65535.5f, 0.5f, 0.f, 0.f, 0.f, 1.f, 65536, 1, -1.f, 1.f, &ix, &iy) && ix == 65535 && iy == 0, "last column of the widest grid");
  CHECK(!cell_of(65536.f, 0.5f, 0.f, 0.f, 0.f, 1.f, 65536, 1, -1.f, 1.f, &ix, &iy), "one past the widest grid");
}

static void check_bands() {
  const int shapes[][3] = {{1, 1, 4096}, {16, 12, 4096}, {64, 64, 4096}, {128, 128, 4096}, {64, 96, 4096}, {100, 7, 64}, {4097, 3, 4096},
                           {65536, 1, 4096}, {1, 65536, 4096}, {5000, 13, 4096}, {37, 23, 7}, {4096, 16, 4096}, {3, 5, 1}};
  for (const auto& s : shapes) {
    const int nx = s[0], ny = s[1], cap = s[2], nb = smj_hmap_bands(nx, ny, cap);
    std::vector<int> owner((size_t)nx * ny, -1);
    for (int b = 0; b < nb; b++) {
      const smj_hmap_band_t B = smj_hmap_band(nx, ny, cap, b);
      CHECK(B.rows >= 1 && B.cols >= 1 && B.rows * B.cols <= cap && B.r0 >= 0 && B.r0 + B.rows <= ny && B.c0 >= 0 && B.c0 + B.cols <= nx,
            "band %d of %d x %d cap %d: rows %d+%d cols %d+%d", b, nx, ny, cap, B.r0, B.rows, B.c0, B.cols);
      CHECK(B.rows == 1 || B.cols == nx, "a band of several rows holds whole rows");
      for (int iy = B.r0; iy < B.r0 + B.rows; iy++)
        for (int ix = B.c0; ix < B.c0 + B.cols; ix++) {
          const int slot = smj_hmap_slot(B, ix, iy);
          CHECK(slot >= 0 && slot < B.rows * B.cols && (long long)B.r0 * nx + B.c0 + slot == (long long)iy * nx + ix, "slot of (%d, %d) in band %d", iy, ix, b);
          CHECK(owner[(size_t)iy * nx + ix] == -1, "cell (%d, %d) in two bands", iy, ix);
          owner[(size_t)iy * nx + ix] = b;
        }
      CHECK(smj_hmap_slot(B, B.c0 - 1, B.r0) == -1 && smj_hmap_slot(B, B.c0 + B.cols, B.r0) == -1 && smj_hmap_slot(B, B.c0, B.r0 - 1) == -1 &&
            smj_hmap_slot(B, B.c0, B.r0 + B.rows) == -1, "a cell outside band %d has a slot", b);
    }
    for (int o : owner) CHECK(o >= 0, "a cell of %d x %d (cap %d) is in no band", nx, ny, cap);
  }
  CHECK(smj_hmap_bands(64, 64, SMJ_HMAP_BAND_CELLS) == 1, "a 64 x 64 grid is a single band");
  CHECK(smj_hmap_bands(128, 128, SMJ_HMAP_BAND_CELLS) == 4 && smj_hmap_bands(64, 96, SMJ_HMAP_BAND_CELLS) == 2, "128 x 128 is four bands, 64 x 96 two");
}

// the split of a band store against a brute-force enumeration: every cell stored exactly once, the groups on 16-byte boundaries
static void check_store_split() {
  for (int ncell = 0; ncell <= 40; ncell++)
    for (int mis = 0; mis <= 3; mis++) {
      const uintptr_t out = 0x1000u + 4u * (unsigned)mis;
      const smj_hmap_split_t s = smj_hmap_store_split(out, ncell);
      std::vector<int> stored((size_t)ncell, 0);
      bool inside = true;
      for (int g = 0; g < s.groups; g++) {
        const int c = s.lead + 4 * g;
        CHECK((out + 4u * (unsigned)c) % 16u == 0, "ncell %d misaligned by %d words: group %d starts off a 16-byte boundary", ncell, mis, g);
        for (int k = 0; k < 4; k++) {
          if (c + k >= 0 && c + k < ncell) stored[(size_t)(c + k)]++;
          else inside = false;
        }
      }
      for (int t = 0; t < s.rest; t++) {
        const int c = smj_hmap_split_rest(s, t);
        if (c >= 0 && c < ncell) stored[(size_t)c]++;
        else inside = false;
      }
      CHECK(inside, "ncell %d misaligned by %d words: a store outside the band", ncell, mis);
      CHECK(s.lead >= 0 && s.lead <= 3 && s.rest >= 0 && s.rest <= 6, "ncell %d misaligned by %d words: lead %d rest %d", ncell, mis, s.lead, s.rest);
      for (int c = 0; c < ncell; c++) CHECK(stored[(size_t)c] == 1, "ncell %d misaligned by %d words: cell %d stored %d times", ncell, mis, c, stored[(size_t)c]);
    }
}

struct Map { std::vector<float> z; std::vector<int> n; };

// what one launch does, serially: per band the two arrays, every kept pixel scattered with max / add, decoded and stored once
static void emulate(const std::vector<float>& depth, int W, int H, int stride, float fovy, const float* T, float x0, float y0, float cell, int nx, int ny,
                    float zl, float zh, int cap, int accumulate, Map* out) {
  const float th = tanf(fovy * 3.14159265358979323846f / 360.f), aspect = (float)W / (float)H, inv_cell = 1.f / cell;
  const int wp = smj_points_grid(W, stride), hp = smj_points_grid(H, stride);
  for (int band = 0; band < smj_hmap_bands(nx, ny, cap); band++) {
    const smj_hmap_band_t b = smj_hmap_band(nx, ny, cap, band);
    const int ncell = b.rows * b.cols, g0 = b.r0 * nx + b.c0;
    std::vector<uint32_t> keys((size_t)ncell), cnt((size_t)ncell);   // exactly the band: the sanitizer sees any slot beyond it
    for (int c = 0; c < ncell; c++) {
      keys[(size_t)c] = accumulate ? smj_hmap_key_of_stored(out->z[(size_t)(g0 + c)]) : 0u;
      cnt[(size_t)c] = accumulate ? (uint32_t)out->n[(size_t)(g0 + c)] : 0u;
    }
    for (int i = 0; i < hp; i++)
      for (int j = 0; j < wp; j++) {
        int u, v, ix, iy;
        float z;
        smj_points_pixel(i, j, stride, &u, &v);
        if (!smj_hmap_pixel(depth[(size_t)v * W + u], u, v, W, H, th, aspect, T, x0, y0, inv_cell, nx, ny, zl, zh, &ix, &iy, &z)) continue;
        const int slot = smj_hmap_slot(b, ix, iy);
        if (slot < 0) continue;
        keys[(size_t)slot] = std::max(keys[(size_t)slot], smj_hmap_key(z));
        cnt[(size_t)slot] += 1u;
      }
    for (int c = 0; c < ncell; c++) {
      out->z[(size_t)(g0 + c)] = smj_hmap_unkey(keys[(size_t)c]);
      out->n[(size_t)(g0 + c)] = (int)cnt[(size_t)c];
    }
  }
}

static bool same(const Map& a, const Map& b) {
  return a.z.size() == b.z.size() && !memcmp(a.z.data(), b.z.data(), 4 * a.z.size()) && !memcmp(a.n.data(), b.n.data(), 4 * a.n.size());
}

static void check_scatter(int W, int H, int stride, int nx, int ny, float cell, float x0, float y0, float zl, float zh, unsigned seed) {
  // camera 1.3 m up, pitched 0.75 rad down and yawed 0.45 (the scene of tests/height_map_ref.py), as body pose + camera offset
  const double cy = std::cos(0.45), sy = std::sin(0.45), cpi = std::cos(-0.75), spi = std::sin(-0.75);
  const double yaw[9] = {cy, -sy, 0, sy, cy, 0, 0, 0, 1}, look[9] = {0, 0, -1, -1, 0, 0, 0, 1, 0}, pit[9] = {1, 0, 0, 0, cpi, -spi, 0, spi, cpi};
  double lp[9];
  Pose cb{}, cam{};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      lp[3 * i + j] = 0;
      for (int k = 0; k < 3; k++) lp[3 * i + j] += look[3 * i + k] * pit[3 * k + j];
      cb.m[3 * i + j] = (float)yaw[3 * i + j];
    }
  for (int k = 0; k < 9; k++) cam.m[k] = (float)lp[k];
  cb.p[0] = 0.03f; cb.p[1] = -0.02f; cb.p[2] = 1.25f;
  cam.p[0] = 0.01f; cam.p[1] = -0.015f; cam.p[2] = 0.05f;
  // fp64 camera pose from the same fp32 inputs
  double cpos[3], cmat[9];
  for (int i = 0; i < 3; i++) {
    cpos[i] = cb.p[i];
    for (int k = 0; k < 3; k++) cpos[i] += (double)cb.m[3 * i + k] * cam.p[k];
    for (int j = 0; j < 3; j++) {
      cmat[3 * i + j] = 0;
      for (int k = 0; k < 3; k++) cmat[3 * i + j] += (double)cb.m[3 * i + k] * cam.m[3 * k + j];
    }
  }
  const double fovy = 58.0, thd = std::tan(fovy * M_PI / 360.0);
  std::mt19937 g(seed);
  std::uniform_real_distribution<double> U(0, 1);
  std::vector<float> depth((size_t)W * H);
  for (int v = 0; v < H; v++)
    for (int u = 0; u < W; u++) {
      const double xn = ((u + 0.5) / W * 2 - 1) * thd * W / H, yn = (1 - (v + 0.5) / H * 2) * thd;
      double t = 1e30;
      const double planes[3][2] = {{2, 0.0}, {0, 2.1}, {1, 1.4}};
      for (const auto& pl : planes) {
        const int a = (int)pl[0];
        const double dir = cmat[3 * a] * xn + cmat[3 * a + 1] * yn - cmat[3 * a + 2], tt = (pl[1] - cpos[a]) / dir;
        if (tt > 0 && tt < t) t = tt;
      }
      float d = t < 30 ? (float)(t + 0.02 * (U(g) - 0.5)) : 0.f;   // a rough surface: the max of a cell is not its first or last pixel
      const double r = U(g);
      if (r < 0.01) d = 0.f;
      else if (r < 0.015) d = std::numeric_limits<float>::quiet_NaN();
      else if (r < 0.02) d = INF;
      else if (r < 0.025) d = -d;
      depth[(size_t)v * W + u] = d;
    }
  float T[12];
  smj_points_transform(SMJ_PT_WORLD, cb.p, cb.m, cam.p, cam.m, nullptr, nullptr, T);
  const size_t nc = (size_t)nx * ny;
  Map one{std::vector<float>(nc, 7.f), std::vector<int>(nc, 7)};
  emulate(depth, W, H, stride, (float)fovy, T, x0, y0, cell, nx, ny, zl, zh, nx * ny, 0, &one);   // one band
  std::vector<int> caps = {(int)SMJ_HMAP_BAND_CELLS, 1024, 3 * nx};
  if (W * H < 2000) caps.insert(caps.end(), {nx, nx > 8 ? nx / 2 - 1 : 1, 1});   // down to pieces of a row and single cells, on the small image
  for (int cap : caps) {
    Map many{std::vector<float>(nc, 7.f), std::vector<int>(nc, 7)};
    emulate(depth, W, H, stride, (float)fovy, T, x0, y0, cell, nx, ny, zl, zh, cap, 0, &many);
    CHECK(same(one, many), "%d x %d cut with %d cells per band differs from one band", nx, ny, cap);
  }
  // long-hand fp64 with the comparison rule
  const double EPS = 32 * std::ldexp(1.0, -24);
  std::vector<long> n_lo(nc, 0), n_hi(nc, 0);
  std::vector<double> z_lo(nc, -INFINITY), z_hi(nc, -INFINITY), m_z(nc, 0.0);
  long valid = 0, amb = 0;
  for (int v = 0; v < H; v += stride)
    for (int u = 0; u < W; u += stride) {
      const float df = depth[(size_t)v * W + u];
      if (!(df > 0.f && df <= 3.402823466e38f)) continue;
      valid++;
      const double d = df, xn = ((u + 0.5) / W * 2 - 1) * thd * W / H, yn = (1 - (v + 0.5) / H * 2) * thd;
      const double c[3] = {d * xn, d * yn, -d};
      double p[3], S = d * (std::fabs(xn) + std::fabs(yn) + 1);
      for (int i = 0; i < 3; i++) p[i] = cpos[i] + cmat[3 * i] * c[0] + cmat[3 * i + 1] * c[1] + cmat[3 * i + 2] * c[2];
      for (int k = 0; k < 3; k++) S += std::fabs((double)cb.p[k]) + std::fabs((double)cam.p[k]);
      const double m = EPS * S + std::ldexp(1.0, -22) * (std::fabs(p[0] - x0) + std::fabs(p[1] - y0));
      const double ixl = std::floor((p[0] - m - x0) / cell), ixh = std::floor((p[0] + m - x0) / cell);
      const double iyl = std::floor((p[1] - m - y0) / cell), iyh = std::floor((p[1] + m - y0) / cell);
      const bool z_in = p[2] - m >= zl && p[2] + m <= zh, z_out = p[2] + m < zl || p[2] - m > zh;
      const bool grid_out = ixh < 0 || ixl >= nx || iyh < 0 || iyl >= ny, grid_in = ixl >= 0 && ixh < nx && iyl >= 0 && iyh < ny;
      if (grid_out || z_out) continue;
      const bool sure = ixl == ixh && iyl == iyh && grid_in && z_in;
      if (!sure) amb++;
      for (int iy = (int)std::max(iyl, 0.0); iy <= (int)std::min(iyh, ny - 1.0); iy++)
        for (int ix = (int)std::max(ixl, 0.0); ix <= (int)std::min(ixh, nx - 1.0); ix++) {
          const size_t q = (size_t)iy * nx + ix;
          if (sure) { n_lo[q]++; z_lo[q] = std::max(z_lo[q], p[2]); }
          n_hi[q]++;
          z_hi[q] = std::max(z_hi[q], p[2]);
          m_z[q] = std::max(m_z[q], m);
        }
    }
  long occupied = 0;
  for (size_t q = 0; q < nc; q++) {
    const int n = one.n[q];
    const float h = one.z[q];
    occupied += n > 0;
    CHECK(n_lo[q] <= n && n <= n_hi[q], "cell %zu: count %d outside [%ld, %ld]", q, n, n_lo[q], n_hi[q]);
    CHECK(std::isnan(h) == (n == 0), "cell %zu: height %g with count %d", q, h, n);
    if (!std::isnan(h)) CHECK(z_lo[q] - m_z[q] <= h && h <= z_hi[q] + m_z[q], "cell %zu: height %.9g outside [%.9g, %.9g] +- %.3g", q, h, z_lo[q], z_hi[q], m_z[q]);
  }
  printf("%d x %d stride %d, grid %d x %d cell %g: valid %ld, ambiguous %ld (%.3f %%), occupied cells %ld\n", W, H, stride, nx, ny, cell, valid, amb,
         100.0 * amb / std::max(valid, 1L), occupied);
  CHECK(amb * 100 <= valid, "more than 1 %% ambiguous points");
  CHECK(occupied * 20 >= (long)nc || nc < 20, "the scene misses the grid: %ld of %zu cells occupied", occupied, nc);
  // accumulate: map(A) then accumulate(B) == fmax / sum of the two, in either order (B: the other stride phase of the same image)
  if (stride > 1) {
    std::vector<float> shifted(depth.size(), 0.f);   // phase (1, 1): pixel (u, v) of `shifted` is pixel (u + 1, v + 1) of the image
    for (int v = 0; v + 1 < H; v++)
      for (int u = 0; u + 1 < W; u++) shifted[(size_t)v * W + u] = depth[(size_t)(v + 1) * W + u + 1];
    Map a{std::vector<float>(nc), std::vector<int>(nc)}, b = a, ab = a, ba = a;
    emulate(depth, W, H, stride, (float)fovy, T, x0, y0, cell, nx, ny, zl, zh, 1024, 0, &a);
    emulate(shifted, W, H, stride, (float)fovy, T, x0, y0, cell, nx, ny, zl, zh, 1024, 0, &b);
    emulate(depth, W, H, stride, (float)fovy, T, x0, y0, cell, nx, ny, zl, zh, 1024, 0, &ab);
    emulate(shifted, W, H, stride, (float)fovy, T, x0, y0, cell, nx, ny, zl, zh, 100, 1, &ab);
    emulate(shifted, W, H, stride, (float)fovy, T, x0, y0, cell, nx, ny, zl, zh, 1024, 0, &ba);
    emulate(depth, W, H, stride, (float)fovy, T, x0, y0, cell, nx, ny, zl, zh, 100, 1, &ba);
    CHECK(same(ab, ba), "accumulate depends on the order");
    for (size_t q = 0; q < nc; q++) {
      const float want = std::isnan(a.z[q]) ? b.z[q] : std::isnan(b.z[q]) ? a.z[q] : std::max(a.z[q], b.z[q]);
      CHECK(to_bits(ab.z[q]) == to_bits(want) && ab.n[q] == a.n[q] + b.n[q], "cell %zu: accumulate gives (%g, %d), the parts (%g, %d) and (%g, %d)", q, ab.z[q],
            ab.n[q], a.z[q], a.n[q], b.z[q], b.n[q]);
    }
  }
}

int main() {
  check_key();
  check_cell_rule();
  check_bands();
  check_store_split();
  check_scatter(37, 23, 1, 64, 64, 0.05f, -1.613f, -1.587f, -0.05f, 1.0f, 1);
  check_scatter(424, 240, 1, 64, 64, 0.05f, -1.613f, -1.587f, -0.05f, 1.0f, 2);
  check_scatter(424, 240, 3, 16, 12, 0.05f, 0.487f, -0.313f, -0.05f, 1.0f, 3);
  check_scatter(480, 270, 3, 64, 96, 0.0625f, -1.613f, -2.587f, -INF, INF, 4);
  check_scatter(37, 23, 1, 1, 1, 1e6f, -5e5f, -5e5f, -INF, INF, 5);
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
