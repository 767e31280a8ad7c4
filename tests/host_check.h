// What the host check programs of the device headers share (tests/{points,hmap,occ,edt,nav}/*_check.cpp): the CHECK macro with its
// failure counter, the special floats and bit casts, a pose of fp32 numbers with a seeded random one, the cover of the store groups,
// the cover of the field copy's split.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

static int failures = 0;
#define CHECK(cond, ...)                                \
  do {                                                  \
    if (!(cond)) {                                      \
      if (failures++ < 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    }                                                   \
  } while (0)

static inline float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
static inline uint32_t to_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static const float INF = std::numeric_limits<float>::infinity();
static const float NaN = std::numeric_limits<float>::quiet_NaN();

struct Pose { float p[3], m[9]; };

static inline Pose random_pose(std::mt19937& g, double reach) {
  std::normal_distribution<double> n(0, 1);
  std::uniform_real_distribution<double> t(-reach, reach);
  double q[4], s = 0;
  for (double& x : q) { x = n(g); s += x * x; }
  for (double& x : q) x /= std::sqrt(s);
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y), 2 * (x * y + w * z), 1 - 2 * (x * x + z * z),
                       2 * (y * z - w * x), 2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)};
  Pose P;
  for (int k = 0; k < 9; k++) P.m[k] = (float)R[k];
  for (int k = 0; k < 3; k++) P.p[k] = (float)t(g);
  return P;
}

// The store's groups (csrc/smj_grid.h, handed in so that this header needs none of the device headers): for every run of
// n = 1 .. NMAX cells and every alignment al = 0 .. 3, each index in [0, n) lies in exactly one of the groups k = 0 .. groups(n) - 1.
template <int NMAX, class Groups, class First>
static void check_store_groups(Groups groups, First first) {
  for (int n = 1; n <= NMAX; n++)
    for (int al = 0; al < 4; al++)
      for (int c = 0; c < n; c++) {
        int holders = 0;
        for (int k = 0; k < groups(n); k++) holders += first(k, al) <= c && c < first(k, al) + 4;
        CHECK(holders == 1, "groups of %d cells al %d: cell %d in %d groups", n, al, c, holders);
      }
}

// The split of the copy of an env's byte field into LDS (csrc/smj_scan.h, handed in): for every alignment 0 .. 15 of the global
// address and every ncell = 0 .. CELLS, each byte is copied exactly once (lead bytes, groups of 16, the tail), every group starts on
// a multiple of 16 in both address spaces (LDS byte sh + i holds byte i), and the copy stays within s_raw[CELLS + 16].
template <int CELLS, class Split>
static void check_stage_split(Split split) {
  for (int al = 0; al < 16; al++)
    for (int ncell = 0; ncell <= CELLS; ncell++) {
      const uintptr_t g = 0x7f3c5000u + (uintptr_t)al;
      const auto s = split(g, ncell);
      int copies[CELLS + 16] = {};
      CHECK(s.sh == al && s.lead >= 0 && s.lead < 16 && s.lead <= ncell && s.groups >= 0 && s.tail == s.lead + 16 * s.groups && s.tail <= ncell && ncell - s.tail < 16,
            "split of %d bytes at alignment %d: sh %d lead %d groups %d tail %d", ncell, al, s.sh, s.lead, s.groups, s.tail);
      for (int i = 0; i < s.lead && i < CELLS + 16; i++) copies[i]++;
      for (int q = 0; q < s.groups; q++) {
        const int first = s.lead + 16 * q;
        CHECK((g + (uintptr_t)first) % 16 == 0 && (s.sh + first) % 16 == 0, "group %d of %d bytes at alignment %d starts off a boundary", q, ncell, al);
        for (int i = first; i < first + 16 && i < CELLS + 16; i++) copies[i]++;
      }
      for (int i = s.tail; i < ncell; i++) copies[i]++;
      for (int i = 0; i < CELLS + 16; i++)
        CHECK(copies[i] == (i < ncell), "%d bytes at alignment %d: byte %d copied %d times", ncell, al, i, copies[i]);
      CHECK(ncell == 0 || s.sh + ncell - 1 < CELLS + 16, "%d bytes at alignment %d leave the LDS array", ncell, al);
    }
}
