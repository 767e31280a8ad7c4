// Exact squared Euclidean distance fields of occupancy grids (smj_occupancy_to_distance, include/smj_distance.h): the obstacle
// predicate, the row rule on a bit mask, the column rule with its tie order and stop condition, and the cut of a grid into column
// strips as plain inline functions.  The kernel of smj_edt.hip calls exactly these; the header also compiles under a host compiler,
// so tests/edt/edt_check.cpp runs the shipped code serially against brute force.  Integers only.
//
// The rule.  Per cell (y, x) the lexicographic minimum over obstacle cells (j, i) of ((y - j)^2 + (x - i)^2, j nx + i): the squared
// distance in cells and, among equal distances, the smallest linear index.  It separates into two passes:
//   rows:     off[j][x] = i - x of the obstacle i of row j nearest to x, the LEFT one of two at equal distance (the smaller index);
//   columns:  the minimum over rows j of (off[j][x]^2 + (y - j)^2, j nx + x + off[j][x]), by the full lexicographic compare, so the
//             order in which the rows are visited does not matter.
// With a bound R > 0 a cell whose minimum exceeds R^2 has none; offsets beyond R and rows beyond R can then be left out early.
#pragma once
#include "smj_grid.h"   // SMJ_GRID_HD and the store's 16-byte groups

// SMJ_EDT_NONE: dist2 of a cell with no obstacle (in reach); = SMJ_DIST_NONE of the public header.  The largest grid, the longest
// side (row offsets fit int16, dist2 < 2^25), the cells of one strip (int16 offsets: 32 KiB of LDS) and the offset of "none".
enum { SMJ_EDT_NONE = 1 << 30, SMJ_EDT_MAX_CELLS = 65536, SMJ_EDT_MAX_SIDE = 4096, SMJ_EDT_STRIP_CELLS = 16384, SMJ_EDT_NO_OFF = -32768 };
enum { SMJ_EDT_MASK_WORDS = SMJ_EDT_MAX_CELLS / 64 };   // the obstacle mask of a whole grid: bit c of the mask is cell c, 8 KiB

// Obstacle: hit >= min_hits, or -- with unknown_is_obstacle and a miss layer -- a cell no ray has seen (hit == 0 && miss == 0).
SMJ_GRID_HD bool smj_edt_obstacle(int hit, int miss, int have_miss, int min_hits, int unknown_is_obstacle) {
  return hit >= min_hits || (unknown_is_obstacle && have_miss && hit == 0 && miss == 0);
}

// Column strips.  A workgroup holds the offsets of [ny] x [w] cells, ny w <= SMJ_EDT_STRIP_CELLS: the fewest strips that allow it,
// of equal width (the last one may be narrower).  ny <= 4096 leaves w >= 4.  128 x 128 is one strip, 256 x 256 four of 64 columns.
struct smj_edt_strip_t { int c0, w; };
SMJ_GRID_HD int smj_edt_strip_width(int nx, int ny) {
  const int wmax = SMJ_EDT_STRIP_CELLS / ny;
  const int n = (nx + wmax - 1) / wmax;
  return (nx + n - 1) / n;
}
SMJ_GRID_HD int smj_edt_strips(int nx, int ny) {
  const int w = smj_edt_strip_width(nx, ny);
  return (nx + w - 1) / w;
}
SMJ_GRID_HD smj_edt_strip_t smj_edt_strip(int nx, int ny, int s) {
  smj_edt_strip_t t;
  const int w = smj_edt_strip_width(nx, ny);
  t.c0 = s * w;
  t.w = nx - t.c0 < w ? nx - t.c0 : w;
  return t;
}

// The highest set bit of the mask in [lo, pos], or -1; the lowest set bit in [pos, hi], or -1.  lo <= pos <= hi, all inside the mask.
SMJ_GRID_HD int smj_edt_prev(const unsigned long long* mask, int lo, int pos) {
  int wi = pos >> 6;
  const int wlo = lo >> 6;
  unsigned long long bits = mask[wi] & (~0ull >> (63 - (pos & 63)));
  for (;;) {
    if (wi == wlo) bits &= ~0ull << (lo & 63);
    if (bits) return (wi << 6) + 63 - __builtin_clzll(bits);
    if (wi == wlo) return -1;
    bits = mask[--wi];
  }
}
SMJ_GRID_HD int smj_edt_next(const unsigned long long* mask, int pos, int hi) {
  int wi = pos >> 6;
  const int whi = hi >> 6;
  unsigned long long bits = mask[wi] & (~0ull << (pos & 63));
  for (;;) {
    if (wi == whi) bits &= ~0ull >> (63 - (hi & 63));
    if (bits) return (wi << 6) + __builtin_ctzll(bits);
    if (wi == whi) return -1;
    bits = mask[++wi];
  }
}

// The row rule: the signed offset from cell (y, x) to the nearest obstacle of row y, ties to the left; SMJ_EDT_NO_OFF if the row has
// none -- or, with R > 0, none within R cells (such a one cannot give dist2 <= R^2).  The mask is that of the whole grid, so the
// search crosses the edges of a strip.
SMJ_GRID_HD int smj_edt_row_offset(const unsigned long long* mask, int nx, int y, int x, int R) {
  const int row = y * nx, pos = row + x;
  int lo = row, hi = row + nx - 1;
  if (R > 0) {
    if (pos - R > lo) lo = pos - R;
    if (pos + R < hi) hi = pos + R;
  }
  const int l = smj_edt_prev(mask, lo, pos), r = smj_edt_next(mask, pos, hi);
  if (l < 0 && r < 0) return SMJ_EDT_NO_OFF;
  if (r < 0 || (l >= 0 && pos - l <= r - pos)) return l - pos;
  return r - pos;
}

// The column rule for cell (y, x): off points at column x's offsets, off[j * stride] that of row j.  Only rows jlo <= j <= jhi are
// read: the caller guarantees that every other row of this column holds SMJ_EDT_NO_OFF (jlo > jhi: no row holds anything).  The
// search goes outward from row y, the row above before the row below, and stops at the first dy with dy^2 > best (strictly: at
// dy^2 == best the cell straight above still wins by its smaller index), with dy > R, or with both rows outside [jlo, jhi].
// Candidates are compared as (dist2, index), so the result does not depend on that order.  R > 0: a minimum above R^2 is none.
SMJ_GRID_HD void smj_edt_column(const int16_t* off, int stride, int nx, int y, int x, int jlo, int jhi, int R, int* dist2, int* nearest) {
  int best = SMJ_EDT_NONE, at = -1;
  if (jlo <= jhi) {
    if (y >= jlo && y <= jhi) {
      const int o = off[y * stride];
      if (o != SMJ_EDT_NO_OFF) { best = o * o; at = y * nx + x + o; }
    }
    int dy = y < jlo ? jlo - y : y > jhi ? y - jhi : 1;   // the nearer rows hold nothing
    for (; dy * dy <= best && (R <= 0 || dy <= R); dy++) {
      const int ja = y - dy, jb = y + dy;
      if (ja < jlo && jb > jhi) break;
      if (ja >= jlo && ja <= jhi) {
        const int o = off[ja * stride];
        if (o != SMJ_EDT_NO_OFF) {
          const int d = o * o + dy * dy, k = ja * nx + x + o;
          if (d < best || (d == best && k < at)) { best = d; at = k; }
        }
      }
      if (jb >= jlo && jb <= jhi) {
        const int o = off[jb * stride];
        if (o != SMJ_EDT_NO_OFF) {
          const int d = o * o + dy * dy, k = jb * nx + x + o;
          if (d < best || (d == best && k < at)) { best = d; at = k; }
        }
      }
    }
    if (R > 0 && best > R * R) { best = SMJ_EDT_NONE; at = -1; }
  }
  *dist2 = best;
  *nearest = at;
}

#if defined(__HIPCC__)
// Launch (smj_edt.hip).  miss and nearest may be null.
void smj_launch_edt(int num_envs, const int* hit, const int* miss, int nx, int ny, int min_hits, int unknown_is_obstacle, int R,
                    int* dist2, int* nearest, hipStream_t stream);
#endif
