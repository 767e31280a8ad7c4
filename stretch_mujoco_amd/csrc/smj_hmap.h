// Egocentric height maps from the depth images (smj_depth_to_heightmap, include/smj_heightmap.h): the binning rule, the
// order-preserving key of z and the cut of a grid into bands as plain inline functions.  The kernel of smj_hmap.hip calls exactly
// these (and smj_points.h for the point of a pixel); the header also compiles under a host compiler, so tests/hmap/hmap_check.cpp
// checks the shipped code against long-hand fp64.
//
// Conventions.  The grid is [ny][nx] cells of side `cell`, row-major, rows follow y: cell (iy, ix) covers
// [x0 + ix cell, x0 + (ix + 1) cell) x [y0 + iy cell, y0 + (iy + 1) cell).  Per cell: the largest z of the points that fall into it
// with z_lo <= z <= z_hi, and their number.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "smj_points.h"

// Cells that one workgroup holds in LDS (smj_hmap.hip has the reasoning): 8 bytes per cell, 32 KiB.  A 64 x 64 grid is one band.
enum { SMJ_HMAP_BAND_CELLS = 4096, SMJ_HMAP_MAX_CELLS = 65536 };

// Order-preserving key of a float: a < b (as floats, -0 < +0 included) <=> key(a) < key(b) as unsigned, over every non-NaN value
// (+-0, denormals, +-inf).  Key 0 would be the bit pattern 0xffffffff, a NaN: no number produces it, so 0 means "empty".
SMJ_PT_HD uint32_t smj_hmap_key(float z) {
  uint32_t bits;
  memcpy(&bits, &z, 4);
  return bits ^ (bits >> 31 ? 0xffffffffu : 0x80000000u);
}

SMJ_PT_HD float smj_hmap_unkey(uint32_t key) {   // inverse of smj_hmap_key; key 0 (empty) -> a quiet NaN
  if (key == 0u) return __builtin_nanf("");
  const uint32_t bits = key ^ (key >> 31 ? 0x80000000u : 0xffffffffu);
  float z;
  memcpy(&z, &bits, 4);
  return z;
}

// start value of a cell's key with accumulate: what the buffer holds, NaN meaning empty
SMJ_PT_HD uint32_t smj_hmap_key_of_stored(float z) { return z != z ? 0u : smj_hmap_key(z); }

// The binning rule.  inv_cell = 1.f / cell, rounded once on the host.  Every compare is a float compare made before any conversion to
// int, so a NaN, an infinity or a value beyond the int range fails one of them and nothing undefined is evaluated.
SMJ_PT_HD bool smj_hmap_cell(float x, float y, float z, float x0, float y0, float inv_cell, int nx, int ny, float z_lo, float z_hi,
                             int* ix, int* iy) {
  const float fx = floorf((x - x0) * inv_cell), fy = floorf((y - y0) * inv_cell);
  if (!(fx >= 0.f && fx < (float)nx && fy >= 0.f && fy < (float)ny && z >= z_lo && z <= z_hi)) return false;
  *ix = (int)fx;
  *iy = (int)fy;
  return true;
}

// One pixel: depth d at image pixel (u, v) -> kept or not, its cell and z.  T as smj_points_transform gives it.  An invalid depth
// gives NaN coordinates (smj_points_point), which smj_hmap_cell drops.
SMJ_PT_HD bool smj_hmap_pixel(float d, int u, int v, int width, int height, float th, float aspect, const float* T, float x0, float y0,
                              float inv_cell, int nx, int ny, float z_lo, float z_hi, int* ix, int* iy, float* z) {
  float xn, yn, p[3];
  smj_points_dir(u, v, width, height, th, aspect, &xn, &yn);
  smj_points_point(d, xn, yn, T, p);
  *z = p[2];
  return smj_hmap_cell(p[0], p[1], p[2], x0, y0, inv_cell, nx, ny, z_lo, z_hi, ix, iy);
}

// Bands.  A grid of more than `cap` cells is cut into bands of whole rows: rows_per_band = cap / nx.  (A row longer than cap, which
// only a grid of a few very long rows has, is cut into pieces of cap columns; a band is then one such piece.)  Either way a band is
// a rectangle rows [r0, r0 + rows) x columns [c0, c0 + cols) whose cells are CONTIGUOUS in the row-major grid, from flat index
// r0 nx + c0 on: rows > 1 only where cols == nx.
struct smj_hmap_band_t { int r0, rows, c0, cols; };

SMJ_PT_HD int smj_hmap_col_pieces(int nx, int cap) { return nx <= cap ? 1 : (nx + cap - 1) / cap; }
SMJ_PT_HD int smj_hmap_rows_per_band(int nx, int cap) { return nx <= cap ? cap / nx : 1; }
SMJ_PT_HD int smj_hmap_bands(int nx, int ny, int cap) {
  const int rpb = smj_hmap_rows_per_band(nx, cap);
  return ((ny + rpb - 1) / rpb) * smj_hmap_col_pieces(nx, cap);
}
SMJ_PT_HD smj_hmap_band_t smj_hmap_band(int nx, int ny, int cap, int band) {
  const int pieces = smj_hmap_col_pieces(nx, cap), rpb = smj_hmap_rows_per_band(nx, cap);
  smj_hmap_band_t b;
  b.r0 = (band / pieces) * rpb;
  b.rows = ny - b.r0 < rpb ? ny - b.r0 : rpb;
  b.c0 = (band % pieces) * cap;
  b.cols = pieces == 1 ? nx : (nx - b.c0 < cap ? nx - b.c0 : cap);
  return b;
}
// cell (iy, ix) -> its slot in the band's arrays, or -1 if the band does not hold it; the flat grid index is r0 nx + c0 + slot
SMJ_PT_HD int smj_hmap_slot(smj_hmap_band_t b, int ix, int iy) {
  const unsigned r = (unsigned)(iy - b.r0), c = (unsigned)(ix - b.c0);
  return r < (unsigned)b.rows && c < (unsigned)b.cols ? (int)(r * (unsigned)b.cols + c) : -1;
}

// The store of a band of ncell 4-byte cells to the address `out` (4-byte aligned): `lead` single cells up to the first 16-byte
// boundary, `groups` groups of four cells from there (16-byte stores), and the tail from cell tail0 on.  The `rest` = lead + tail
// single cells (at most 6) are numbered t = 0 .. rest - 1 by smj_hmap_split_rest.  Every cell is stored exactly once.
struct smj_hmap_split_t { int lead, groups, tail0, rest; };

SMJ_PT_HD smj_hmap_split_t smj_hmap_store_split(uintptr_t out, int ncell) {
  smj_hmap_split_t s;
  s.lead = (int)((16u - (unsigned)(out & 15u)) & 15u) >> 2;
  if (s.lead > ncell) s.lead = ncell;
  s.groups = (ncell - s.lead) >> 2;
  s.tail0 = s.lead + 4 * s.groups;
  s.rest = s.lead + (ncell - s.tail0);
  return s;
}
SMJ_PT_HD int smj_hmap_split_rest(smj_hmap_split_t s, int t) { return t < s.lead ? t : s.tail0 + (t - s.lead); }

#if defined(__HIPCC__)
// Launch (smj_hmap.hip).  kind / body as smj_launch_points; count may be null.
void smj_launch_hmap(const float* xpose, long ld, int num_envs, const int* cam_bodyid, const float* cam_pos, const float* cam_mat,
                     int cam, int width, int height, float fovy_deg, const float* depth, int stride, int kind, int body, float x0,
                     float y0, float cell, int nx, int ny, float z_lo, float z_hi, int accumulate, float* zmax, int* count,
                     hipStream_t stream);
#endif
