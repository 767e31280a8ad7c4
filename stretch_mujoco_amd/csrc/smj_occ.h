// 2-D occupancy grids from the lidar scan (smj_lidar_to_occupancy, include/smj_occupancy.h): the ray of a rangefinder in the
// requested frame, the classification of a range, the cells of a ray's end points and the closed-form line between them as plain
// inline functions.  The kernel of smj_occ.hip calls exactly these (and smj_hmap.h for the cut of the grid into bands); the header
// also compiles under a host compiler, so tests/occ/occ_check.cpp checks the shipped code against long-hand fp64.
//
// Conventions.  The grid is that of smj_hmap.h: [ny][nx] cells of side `cell`, row-major, rows follow y; it lies in the xy plane of
// the frame, z is not used.  Per cell two counts: `hit`, the rays that end in it on something, and `miss`, the rays that pass
// through it (or, for a ray without a return, end in it on nothing).
#pragma once
#include <math.h>
#include <stdint.h>

#include "smj_hmap.h"

// Cells one workgroup holds in LDS (8 bytes per cell, as the height map), the largest grid and the longest ray in cells.
enum { SMJ_OCC_BAND_CELLS = SMJ_HMAP_BAND_CELLS, SMJ_OCC_MAX_CELLS = 65536, SMJ_OCC_MAX_STEPS = 8192 };
enum { SMJ_OCC_WORLD = 0, SMJ_OCC_BODY = 1 };                    // frame kinds of smj_occ_ray
enum { SMJ_OCC_DROP = 0, SMJ_OCC_RETURN = 1, SMJ_OCC_CLEAR = 2 };   // what a range makes of its ray

// Classification: float compares on the range as stored, so there is no rounding.  NaN: dropped.  0 <= r < r_min: dropped (the ray
// ends on the robot itself).  r_min <= r <= r_max: a return, length r.  r < 0 (nothing hit) or r > r_max: no return -- with
// no_return_clears the ray is free over r_max and has no hit, without it the ray is dropped.
SMJ_PT_HD int smj_occ_classify(float r, float r_min, float r_max, int no_return_clears, float* len) {
  *len = 0.f;
  if (r != r) return SMJ_OCC_DROP;
  if (r >= r_min && r <= r_max) { *len = r; return SMJ_OCC_RETURN; }
  if (r >= 0.f && r < r_min) return SMJ_OCC_DROP;
  if (!no_return_clears) return SMJ_OCC_DROP;
  *len = r_max;
  return SMJ_OCC_CLEAR;
}

// Origin and direction of one rangefinder, as smj_lidar_kernel (smj_render.hip) forms them from the pose (bp, bm) of the site's
// body: o = bp + bm site_pos, d = bm lz with lz the site's +Z column, used as stored (not renormalised).  SMJ_OCC_BODY: expressed in
// the body with pose (fp, fm): o_F = fm' (o - fp), d_F = fm' d.  Only x and y are produced.
SMJ_PT_HD void smj_occ_ray(int kind, const float* bp, const float* bm, const float* site_pos, const float* lz, const float* fp,
                           const float* fm, float* o, float* d) {
  float ow[3], dw[3];
  for (int i = 0; i < 3; i++) {
    ow[i] = bp[i] + (bm[3 * i] * site_pos[0] + bm[3 * i + 1] * site_pos[1] + bm[3 * i + 2] * site_pos[2]);
    dw[i] = bm[3 * i] * lz[0] + bm[3 * i + 1] * lz[1] + bm[3 * i + 2] * lz[2];
  }
  if (kind == SMJ_OCC_WORLD) {
    o[0] = ow[0]; o[1] = ow[1];
    d[0] = dw[0]; d[1] = dw[1];
    return;
  }
  const float e[3] = {ow[0] - fp[0], ow[1] - fp[1], ow[2] - fp[2]};
  for (int i = 0; i < 2; i++) {
    o[i] = fm[i] * e[0] + fm[3 + i] * e[1] + fm[6 + i] * e[2];
    d[i] = fm[i] * dw[0] + fm[3 + i] * dw[1] + fm[6 + i] * dw[2];
  }
}

// One ray as the kernel walks it: the cells of its two ends and what it is.
struct smj_occ_line_t { int ax, ay, bx, by, kind; };

// The cells a = cell(o), b = cell(o + len d), by the rule of smj_hmap.h: floorf((x - x0) * inv_cell), every float compare before any
// conversion to int.  A ray whose origin's float index lies outside +-2^20 in either coordinate is dropped; so is one whose end lies
// more than 2 SMJ_OCC_MAX_STEPS cells from its origin, which takes a direction twice the unit length (the entry keeps
// r_max / cell <= SMJ_OCC_MAX_STEPS) or a pose that is not finite.  So |index| < 2^21 and 2 i d_min of smj_occ_cell stays below 2^30.
SMJ_PT_HD smj_occ_line_t smj_occ_line(int kind, const float* o, const float* d, float len, float x0, float y0, float inv_cell) {
  smj_occ_line_t L = {0, 0, 0, 0, SMJ_OCC_DROP};
  if (kind == SMJ_OCC_DROP) return L;
  const float fax = floorf((o[0] - x0) * inv_cell), fay = floorf((o[1] - y0) * inv_cell);
  if (!(fabsf(fax) <= 1048576.f && fabsf(fay) <= 1048576.f)) return L;
  const float ex = o[0] + len * d[0], ey = o[1] + len * d[1];
  const float fbx = floorf((ex - x0) * inv_cell), fby = floorf((ey - y0) * inv_cell);
  const float reach = 2.f * (float)SMJ_OCC_MAX_STEPS;
  if (!(fabsf(fbx - fax) <= reach && fabsf(fby - fay) <= reach)) return L;   // differences of integers below 2^22: exact
  L.ax = (int)fax; L.ay = (int)fay;
  L.bx = (int)fbx; L.by = (int)fby;
  L.kind = kind;
  return L;
}

// number of steps of the line: its cells are i = 0 .. n
SMJ_PT_HD int smj_occ_steps(smj_occ_line_t L) {
  const int dx = L.bx - L.ax, dy = L.by - L.ay;
  const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
  return adx > ady ? adx : ady;
}

// Cell i of the closed-form Bresenham line from a to b, 0 <= i <= n: the major coordinate is a + i s, the minor one
// a_min + s_min ((2 i d_min + n) / (2 n)) by integer division; x is the major axis when |dx| >= |dy|; n = 0 is the single cell a.
// Any (ray, i) is evaluated on its own: no running error term.
SMJ_PT_HD void smj_occ_cell(smj_occ_line_t L, int n, int i, int* ix, int* iy) {
  const int dx = L.bx - L.ax, dy = L.by - L.ay;
  const int adx = dx < 0 ? -dx : dx, ady = dy < 0 ? -dy : dy;
  const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1;
  if (n == 0) { *ix = L.ax; *iy = L.ay; return; }
  if (adx >= ady) {
    *ix = L.ax + i * sx;
    *iy = L.ay + sy * ((2 * i * ady + n) / (2 * n));
  } else {
    *iy = L.ay + i * sy;
    *ix = L.ax + sx * ((2 * i * adx + n) / (2 * n));
  }
}

// what cell i of the line adds to: 1 the hit layer, 0 the miss layer.  A return: miss for i < n, hit for i = n; a clearing ray: miss
SMJ_PT_HD int smj_occ_layer(smj_occ_line_t L, int n, int i) { return L.kind == SMJ_OCC_RETURN && i == n; }

#if defined(__HIPCC__)
// Launch (smj_occ.hip).  kind / body: SMJ_OCC_* and, for SMJ_OCC_BODY, the fused body; miss may be null.
struct SmjScanSource;   // smj_scan.h
void smj_launch_occ(const SmjScanSource& src, int num_envs, int nlidar, int kind, int body, float x0, float y0, float cell, int nx, int ny,
                    float r_min, float r_max, int no_return_clears, int accumulate, int* hit, int* miss, hipStream_t stream);
#endif
