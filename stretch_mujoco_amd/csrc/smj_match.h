// Correlative scan matching on likelihood fields (smj_scan_to_pose, include/smj_scanmatch.h).  The point of a ray, the placed test and
// the cell of a point, the clamp of a bias, the score J, the candidate index and its inverse, the (J, i) order, the status of an env
// and the output pose, as plain inline functions.  The kernel of smj_match.hip calls exactly these; the header also compiles under a
// host compiler, so tests/match/match_check.cpp runs the shipped code serially against its own loops.
//
// The rule.  The returns of a scan are points of the robot's frame (smj_occ.h forms the ray, this header its end).  A candidate is a
// rotation t of a table shared by all envs and a shift (dy, dx) in whole cells.  Per rotation every point is laid over the grid from
// the prior pose turned by angle[t] (smj_drive.h's transform) and gets a cell, or none when it lies more than 32 cells off the grid:
// then no allowed shift reaches the grid.  S is the sum of the field over the shifted cells that are on the grid and
// J = S - bias[t] - shift_weight (dx dx + dy dy).  The largest J wins, the smallest index among equal J.  Only the point and its cell
// use floats; the rest is integers.
#pragma once
#include <math.h>
#include "smj_occ.h"     // smj_occ_classify, smj_occ_ray
#include "smj_drive.h"   // SMJ_GRID_HD, smj_drive_finite, smj_drive_world_x / _y

// The limits: rotations, the window on either side (also the band round the grid in which a point keeps its cell), the weight of a
// shift, the rays of a scan (and so min_points), the largest bias, and the grid limits of the entries whose maps are matched here.
// With 1024 points of at most 255 the sum S stays below 2^18; bias <= 2^20 and shift_weight (dx dx + dy dy) <= 1024 * 2048 = 2^21
// keep J above -2^22.
enum { SMJ_MATCH_MAX_ANGLES = 64, SMJ_MATCH_MAX_WINDOW = 32, SMJ_MATCH_MAX_SHIFT_WEIGHT = 1024, SMJ_MATCH_MAX_POINTS = 1024,
       SMJ_MATCH_MAX_BIAS = 1 << 20, SMJ_MATCH_MAX_CELLS = 65536, SMJ_MATCH_MAX_SIDE = 4096 };
// The public header's macros, token for token, so that a translation unit may include both.
#define SMJ_MATCH_OK 0
#define SMJ_MATCH_FEW 1
#define SMJ_MATCH_OFF 2
#define SMJ_MATCH_NO_CELL (-32768)

// The end of a ray of length len in the frame of its origin o and direction d (smj_occ_ray), in fp32.
SMJ_GRID_HD void smj_match_point(const float* o, const float* d, float len, float* p) {
  p[0] = o[0] + len * d[0];
  p[1] = o[1] + len * d[1];
}

// The float index of a coordinate, as smj_drive_cell forms it before its range test.
SMJ_GRID_HD float smj_match_floor(float w, float origin, float cell) { return floorf((w - origin) / cell); }

// Placed: within SMJ_MATCH_MAX_WINDOW cells of the grid.  Compares of floats, so NaN and values no int holds are never converted.
SMJ_GRID_HD bool smj_match_placed(float fx, float fy, int nx, int ny) {
  const float w = (float)SMJ_MATCH_MAX_WINDOW;
  return fx >= -w && fx < (float)nx + w && fy >= -w && fy < (float)ny + w;   // nx + 32 <= 4128: exact
}

// The cell (ix, iy) of the point (px, py) of the robot's frame at pose (x, y) with c = cosf(theta_t), s = sinf(theta_t); both words
// SMJ_MATCH_NO_CELL when the point is not placed.
SMJ_GRID_HD bool smj_match_cell(float x, float y, float c, float s, float px, float py, float x0, float y0, float cell, int nx, int ny, int* ix,
                                int* iy) {
  const float fx = smj_match_floor(smj_drive_world_x(x, c, s, px, py), x0, cell), fy = smj_match_floor(smj_drive_world_y(y, c, s, px, py), y0, cell);
  const bool placed = smj_match_placed(fx, fy, nx, ny);
  *ix = placed ? (int)fx : SMJ_MATCH_NO_CELL;
  *iy = placed ? (int)fy : SMJ_MATCH_NO_CELL;
  return placed;
}

// A cell in one word, as the kernel keeps it in LDS: |ix|, |iy| <= 32768 fit 16 bits each.  SMJ_MATCH_NO_CELL packs like any other
// value and, shifted by at most 32, stays off every grid: a list that held it would sum the same (the kernel lists placed points only).
SMJ_GRID_HD int smj_match_pack(int ix, int iy) { return (int)(((unsigned)iy << 16) | ((unsigned)ix & 0xffffu)); }
SMJ_GRID_HD int smj_match_pack_x(int w) { return (int)(short)(w & 0xffff); }
SMJ_GRID_HD int smj_match_pack_y(int w) { return w >> 16; }

// What a placed point adds to S at shift (dy, dx): the linear cell to read, -1 when the shifted cell is off the grid.
SMJ_GRID_HD int smj_match_shifted(int ix, int iy, int dx, int dy, int nx, int ny) {
  const int sx = ix + dx, sy = iy + dy;
  return (unsigned)sx < (unsigned)nx && (unsigned)sy < (unsigned)ny ? sy * nx + sx : -1;
}

SMJ_GRID_HD int smj_match_bias(int b) { return b < 0 ? 0 : b > SMJ_MATCH_MAX_BIAS ? SMJ_MATCH_MAX_BIAS : b; }

// J of a candidate; `bias` is already clamped.
SMJ_GRID_HD int smj_match_score(int S, int bias, int shift_weight, int dx, int dy) { return S - bias - shift_weight * (dx * dx + dy * dy); }

// The candidate index i = (t (2 wy + 1) + (dy + wy)) (2 wx + 1) + (dx + wx) (below 64 * 65 * 65) and its inverse.
SMJ_GRID_HD int smj_match_index(int t, int dy, int dx, int wx, int wy) { return (t * (2 * wy + 1) + (dy + wy)) * (2 * wx + 1) + (dx + wx); }
SMJ_GRID_HD void smj_match_unindex(int i, int wx, int wy, int* t, int* dy, int* dx) {
  const int WX = 2 * wx + 1, WY = 2 * wy + 1, row = i / WX;
  *dx = i - row * WX - wx;
  *t = row / WY;
  *dy = row - *t * WY - wy;
}

// The order of the candidates: (J descending, i ascending).  A total order, so the first does not depend on how it is reduced.
SMJ_GRID_HD bool smj_match_before(int Ja, int ia, int Jb, int ib) { return Ja > Jb || (Ja == Jb && ia < ib); }

// The status of an env.  n: the returns whose point is finite.
SMJ_GRID_HD int smj_match_status(bool pose_finite, int n, int min_points) {
  if (!pose_finite) return SMJ_MATCH_OFF;
  return n < min_points ? SMJ_MATCH_FEW : SMJ_MATCH_OK;
}

// The output pose of the winner (t, dy, dx): the prior moved by whole cells, turned by angle[t].
SMJ_GRID_HD float smj_match_pose_xy(int shift, float cell, float prior) { return fmaf((float)shift, cell, prior); }
SMJ_GRID_HD float smj_match_pose_theta(float theta, float angle) { return theta + angle; }

#if defined(__HIPCC__)
// Launch (smj_match.hip).  bias, score and cell_out may be null.
struct SmjScanSource;   // smj_scan.h
void smj_launch_match(const SmjScanSource& src, int num_envs, int nlidar, int body, float r_min, float r_max, const uint8_t* field, int nx, int ny,
                      float x0, float y0, float cell, const float* pose, const float* angle, const int* bias, int T, int wx, int wy, int shift_weight,
                      int min_points, float* pose_out, int* best, int* score, int* cell_out, hipStream_t stream);
#endif
