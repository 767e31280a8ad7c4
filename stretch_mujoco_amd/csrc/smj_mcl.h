// Monte Carlo localisation on likelihood fields: the measurement update and the resampling step of a particle filter
// (smj_scan_to_particles, include/smj_localize.h).  What a point adds to the weight of a particle, the cut and the weight above it,
// the offset of a draw, the threshold of a slot, the ancestor of a threshold on an array of inclusive sums, the effective sample
// size and the status of an env, as plain inline functions.  The kernel of smj_mcl.hip calls exactly these; the header also compiles
// under a host compiler, so tests/mcl/mcl_check.cpp runs the shipped code serially against its own loops.
//
// The rule.  The returns of a scan are points of the robot's frame (smj_occ.h forms the ray, smj_match.h its end).  A particle is a
// pose of its own -- no lattice: every particle has its own sine and cosine.  Every point is laid over the grid from the particle by
// the matcher's chain at a rotation offset of 0 (smj_match_cell) and reads the field where it lands (smj_match_shifted at shift 0);
// S is the sum.  Only the point and its cell use floats.  From S on everything is integers: the best particle in the matcher's
// (S descending, j ascending) order, w = max(S - cut, 0) with cut = max(S_max - span, 0), and systematic resampling on the inclusive
// sums of w with one random word per env.
#pragma once
#include <math.h>
#include <stdint.h>
#include "smj_match.h"   // smj_match_point, smj_match_cell, smj_match_shifted, smj_match_before; smj_occ.h, smj_drive.h below it

// The limits: particles per env, the span of the weights, and the matcher's for the scan and the grid.  S < 2^18 (1024 points of at
// most 255), so w < 2^18, total < 2^30 and the sum of squares < 2^48.
enum { SMJ_MCL_MAX_PARTICLES = 4096, SMJ_MCL_MAX_SPAN = 1 << 18, SMJ_MCL_MAX_POINTS = SMJ_MATCH_MAX_POINTS, SMJ_MCL_STAT_WORDS = 8 };
// The public header's macros, token for token, so that a translation unit may include both.
#define SMJ_MCL_OK 0
#define SMJ_MCL_FEW 1
#define SMJ_MCL_LOST 2
// the words of an env's stat row
enum { SMJ_MCL_STAT_BEST = 0, SMJ_MCL_STAT_SMAX = 1, SMJ_MCL_STAT_N = 2, SMJ_MCL_STAT_STATUS = 3, SMJ_MCL_STAT_TOTAL = 4, SMJ_MCL_STAT_ESS = 5,
       SMJ_MCL_STAT_CUT = 6, SMJ_MCL_STAT_DISTINCT = 7 };

// A particle counts iff its three words are finite; any other has S = 0.
SMJ_GRID_HD bool smj_mcl_finite(float x, float y, float theta) { return smj_drive_finite(x) && smj_drive_finite(y) && smj_drive_finite(theta); }

// What the point (px, py) of the robot's frame adds to S of the particle (x, y) with c = cosf(theta), s = sinf(theta): the field
// under its cell, 0 when the cell is off the grid.  `field` is the env's [ny][nx] bytes.
SMJ_GRID_HD int smj_mcl_point_weight(float x, float y, float c, float s, float px, float py, float x0, float y0, float cell, int nx, int ny,
                                     const uint8_t* field) {
  int ix, iy;
  if (!smj_match_cell(x, y, c, s, px, py, x0, y0, cell, nx, ny, &ix, &iy)) return 0;
  const int at = smj_match_shifted(ix, iy, 0, 0, nx, ny);
  return at >= 0 ? (int)field[at] : 0;
}

// cut = max(S_max - span, 0) and w = max(S - cut, 0): the best particle keeps min(S_max, span), one that lies span below it nothing.
SMJ_GRID_HD int smj_mcl_cut(int s_max, int span) { return s_max > span ? s_max - span : 0; }
SMJ_GRID_HD int smj_mcl_w(int S, int cut) { return S > cut ? S - cut : 0; }

// The offset of the comb: o = (draw * total) >> 32 in 64 bits, so 0 <= o < total for total >= 1.
SMJ_GRID_HD unsigned smj_mcl_offset(unsigned draw, int total) { return (unsigned)(((uint64_t)draw * (uint64_t)(unsigned)total) >> 32); }

// The threshold of slot k: u_k = (k total + o) / P in 64 bits; below total for every k < P since o < total.
SMJ_GRID_HD int smj_mcl_threshold(int k, int total, unsigned o, int P) { return (int)(((uint64_t)(unsigned)k * (uint64_t)(unsigned)total + o) / (uint64_t)(unsigned)P); }

// The ancestor of a threshold: the smallest j with C[j] > u on the inclusive sums C[0 .. P-1] (non-decreasing, C[P-1] = total > u).
// A particle of weight 0 has C[j] = C[j-1] and is never the smallest.
SMJ_GRID_HD int smj_mcl_ancestor(const int* C, int P, int u) {
  int lo = 0, hi = P - 1;   // the answer lies in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (C[mid] > u) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The effective sample size floor(total^2 / sq), sq = sum of w^2 >= 1 (an env that is SMJ_MCL_OK has w >= 1 at its best particle).
SMJ_GRID_HD int smj_mcl_ess(int total, uint64_t sq) { return (int)(((uint64_t)(unsigned)total * (uint64_t)(unsigned)total) / sq); }

// The status of an env.  n: the returns whose point is finite; s_max: S of the best particle.
SMJ_GRID_HD int smj_mcl_status(int n, int min_points, int s_max) {
  if (n < min_points) return SMJ_MCL_FEW;
  return s_max == 0 ? SMJ_MCL_LOST : SMJ_MCL_OK;
}

#if defined(__HIPCC__)
// Launch (smj_mcl.hip).  noise, draw (when resample = 0), ancestor and pose_out may be null.  stage_field: the env's field is copied
// into LDS (0: gathered from global memory through L2).
struct SmjScanSource;   // smj_scan.h
void smj_launch_mcl(const SmjScanSource& src, int num_envs, int nlidar, int body, float r_min, float r_max, const uint8_t* field, int nx, int ny,
                    float x0, float y0, float cell, const float* particle, int P, const float* noise, const unsigned* draw, int span, int min_points,
                    int resample, float* particle_out, int* weight, int* ancestor, int* stat, float* pose_out, int stage_field, hipStream_t stream);
#endif
