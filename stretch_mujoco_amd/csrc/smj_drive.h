// Base commands from navigation fields (smj_navigation_to_velocity, include/smj_drive.h): a trajectory-rollout local planner.  The
// cell of a point, what a swept point and the scoring point contribute, the blocked predicate, the score, the (score, k) order and
// the status of an env, as plain inline functions.  The kernel of smj_drive.hip calls exactly these; the header also compiles under
// a host compiler, so tests/drive/drive_check.cpp runs the shipped code serially against its own double loop.
//
// The rule.  A candidate k is a command (v_k, w_k), P - 1 swept points and one scoring point, all in the robot's frame and shared
// by every env.  It is blocked iff a swept point lies on a cell with cost >= lethal, or outside the grid unless outside_is_free, or
// its scoring point is outside or on a cell whose potential is SMJ_NAV_NONE, or the command is out of reach of the current twist.
// Otherwise score_k = goal_weight * potential[scoring cell] + obstacle_weight * max swept cost + bias_k in 64 bits.  The smallest
// score wins, the smallest k among equal scores.  Only the cell of a point uses floats; the rest is integers and fp32 compares.
#pragma once
#include <math.h>
#include "smj_grid.h"   // SMJ_GRID_HD

// The limits: candidates, points per candidate and table entries (a workgroup walks the table once; 32768 entries are 128 rounds of
// 256 threads), the grid limits of the navigation entry whose potential is read here, and the largest weight: with g < 2^30,
// o <= 255 and |bias| < 2^31 the score stays below 65535 * 2^30 + 65535 * 255 + 2^31 < 2^47.
enum { SMJ_DRIVE_MAX_CANDIDATES = 1024, SMJ_DRIVE_MAX_POINTS = 256, SMJ_DRIVE_MAX_TABLE = 32768, SMJ_DRIVE_MAX_CELLS = 65536, SMJ_DRIVE_MAX_SIDE = 4096,
       SMJ_DRIVE_MAX_WEIGHT = 65535 };
// The public header's macros, token for token, so that a translation unit may include both.
#define SMJ_DRIVE_OK 0
#define SMJ_DRIVE_ARRIVED 1
#define SMJ_DRIVE_BLOCKED 2
#define SMJ_DRIVE_OFF_GRID 3
#define SMJ_DRIVE_NO_SCORE 0x7fffffffffffffffLL
// the potential of a cell without a path: SMJ_NAV_NONE of include/smj_navigation.h (smj_capi.hip holds the two together)
enum { SMJ_DRIVE_NAV_NONE = 1 << 30 };
// What a swept point contributes to its candidate: its cell's cost (0 .. 255), or SMJ_DRIVE_SWEPT_BLOCKS, which is above every
// cost, so that one maximum over the swept points carries both the largest cost and whether any of them blocks.
enum { SMJ_DRIVE_SWEPT_BLOCKS = 256 };

SMJ_GRID_HD bool smj_drive_finite(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN

// A point of the robot's frame in the grid's frame: (x + c px - s py, y + s px + c py), c = cosf(theta), s = sinf(theta).
SMJ_GRID_HD float smj_drive_world_x(float x, float c, float s, float px, float py) { return x + c * px - s * py; }
SMJ_GRID_HD float smj_drive_world_y(float y, float c, float s, float px, float py) { return y + s * px + c * py; }

// The linear cell iy nx + ix of a point of the grid's frame, ix = floor((wx - x0) / cell), iy = floor((wy - y0) / cell); -1 when the
// point is not finite or off the grid.  The compares run on the floats, so no out-of-range value is ever converted.
SMJ_GRID_HD int smj_drive_cell(float wx, float wy, float x0, float y0, float cell, int nx, int ny) {
  const float fx = floorf((wx - x0) / cell), fy = floorf((wy - y0) / cell);
  if (!(fx >= 0.0f && fx < (float)nx && fy >= 0.0f && fy < (float)ny)) return -1;
  return (int)fy * nx + (int)fx;
}

// A swept point on `cell` (-1: outside), whose cost is `cost` (read only where cell >= 0; 0 without a cost layer).
SMJ_GRID_HD int smj_drive_swept(int cell, int cost, int lethal, int outside_is_free) {
  if (cell < 0) return outside_is_free ? 0 : SMJ_DRIVE_SWEPT_BLOCKS;
  return cost >= lethal ? SMJ_DRIVE_SWEPT_BLOCKS : cost;
}

// The dynamic window, in fp32 exactly as the public header writes it: a NaN anywhere makes it false.
SMJ_GRID_HD bool smj_drive_in_window(float vk, float wk, float v, float w, float max_dv, float max_dw) {
  return fabsf(vk - v) <= max_dv && fabsf(wk - w) <= max_dw;
}

// swept: the maximum of smj_drive_swept over the candidate's swept points (0 when it has none); goal: the potential at the scoring
// point, SMJ_DRIVE_NAV_NONE when that point is outside; in_window: true without a twist.
SMJ_GRID_HD bool smj_drive_is_blocked(int swept, int goal, bool in_window) {
  return swept >= SMJ_DRIVE_SWEPT_BLOCKS || goal >= SMJ_DRIVE_NAV_NONE || !in_window;
}

SMJ_GRID_HD long long smj_drive_score(int swept, int goal, bool in_window, int goal_weight, int obstacle_weight, int bias) {
  if (smj_drive_is_blocked(swept, goal, in_window)) return SMJ_DRIVE_NO_SCORE;
  return (long long)goal_weight * goal + (long long)obstacle_weight * swept + bias;
}

// The order of the candidates: (score, k) ascending.  A total order, so the minimum does not depend on how it is reduced.
SMJ_GRID_HD bool smj_drive_before(long long sa, int ka, long long sb, int kb) { return sa < sb || (sa == sb && ka < kb); }

// The status of an env.  own_cell: the cell of (x, y), -1 outside; own_potential: the potential there (read only where
// own_cell >= 0); best_score: the minimum over the candidates.
SMJ_GRID_HD int smj_drive_status(bool pose_finite, int own_cell, int own_potential, int arrive_potential, long long best_score) {
  if (!pose_finite || own_cell < 0) return SMJ_DRIVE_OFF_GRID;
  if (own_potential <= arrive_potential) return SMJ_DRIVE_ARRIVED;
  return best_score == SMJ_DRIVE_NO_SCORE ? SMJ_DRIVE_BLOCKED : SMJ_DRIVE_OK;
}

// The schedule: table entry i = k P + p is handled in round i / threads by thread i % threads (consecutive lanes, consecutive
// entries), candidate k's score by thread k % threads.
SMJ_GRID_HD int smj_drive_rounds(int n, int threads) { return (n + threads - 1) / threads; }

#if defined(__HIPCC__)
// Launch (smj_drive.hip).  twist, cost, bias, score and cell_out may be null.
void smj_launch_drive(int num_envs, const float* pose, const float* twist, const uint8_t* cost, const int* potential, int nx, int ny, float x0, float y0,
                      float cell, const float* command, const float* point, const int* bias, int K, int P, int lethal, int outside_is_free,
                      int goal_weight, int obstacle_weight, int arrive_potential, float max_dv, float max_dw, float* cmd, int* best, long long* score,
                      int* cell_out, hipStream_t stream);
#endif
