/* smj_drive.h -- base commands from navigation fields: a trajectory-rollout local planner (libsmj.so, HIP / gfx950).
 *
 * Part of the C-ABI: smj_frontier.h includes this file, smj_navigation.h includes that one, and so on up to smj.h, so a caller includes
 * smj.h alone.  It is a header of its own because existing tests fix the include list of smj.h and the contents of the headers before
 * it; what is declared here is listed in lib.DRIVE_EXPORTS and held to the library by tests/test_drive_capi.py.  Same rules as smj.h:
 * caller-owned device pointers, 0 on success, a negative code and smj_last_error otherwise, asynchronous on the caller's stream.
 */
#ifndef SMJ_DRIVE_H
#define SMJ_DRIVE_H
#include "smj.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The status of an env (best_dev), and the score of a blocked candidate (score_dev): INT64_MAX. */
#define SMJ_DRIVE_OK 0
#define SMJ_DRIVE_ARRIVED 1
#define SMJ_DRIVE_BLOCKED 2
#define SMJ_DRIVE_OFF_GRID 3
#define SMJ_DRIVE_NO_SCORE 0x7fffffffffffffffLL

/* Per env the best of a table of candidate base commands, judged on the costmap and on the potential of smj_costmap_to_navigation:
 * the layer between that entry and set_base_velocity.  num_envs is the context's; the entry needs no bound slot, no model tables and
 * no workspace.
 *
 * Inputs.
 * pose_dev: float32 [3][num_envs], rows x, y, theta in the grid's frame -- the layout of SMJ_SLOT_BASE_POSE.
 * twist_dev: float32 [2][num_envs], rows v, w: the current velocity; or null: no dynamic window.
 * cost_dev: uint8 [num_envs][ny][nx], any alignment, or null: cost 0 everywhere.
 * potential_dev: int32 [num_envs][ny][nx], row-major, rows follow y, linear index c = y nx + x: what smj_costmap_to_navigation wrote.
 * nx, ny in [1, 4096] and nx ny <= 65536 (that entry's limits); cell finite and > 0; x0, y0 finite: the corner of cell (0, 0).
 * The candidate table, SHARED BY ALL ENVS: command_dev float32 [K][2], the (v, w) candidate k stands for; point_dev float32
 * [K][P][2], points (px, py) in the robot's frame, x forward, y left; bias_dev int32 [K], or null for 0.  K = num_candidates in
 * [1, 1024], P = num_points in [1, 256], K P <= 32768.  The first P - 1 points of a candidate are its swept points (arc samples, or
 * a footprint outline at every sample: the entry does not care), the last one is its scoring point.
 * 1 <= lethal <= 256; outside_is_free 0 or not; goal_weight, obstacle_weight in [0, 65535]; 0 <= arrive_potential < SMJ_NAV_NONE;
 * max_dv, max_dw >= 0 (+inf is fine), read only with twist_dev.
 *
 * Placing a point -- the only floats.  With the fp32 values c = cosf(theta), s = sinf(theta) (the accurate functions) a point lies
 * at wx = x + c px - s py, wy = y + s px + c py, in the cell ix = floor((wx - x0) / cell), iy = floor((wy - y0) / cell), all in fp32.
 * A point is OUTSIDE when wx or wy is not finite or the cell is off the grid.  The robot's own cell is that of (x, y).
 *
 * Per candidate k -- integers, and compares of fp32 values that need no rounding.  BLOCKED iff
 *   a swept point is on a cell with cost >= lethal, or
 *   a swept point is outside and outside_is_free == 0, or
 *   the scoring point is outside, or its cell's potential is SMJ_NAV_NONE, or
 *   twist_dev is given and !(fabsf(v_k - v) <= max_dv && fabsf(w_k - w) <= max_dw), in fp32 as written: a NaN twist blocks.
 * Otherwise o_k is the largest cost over the swept points (an outside-but-free point counts 0; 0 when P == 1), g_k the potential at
 * the scoring point and score_k = goal_weight g_k + obstacle_weight o_k + bias_k in 64 bits (below 2^47 in magnitude).
 *
 * Per env the status:
 *   SMJ_DRIVE_OFF_GRID  x, y or theta is not finite, or the own cell is outside;
 *   SMJ_DRIVE_ARRIVED   otherwise, potential[own cell] <= arrive_potential;
 *   SMJ_DRIVE_BLOCKED   otherwise, every candidate is blocked;
 *   SMJ_DRIVE_OK        otherwise.
 * THE SMALLEST SCORE WINS; AMONG EQUAL SCORES THE SMALLEST k WINS.
 *
 * Outputs.
 * cmd_dev: float32 [2][num_envs], required, rows v and w.  With status SMJ_DRIVE_OK the winner's command_dev row, bit for bit;
 * otherwise (0, 0).
 * best_dev: int32 [num_envs][2], required: the winner's k with status SMJ_DRIVE_OK, -1 otherwise; and the status.
 * score_dev: int64 [num_envs][K], or null: every candidate's score as evaluated, whatever the status; SMJ_DRIVE_NO_SCORE for a
 * blocked one.
 * cell_dev: int32 [num_envs][K][P], or null: the linear cell of every point, -1 when outside.
 * A null score_dev or cell_dev is left untouched.  Every output is unique, so two calls give identical arrays whatever the order of
 * evaluation; the inputs are unchanged; nothing outside the outputs is written (one workgroup per env, no global atomics).
 * Errors: -1 for a null pose_dev / potential_dev / command_dev / point_dev / cmd_dev / best_dev, a pointer not aligned to 4 bytes
 * (cost_dev excepted; score_dev: 8 bytes), nx or ny outside [1, 4096], nx ny > 65536, cell not finite or not > 0, x0 or y0 not
 * finite, num_candidates outside [1, 1024], num_points outside [1, 256], their product above 32768, lethal outside [1, 256], a weight
 * outside [0, 65535], arrive_potential outside [0, SMJ_NAV_NONE), max_dv or max_dw negative or NaN, an output range that overlaps an
 * input range or another output.  A refused call writes nothing. */
int smj_navigation_to_velocity(smj_ctx* ctx, const void* pose_dev, const void* twist_dev, const void* cost_dev, const void* potential_dev,
                               int nx, int ny, float x0, float y0, float cell,
                               const void* command_dev, const void* point_dev, const void* bias_dev, int num_candidates, int num_points,
                               int lethal, int outside_is_free, int goal_weight, int obstacle_weight, int arrive_potential,
                               float max_dv, float max_dw,
                               void* cmd_dev, void* best_dev, void* score_dev, void* cell_dev, void* stream);

#ifdef __cplusplus
}
#endif
#include "smj_scanmatch.h"
#endif
