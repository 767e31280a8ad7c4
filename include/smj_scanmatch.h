/* smj_scanmatch.h -- where in a map a scan was taken: correlative scan matching on likelihood fields (libsmj.so, HIP / gfx950).
 *
 * Part of the C-ABI: smj_drive.h includes this file, smj_frontier.h includes that one, and so on up to smj.h, so a caller includes
 * smj.h alone.  It is a header of its own because existing tests fix the include list of smj.h and the contents of the headers before
 * it; what is declared here is listed in lib.SCANMATCH_EXPORTS and held to the library by tests/test_scanmatch_capi.py.  Same rules as
 * smj.h: caller-owned device pointers, 0 on success, a negative code and smj_last_error otherwise, asynchronous on the caller's stream.
 */
#ifndef SMJ_SCANMATCH_H
#define SMJ_SCANMATCH_H
#include "smj.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The status of an env (best_dev), and both words of cell_dev for a ray that has no cell. */
#define SMJ_MATCH_OK 0
#define SMJ_MATCH_FEW 1
#define SMJ_MATCH_OFF 2
#define SMJ_MATCH_NO_CELL (-32768)

/* Per env the pose, out of a window of rotations and whole-cell shifts round a prior, at which the returns of a lidar scan collect
 * the largest reward from a likelihood field: the localisation step between the maps of this chain and everything that needs the
 * robot's pose in them.  num_envs and nlidar are the context's; the entry needs SMJ_SLOT_XPOSE bound (the rays' geometry in the
 * robot's frame is read from it) and the model's lidar tables; nlidar <= 1024.  No workspace, no global atomics.
 *
 * Inputs.
 * lidar_dev, lidar_ld: the scan as smj_lidar_to_occupancy takes it: float32 [nlidar][lidar_ld], range k of env e at k lidar_ld + e.
 * frame: a fused body id >= 0, the robot's frame; SMJ_FRAME_WORLD and SMJ_FRAME_CAMERA are refused.
 * r_min, r_max: finite, 0 <= r_min <= r_max, r_max / cell <= 8192, as that entry refuses them.
 * field_dev: uint8 [num_envs][ny][nx], any alignment, row-major, rows follow y: the reward of a scan point that lands in the cell.
 * nx, ny in [1, 4096] and nx ny <= 65536; cell finite and > 0; x0, y0 finite: the corner of cell (0, 0).
 * pose_dev: float32 [3][num_envs], rows x, y, theta: the prior in the grid's frame -- the layout of SMJ_SLOT_BASE_POSE.
 * angle_dev: float32 [T], rotation offsets SHARED BY ALL ENVS, T = num_angles in [1, 64]; angle_bias_dev: int32 [T] or null (0), each
 * value read as min(max(b, 0), 1 << 20).
 * wx, wy in [0, 32]: the shifts in whole cells, dx in [-wx, wx], dy in [-wy, wy]; shift_weight in [0, 1024]; min_points in [1, 1024].
 *
 * The points of a scan -- floats, once per env.  Ray k counts when its range is a return (r_min <= r <= r_max); its point is
 * p = o + r d in fp32, with origin o and direction d of the rangefinder in the body `frame`, as smj_lidar_to_occupancy forms them
 * there.  n is the number of returns whose p is finite.
 *
 * Placing, per rotation t -- the only other floats.  theta_t = theta + angle[t]; with c = cosf(theta_t), s = sinf(theta_t) (the
 * accurate functions) the point lies at (x + c px - s py, y + s px + c py) =: (gx, gy), and fx = floorf((gx - x0) / cell),
 * fy = floorf((gy - y0) / cell), all in fp32.  The point is PLACED iff -32 <= fx < nx + 32 and -32 <= fy < ny + 32 (compares of
 * floats: NaN is never converted; outside that band no allowed shift reaches the grid); its cell is then (ix, iy) = ((int)fx, (int)fy).
 *
 * The score -- integers.  S(t, dy, dx) is the sum of field[iy + dy][ix + dx] over the placed points whose shifted cell is on the
 * grid; J = S - bias[t] - shift_weight (dx dx + dy dy) in int32 (S < 2^18, so J > -2^22).  The candidate index is
 * i = (t (2 wy + 1) + (dy + wy)) (2 wx + 1) + (dx + wx).
 * THE LARGEST J WINS; AMONG EQUAL J THE SMALLEST i WINS.
 *
 * Per env the status:
 *   SMJ_MATCH_OFF  x, y or theta is not finite;
 *   SMJ_MATCH_FEW  otherwise, n < min_points;
 *   SMJ_MATCH_OK   otherwise.
 *
 * Outputs.
 * pose_out_dev: float32 [3][num_envs], required.  With SMJ_MATCH_OK (fmaf((float)dx, cell, x), fmaf((float)dy, cell, y), theta_t) of
 * the winner; otherwise the prior, bit for bit.
 * best_dev: int32 [num_envs][4], required: the winner's i (-1 unless SMJ_MATCH_OK), its J (0 unless SMJ_MATCH_OK), n, the status.
 * score_dev: int32 [num_envs][T][2 wy + 1][2 wx + 1], or null: J of every candidate as evaluated, whatever the status.
 * cell_dev: int32 [num_envs][T][nlidar][2], or null: (ix, iy) of every ray and rotation; both words SMJ_MATCH_NO_CELL for a ray that
 * is no return or is not placed.
 * A null score_dev or cell_dev is left untouched.  Every output is unique, so two calls give identical bits whatever the order of
 * evaluation; the inputs are unchanged; nothing outside the outputs is written (one workgroup per env).
 * Errors: -1 for a null lidar_dev / field_dev / pose_dev / angle_dev / pose_out_dev / best_dev, a pointer not aligned to 4 bytes
 * (field_dev excepted), nlidar > 1024, lidar_ld < num_envs, a frame that is no body id or a body id >= nbody, any limit above, an
 * output range that overlaps an input range or another output (the bound SMJ_SLOT_XPOSE is an input: its range runs from its first
 * word to env num_envs-1 of its last row, as the scan's does -- columns beyond num_envs of the last row are free for an output); -5
 * when SMJ_SLOT_XPOSE is not bound; -6 for a model without lidar tables.  A refused call writes nothing. */
int smj_scan_to_pose(smj_ctx* ctx, const void* lidar_dev, long lidar_ld, int frame, float r_min, float r_max,
                     const void* field_dev, int nx, int ny, float x0, float y0, float cell,
                     const void* pose_dev, const void* angle_dev, const void* angle_bias_dev, int num_angles,
                     int wx, int wy, int shift_weight, int min_points,
                     void* pose_out_dev, void* best_dev, void* score_dev, void* cell_dev, void* stream);

#ifdef __cplusplus
}
#endif
#include "smj_mapping.h"
#endif
