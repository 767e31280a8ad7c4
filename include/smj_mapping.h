/* smj_mapping.h -- a lidar scan into a map at a pose handed in: the mapping step of on-device SLAM (libsmj.so, HIP / gfx950).
 *
 * Part of the C-ABI: smj_scanmatch.h includes this file, smj_drive.h includes that one, and so on up to smj.h, so a caller includes
 * smj.h alone.  It is a header of its own because existing tests fix the include list of smj.h and the contents of the headers before
 * it; what is declared here is listed in lib.MAPPING_EXPORTS and held to the library by tests/test_mapping_capi.py.  Same rules as
 * smj.h: caller-owned device pointers, 0 on success, a negative code and smj_last_error otherwise, asynchronous on the caller's stream.
 */
#ifndef SMJ_MAPPING_H
#define SMJ_MAPPING_H
#include "smj.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The status of an env (info_dev), and all four words of cell_dev for a ray that is not kept. */
#define SMJ_MAP_OK 0
#define SMJ_MAP_GATED 1
#define SMJ_MAP_OFF 2
#define SMJ_MAP_NO_CELL (-1073741824)

/* Per env the ray-traced occupancy counts of one lidar scan, laid into a map from a pose that is an INPUT: what smj_lidar_to_occupancy
 * does in the world frame with the simulator's own pose, done with the pose an estimator believes in -- smj_scan_to_pose's
 * pose_out_dev goes in as it is, and its status word gates the env.  Match, integrate, distance field, match again then run per env
 * on the device with nothing read back.  num_envs and nlidar are the context's; the entry needs SMJ_SLOT_XPOSE bound (the rays'
 * geometry in the robot's frame is read from it) and the model's lidar tables; nlidar <= 1024.  No workspace, no global atomics.
 *
 * Inputs.
 * lidar_dev, lidar_ld: the scan as smj_lidar_to_occupancy takes it: float32 [nlidar][lidar_ld], range k of env e at k lidar_ld + e.
 * frame: a fused body id >= 0, the robot's frame; SMJ_FRAME_WORLD and SMJ_FRAME_CAMERA are refused.
 * r_min, r_max: finite, 0 <= r_min <= r_max, r_max / cell <= 8192, as that entry refuses them.
 * pose_dev: float32 [3][num_envs], rows x, y, theta: the robot's pose in the map's frame -- the layout of SMJ_SLOT_BASE_POSE and of
 * smj_scan_to_pose's pose_out_dev.
 * gate_dev: int32 or null; the word of env e is gate_dev[e gate_ld], gate_ld >= 1.  AN ENV IS INTEGRATED IFF ITS WORD IS 0: with
 * best_dev + 3 of smj_scan_to_pose and gate_ld = 4 that is its status SMJ_MATCH_OK, with no copy.  Null gates nothing.
 * x0, y0, cell, nx, ny: the grid as smj_lidar_to_occupancy takes it: nx, ny >= 1 and nx ny <= 65536; cell finite and > 0; x0, y0
 * finite: the corner of cell (0, 0); row-major, rows follow y.
 * no_return_clears, accumulate: as smj_lidar_to_occupancy.
 *
 * The rays -- floats, once per ray.  Origin o and direction d of rangefinder k in the body `frame`, as smj_lidar_to_occupancy forms
 * them there.  The range r = lidar[k][e] is classified by that entry's table: dropped, a return of length len = r, or (with
 * no_return_clears) a clearing ray of length len = r_max.  The end in the robot's frame is p = o + len d in fp32.  With
 * c = cosf(theta), s = sinf(theta) (the accurate functions) a point q of the robot's frame lies at
 * (x + c qx - s qy, y + s qx + c qy) =: (gx, gy) and has the float index (floorf((gx - x0) / cell), floorf((gy - y0) / cell)), all
 * in fp32: for q = o that is (fax, fay), for q = p it is (fbx, fby) -- for a return the very operations by which smj_scan_to_pose
 * places the point under a rotation offset of 0, so the end cell of a return is the cell the matcher scored.  Guards, compares of
 * floats made before any conversion: |fax|, |fay| <= 2^20 and |fbx - fax|, |fby - fay| <= 16384.  A ray that fails one -- a NaN
 * anywhere included -- is dropped; a KEPT ray has the cells a = ((int)fax, (int)fay), b = ((int)fbx, (int)fby).
 *
 * The walk -- integers.  A kept ray visits the closed-form Bresenham line of smj_lidar_to_occupancy from a to b, i = 0 .. n with
 * n = max(|bx - ax|, |by - ay|).  A return adds 1 to miss in the cells i < n and 1 to hit in cell i = n; a clearing ray adds 1 to
 * miss in all of them.  Cells outside the grid are skipped: the line is never re-aimed by clipping.
 *
 * Per env the status:
 *   SMJ_MAP_OFF    x, y or theta is not finite (checked before the gate);
 *   SMJ_MAP_GATED  otherwise, the gate word is not 0;
 *   SMJ_MAP_OK     otherwise.
 * An env that is not SMJ_MAP_OK contributes no ray: with accumulate = 1 its slices of hit_dev and miss_dev keep their bits, with
 * accumulate = 0 they are zeroed.
 *
 * Outputs.
 * hit_dev: int32 [num_envs][ny][nx], required; miss_dev: the same shape, or null.  Four-byte alignment suffices (16-byte aligned
 * addresses take wide stores, same values).  accumulate = 0 overwrites them, accumulate = 1 adds to what they hold.
 * info_dev: int32 [num_envs][4], required: the status, the returns kept, the clearing rays kept, and the rays that were classified a
 * return or a clearing ray (so have a finite length) but failed a guard; the last three are 0 unless SMJ_MAP_OK.
 * cell_dev: int32 [num_envs][nlidar][4], or null: (ax, ay, bx, by) of every kept ray; all four words SMJ_MAP_NO_CELL -- a value
 * outside the +-2^21 a cell can take -- for a ray that is not kept and for every ray of an env that is not SMJ_MAP_OK.
 * A null miss_dev or cell_dev is left untouched.  Every output is a unique integer sum or a unique value, so two calls give
 * identical bits whatever the order of evaluation; the inputs are unchanged; nothing outside the outputs is written.
 * Errors: -1 for a null lidar_dev / pose_dev / hit_dev / info_dev, a pointer not aligned to 4 bytes (the gate included),
 * nlidar > 1024, lidar_ld < num_envs, gate_ld < 1, a frame that is no body id or a body id >= nbody, any limit above, an output range
 * that overlaps an input range or another output (the gate's range runs from its first word to that of env num_envs-1; the bound
 * SMJ_SLOT_XPOSE is an input: its range runs from its first word to env num_envs-1 of its last row, as the scan's does); -5 when
 * SMJ_SLOT_XPOSE is not bound; -6 for a model without lidar tables.  A refused call writes nothing. */
int smj_scan_to_map(smj_ctx* ctx, const void* lidar_dev, long lidar_ld, int frame, float r_min, float r_max,
                    const void* pose_dev, const void* gate_dev, long gate_ld,
                    float x0, float y0, float cell, int nx, int ny, int no_return_clears, int accumulate,
                    void* hit_dev, void* miss_dev, void* info_dev, void* cell_dev, void* stream);

#ifdef __cplusplus
}
#endif
#include "smj_localize.h"
#endif
