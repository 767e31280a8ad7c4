/* smj_occupancy.h -- 2-D occupancy grids from the lidar scan (libsmj.so, HIP / gfx950).
 *
 * Part of the C-ABI: smj.h includes this file, so a caller includes smj.h alone.  Like smj_pointcloud.h and smj_heightmap.h it is a
 * header of its own because existing tests fix the declarations of those files; what is declared here is listed in
 * lib.OCCUPANCY_EXPORTS and held to the library by tests/test_occupancy_capi.py.  Same rules as smj.h: caller-owned device
 * pointers, 0 on success, a negative code and smj_last_error otherwise, asynchronous on the caller's stream.
 */
#ifndef SMJ_OCCUPANCY_H
#define SMJ_OCCUPANCY_H
#include "smj.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Ray-traced occupancy counts of one lidar scan in one fused pass: per cell the number of rays that end in it on something (hit)
 * and the number of rays that pass through it (miss).  A cell with neither was not seen.
 * lidar_dev: fp32 [nlidar][lidar_ld], batch-major, exactly what SMJ_SLOT_LIDAR holds after a step with SMJ_READ_LIDAR (metres,
 * -1 = nothing hit); an explicit pointer, so any scan can be fed.  lidar_ld >= num_envs.
 * Ray k of env e: origin o and direction d as the lidar ray cast forms them -- o the pose of the site's body applied to the site's
 * position, d the body's rotation applied to the site's +Z column, used as stored -- expressed in `frame`: SMJ_FRAME_WORLD, or the
 * frame of a fused body F (frame >= 0): o_F = R_F' (o - t_F), d_F = R_F' d.  The grid is the frame's xy plane; z is not used.
 * Range r = lidar[k][e], float compares on the value as stored:
 *     r NaN                       dropped;
 *     0 <= r < r_min              dropped (the ray ends on the robot itself);
 *     r_min <= r <= r_max         a return, end point o + r d;
 *     r < 0 or r > r_max          no return: with no_return_clears the ray is free over r_max (end point o + r_max d, no hit),
 *                                 without it the ray is dropped.
 * Cells, all in fp32 with inv_cell = 1.f / cell: (iy, ix) = (floorf((y - y0) * inv_cell), floorf((x - x0) * inv_cell)), row-major,
 * rows follow y, as smj_depth_to_heightmap.  With a the cell of the origin, b the cell of the end point and
 * n = max(|bx - ax|, |by - ay|), the ray visits the closed-form Bresenham line i = 0 .. n: major coordinate a + i s, minor
 * coordinate a_min + s_min ((2 i d_min + n) / (2 n)) by integer division, x the major axis when |dx| >= |dy|; n = 0 is the cell a
 * alone.  A return adds 1 to miss in the cells i < n and 1 to hit in cell i = n; a clearing ray adds 1 to miss in all of them.
 * Cells outside the grid are skipped: the line is never re-aimed by clipping.  A ray whose origin lies more than 2^20 cells from
 * the grid's corner is dropped.
 * hit_dev, miss_dev: int32 [num_envs][ny][nx]; miss_dev may be null.  Four-byte alignment suffices for all three pointers
 * (16-byte aligned ones take wide accesses, same values).
 * accumulate = 0 overwrites the outputs, accumulate = 1 adds to what they hold.  Both layers are integer sums: the result does not
 * depend on any order, two calls give identical arrays, and scans accumulate in the world frame into a map across steps.
 * Errors: -1 for a null or misaligned lidar_dev / hit_dev, a misaligned miss_dev, lidar_ld < num_envs, nx or ny < 1 or
 * nx * ny > 65536, cell not finite or <= 0, x0 or y0 not finite, r_min or r_max not finite, r_min < 0 or r_min > r_max,
 * r_max / cell > 8192, SMJ_FRAME_CAMERA or a frame below SMJ_FRAME_WORLD, a body id >= nbody; -5 when SMJ_SLOT_XPOSE is unbound
 * (every frame needs the poses); -6 for a model without lidar / ray-casting tables.  A refused call writes nothing.  No workspace
 * is allocated. */
int smj_lidar_to_occupancy(smj_ctx* ctx, const void* lidar_dev, long lidar_ld, int frame,
                           float x0, float y0, float cell, int nx, int ny,
                           float r_min, float r_max, int no_return_clears, int accumulate,
                           void* hit_dev, void* miss_dev, void* stream);

#ifdef __cplusplus
}
#endif
#include "smj_distance.h"
#endif
