/* smj_heightmap.h -- egocentric height maps from the depth images (libsmj.so, HIP / gfx950).
 *
 * Part of the C-ABI: smj.h includes this file, so a caller includes smj.h alone.  Like smj_pointcloud.h it is a header of its own
 * because existing tests fix the declarations of smj.h and smj_pointcloud.h; what is declared here is listed in
 * lib.HEIGHTMAP_EXPORTS and held to the library by tests/test_height_map_capi.py.  Same rules as smj.h: caller-owned device
 * pointers, 0 on success, a negative code and smj_last_error otherwise, asynchronous on the caller's stream.
 */
#ifndef SMJ_HEIGHTMAP_H
#define SMJ_HEIGHTMAP_H
#include "smj.h"
#ifdef __cplusplus
extern "C" {
#endif

/* 2.5-D grid of a depth image in one fused pass: per cell the highest point and the number of points in a height band.
 * camera_id, width, height, fovy_deg, depth_dev, stride and frame mean what they mean for smj_depth_to_points
 * (smj_pointcloud.h): the kept pixels are (u, v) = (s j, s i), the point (x, y, z) of a pixel is the one that entry writes, in
 * SMJ_FRAME_CAMERA, SMJ_FRAME_WORLD or the frame of a fused body (frame >= 0).
 * Binning, all in fp32 with inv_cell = 1.f / cell:
 *     fx = floorf((x - x0) * inv_cell),  fy = floorf((y - y0) * inv_cell);
 *     the point is kept iff 0 <= fx < nx, 0 <= fy < ny and z_lo <= z <= z_hi  (float compares: NaN and infinities drop out);
 *     its cell is (iy, ix) = ((int)fy, (int)fx), row-major, rows follow y.
 * Invalid depths (not finite or <= 0, the NaN points of the cloud) drop out.  The map holds whatever the camera sees, the robot's
 * own arm included: there are no per-pixel labels and no self-filter.
 * zmax_dev: fp32 [num_envs][ny][nx], the largest z of the cell's kept points, a quiet NaN for a cell with none.
 * count_dev: int32 [num_envs][ny][nx], the number of kept points of the cell; may be null.
 * Four-byte alignment suffices for all three pointers (16-byte aligned ones take wide accesses, same values).
 * accumulate = 0 overwrites the outputs.  accumulate = 1 starts from what they hold: NaN in zmax_dev means empty, otherwise the
 * new value is the max of old and new; counts add.  Both reductions are independent of order, so two cameras (or several stride
 * phases) fuse into one map by a second call, and the result does not depend on which comes first.
 * z_lo = -INFINITY / z_hi = INFINITY leave the band open.
 * Errors: -1 for a bad camera id, width / height / stride < 1, nx or ny < 1 or nx * ny > 65536, cell not finite or <= 0, x0 or y0
 * not finite, z_lo or z_hi NaN or z_lo > z_hi, a null or misaligned depth_dev / zmax_dev, a misaligned count_dev, a body id >= nbody
 * or a frame below SMJ_FRAME_WORLD; -5 when frame != SMJ_FRAME_CAMERA and SMJ_SLOT_XPOSE is unbound; -6 for a model without camera
 * tables.  A refused call writes nothing.  No workspace is allocated. */
int smj_depth_to_heightmap(smj_ctx* ctx, int camera_id, int width, int height, float fovy_deg, const void* depth_dev,
                           int stride, int frame,
                           float x0, float y0, float cell, int nx, int ny, float z_lo, float z_hi,
                           int accumulate, void* zmax_dev, void* count_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
