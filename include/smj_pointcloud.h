/* smj_pointcloud.h -- organised point clouds from the depth images (libsmj.so, HIP / gfx950).
 *
 * Part of the C-ABI: smj.h includes this file, so a caller includes smj.h alone.  The entry has a header of its own because the
 * set of entries that smj.h declares is fixed at fifteen (tests/test_contact_readout.py pins the count, tests/test_capi.py ties
 * lib.EXPORTS to it); what is declared here is listed in lib.POINT_EXPORTS and held to the library by
 * tests/test_point_cloud_capi.py in the same way.  Same rules as smj.h: caller-owned device pointers, 0 on success, a negative
 * code and smj_last_error otherwise, asynchronous on the caller's stream.
 */
#ifndef SMJ_POINTCLOUD_H
#define SMJ_POINTCLOUD_H
#include "smj.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Organised point cloud of a depth image, one fused pass (no reference counterpart: users of the reference deproject
 * pull_camera_data() themselves).  depth_dev: fp32 [num_envs][height][width] as smj_render_depth writes it for the same camera,
 * size and fovy_deg -- metres along the optical axis of a MuJoCo camera (x right, y up, looking down -z).  For image pixel (u, v),
 * with the ray caster's pixel-centre rule, th = tan(fovy / 2):
 *     xn = ((u + 0.5) / width * 2 - 1) * th * width / height,      yn = (1 - (v + 0.5) / height * 2) * th,
 * the point of depth d is d (xn, yn, -1) in the MuJoCo camera frame, carried into `frame`:
 *   SMJ_FRAME_CAMERA  the optical frame (x right, y down, z forward, as OpenCV and ROS use it): d (xn, -yn, 1); no state is read;
 *   SMJ_FRAME_WORLD   the camera's world pose, composed as smj_render_depth does it from SMJ_SLOT_XPOSE of the camera's body and
 *                     the model's camera offset;
 *   frame >= 0        the frame of that fused body (an XPOSE entry): R_b' (world point - x_b).
 * Validity: a depth that is not finite or is <= 0 (what max_depth zeroed) gives three quiet NaNs, the convention of organised
 * clouds; the far plane of a raw render (max_depth <= 0) is deprojected like any other value.
 * Stride: stride = s >= 1 keeps the pixels (u, v) = (s j, s i); points_dev is fp32 [num_envs][ceil(height / s)][ceil(width / s)][3],
 * xyz interleaved, grid row i / column j.  Both pointers need only 4-byte alignment (16-byte aligned ones take the wide path, same values).
 * Intrinsics: the matrix that fits these images is compute_K(fovy, width, height) with pixel index u at u + 0.5 (utils.render_K) --
 * NOT the reference's cam_*_K fields, which get_camera_params builds from the sensor resolution (1280 x 720, 1920 x 1080) while
 * the images are 480 x 270 and 424 x 240.
 * Asynchronous on `stream`; the per-env transforms live in a context-owned workspace allocated at the first call.
 * Errors: -5 when frame != SMJ_FRAME_CAMERA and SMJ_SLOT_XPOSE is unbound; -1 for a bad camera id, width / height / stride < 1, a
 * null or misaligned pointer, a body id >= nbody or a frame below SMJ_FRAME_WORLD; -6 for a model without camera tables. */
enum { SMJ_FRAME_CAMERA = -1, SMJ_FRAME_WORLD = -2 };   /* frame >= 0: the frame of that fused body (an XPOSE entry) */
int smj_depth_to_points(smj_ctx* ctx, int camera_id, int width, int height, float fovy_deg, const void* depth_dev,
                        int stride, int frame, void* points_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
