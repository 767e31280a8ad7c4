"""fp64 numpy restatement of smj_depth_to_points (include/smj_pointcloud.h): the reference the point-cloud tests compare against.  A helper,
not a test.  depth is metres along the optical axis of a MuJoCo camera (x right, y up, looking down -z), row 0 at the top."""
import math

import numpy as np


def pixel_dirs(W, H, fovy, stride=1):
    """(xn, yn) of the kept pixels (u, v) = (s j, s i), each [H', W']: the ray caster's pixel-centre rule."""
    th = math.tan(float(fovy) * math.pi / 360)
    u, v = np.meshgrid(np.arange(0, W, stride, dtype=np.float64), np.arange(0, H, stride, dtype=np.float64))
    return ((u + 0.5) / W * 2 - 1) * th * W / H, (1 - (v + 0.5) / H * 2) * th


def deproject(depth, W, H, fovy, stride, cam_xpos, cam_xmat, frame, body_xpos=None, body_xmat=None):
    """depth [H, W] or [B, H, W] -> points [H', W', 3] or [B, H', W', 3] (fp64) in `frame`: "camera" (optical: x right, y down, z
    forward; the poses are not used), "world" (cam_xpos [.., 3], cam_xmat [.., 3, 3]: the camera's world pose) or "body"
    (body_xpos / body_xmat: R_b' (world point - x_b)).  Depths that are not finite or are <= 0 give NaN rows."""
    depth = np.asarray(depth, np.float64)
    single = depth.ndim == 2
    d = depth.reshape(-1, H, W)[:, ::stride, ::stride]
    xn, yn = pixel_dirs(W, H, fovy, stride)
    valid = np.isfinite(d) & (d > 0)
    dv = np.where(valid, d, 0.0)
    pc = np.stack([dv * xn, dv * yn, -dv], -1)                       # MuJoCo camera frame, [B, H', W', 3]
    if frame == "camera":
        pts = pc * np.array([1.0, -1.0, -1.0])
    else:
        cp = np.asarray(cam_xpos, np.float64).reshape(-1, 3)
        cm = np.asarray(cam_xmat, np.float64).reshape(-1, 3, 3)
        pts = np.einsum("bij,bhwj->bhwi", cm, pc) + cp[:, None, None, :]
        if frame == "body":
            bp = np.asarray(body_xpos, np.float64).reshape(-1, 3)
            bm = np.asarray(body_xmat, np.float64).reshape(-1, 3, 3)
            pts = np.einsum("bji,bhwj->bhwi", bm, pts - bp[:, None, None, :])
        elif frame != "world":
            raise ValueError(frame)
    pts = np.where(valid[..., None], pts, np.nan)
    return pts[0] if single else pts


def camera_pose(xpose, cam_bodyid, cam_pos, cam_mat, cam):
    """World pose of camera `cam` per env from the batch-major body poses xpose [nbody*12, B] (xpos 3 + xmat 9) and the model's
    camera offsets: (cam_xpos [B, 3], cam_xmat [B, 3, 3], body_xpos [B, 3]), fp64."""
    xpose = np.asarray(xpose, np.float64)
    b = int(np.asarray(cam_bodyid).reshape(-1)[cam])
    bp, bm = body_pose(xpose, b)
    lp = np.asarray(cam_pos, np.float64).reshape(-1, 3)[cam]
    lm = np.asarray(cam_mat, np.float64).reshape(-1, 3, 3)[cam]
    return bp + bm @ lp, bm @ lm, bp


def body_pose(xpose, b):
    xpose = np.asarray(xpose, np.float64)
    return xpose[12 * b: 12 * b + 3].T.copy(), xpose[12 * b + 3: 12 * b + 12].T.reshape(-1, 3, 3).copy()
