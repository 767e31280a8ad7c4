"""Pure helper functions of the glue layer, batched (work on floats, numpy arrays and torch tensors alike).

Mirrors stretch_mujoco/utils.py: diff_drive_fwd_kinematics (:94-114), diff_drive_inv_kinematics (:117-135),
map_between_ranges (:352-360), compute_K (:56-61), limit_depth_distance (:87-91).
"""
from __future__ import annotations

import math

import numpy as np

from . import config


def diff_drive_fwd_kinematics(w_left, w_right):
    R = config.robot_settings["wheel_diameter"] / 2
    L = config.robot_settings["wheel_separation"]
    if R <= 0:
        raise ValueError("Radius must be greater than zero.")
    if L <= 0:
        raise ValueError("Distance between wheels must be greater than zero.")
    V = R * (w_left + w_right) / 2.0
    omega = R * (w_right - w_left) / L
    return (V, omega)


def diff_drive_inv_kinematics(V, omega):
    R = config.robot_settings["wheel_diameter"] / 2
    L = config.robot_settings["wheel_separation"]
    if R <= 0:
        raise ValueError("Radius must be greater than zero.")
    if L <= 0:
        raise ValueError("Distance between wheels must be greater than zero.")
    w_left = (V - (omega * L / 2)) / R
    w_right = (V + (omega * L / 2)) / R
    return (w_left, w_right)


def map_between_ranges(value, from_min_max, to_min_max):
    return (value - from_min_max[0]) * (to_min_max[1] - to_min_max[0]) / (from_min_max[1] - from_min_max[0]) + to_min_max[0]


def compute_K(fovy: float, width: int, height: int) -> np.ndarray:
    f = 0.5 * height / math.tan(fovy * math.pi / 360)
    return np.array(((f, 0, width / 2), (0, f, height / 2), (0, 0, 1)))


def render_K(fovy: float, width: int, height: int, stride: int = 1) -> np.ndarray:
    """The intrinsic matrix that fits an image rendered at `width` x `height` with vertical field of view `fovy` (degrees), and the
    point clouds made from it (StretchBatchSimulator.pull_point_cloud): compute_K(fovy, width, height) read under the renderer's
    pixel-centre convention -- pixel index u sits at image coordinate u + 0.5, so a point (x, y, z) of the optical frame (x right,
    y down, z forward) lies in pixel (u, v) with K @ (x, y, z) / z = (u + 0.5, v + 0.5, 1).  (The cam_*_K fields of
    pull_camera_data follow the reference instead: the sensor resolution, which is not the image's.)

    stride = s > 1 gives the matrix of the subsampled grid of a point cloud: grid cell (i, j) -- row i, column j -- is image pixel
    (u, v) = (s j, s i), the grid has ceil(height / s) rows and ceil(width / s) columns, and the returned matrix sends the cell's
    point to (j + 0.5, i + 0.5, 1): focal length f / s, principal point ((c - 0.5) / s + 0.5).  With stride = 1 and a strided
    cloud, the projection is the image coordinate (s j + 0.5, s i + 0.5) of the pixel the cell was taken from."""
    if stride < 1:
        raise ValueError("stride must be >= 1")
    K = compute_K(fovy, width, height)
    if stride > 1:
        K[0, 0] /= stride; K[1, 1] /= stride
        K[0, 2] = (K[0, 2] - 0.5) / stride + 0.5
        K[1, 2] = (K[1, 2] - 0.5) / stride + 0.5
    return K


def limit_depth_distance(depth_image_meters, max_depth: float):
    """Values strictly greater than max_depth become 0 (works for numpy arrays and torch tensors)."""
    try:
        import torch

        if isinstance(depth_image_meters, torch.Tensor):
            return torch.where(depth_image_meters > max_depth, torch.zeros_like(depth_image_meters), depth_image_meters)
    except ImportError:  # pragma: no cover
        pass
    return np.where(depth_image_meters > max_depth, 0, depth_image_meters)


def to_real_gripper_range(pos):
    """stretch_mujoco/mujoco_server.py:517-525"""
    return map_between_ranges(pos, config.robot_settings["sim_gripper_min_max"], config.robot_settings["gripper_min_max"])


def to_sim_gripper_range(pos):
    """stretch_mujoco/mujoco_server.py:580-588"""
    return map_between_ranges(pos, config.robot_settings["gripper_min_max"], config.robot_settings["sim_gripper_min_max"])
