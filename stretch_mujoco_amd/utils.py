"""Pure helper functions of the glue layer, batched (work on floats, numpy arrays and torch tensors alike).

Mirrors stretch_mujoco/utils.py: diff_drive_fwd_kinematics (:94-114), diff_drive_inv_kinematics (:117-135),
map_between_ranges (:352-360), compute_K (:56-61), limit_depth_distance (:87-91).
"""
from __future__ import annotations

import math
from typing import Any, NamedTuple

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


class BaseCandidates(NamedTuple):
    """The candidate table of pull_base_command() / smj_navigation_to_velocity, shared by all envs: fp32 tensors on one device."""
    command: Any        # [K, 2]: the (v, w) a candidate stands for
    points: Any         # [K, P, 2]: points in the robot's frame (x forward, y left); the first P - 1 are swept, the last one scores
    bias: Any           # [K] int32 or None: added to the candidate's score


class ScanAngles(NamedTuple):
    """The rotation table of pull_scan_match() / smj_scan_to_pose, shared by all envs: tensors on one device."""
    angles: Any         # [T] fp32: offsets added to the prior's theta [rad]
    bias: Any           # [T] int32: taken from the score of every candidate with that rotation


def scan_angles(window: float = 0.1745, step: float = 0.008727, weight: int = 0, device=None) -> ScanAngles:
    """Rotation offsets for pull_scan_match(): k step for k = 0, -1, +1, -2, +2, .. out to n = round(window / (2 step)) steps on
    either side, so `window` is the whole width searched [rad] and T = 2 n + 1 (the defaults: 10 degrees in steps of half a degree,
    T = 21).  In this order the entry's tie-break -- the smallest index among equal scores -- prefers the smaller rotation.
    bias = weight |k|: what a rotation of k steps costs, in units of the field (255 per scan point on an obstacle).
    Limits of the entry: T <= 64, bias <= 2^20 (ValueError)."""
    import torch

    window, step, weight = float(window), float(step), int(weight)
    if not (np.isfinite(window) and window >= 0 and np.isfinite(step) and step > 0):
        raise ValueError("window >= 0 and step > 0, both finite [rad]")
    n = int(round(window / (2.0 * step)))
    if 2 * n + 1 > 64:
        raise ValueError(f"{2 * n + 1} rotations: T <= 64 (a wider step, or a narrower window)")
    if weight < 0 or weight * n > 1 << 20:
        raise ValueError("weight >= 0 and weight * n <= 2^20")
    k = np.array([0] + [s * j for j in range(1, n + 1) for s in (-1, 1)], np.int64)
    return ScanAngles(angles=torch.tensor(k * step, dtype=torch.float32, device=device),
                      bias=torch.tensor(weight * np.abs(k), dtype=torch.int32, device=device))


def spread_particles(center, half_extent, num_particles: int, generator=None):
    """A first particle set for pull_particle_update(): fp32 [3, B, P], uniform in the box center +- half_extent in (x, y, theta).
    center: a float tensor [3, B] (its device is the result's); half_extent = (metres in x, metres in y, radians), each finite and
    >= 0; P = num_particles in [1, 4096].  generator: a torch.Generator on that device, None for the global one."""
    import torch

    if not isinstance(center, torch.Tensor) or not center.is_floating_point() or center.dim() != 2 or center.shape[0] != 3:
        raise ValueError("center: a float tensor [3, num_envs]")
    try:
        half = [float(v) for v in half_extent]
    except (TypeError, ValueError):
        raise ValueError("half_extent = (metres in x, metres in y, radians)") from None
    if len(half) != 3 or not all(np.isfinite(v) and v >= 0 for v in half):
        raise ValueError("half_extent: three finite numbers >= 0")
    P = int(num_particles)
    if not 1 <= P <= 4096:
        raise ValueError("num_particles must be in [1, 4096]")
    u = torch.rand(3, center.shape[1], P, dtype=torch.float32, device=center.device, generator=generator) * 2.0 - 1.0
    return center.to(torch.float32).unsqueeze(2) + u * torch.tensor(half, dtype=torch.float32, device=center.device).reshape(3, 1, 1)


def particle_noise(sigma_xy: float, sigma_theta: float, shape, generator=None, device=None):
    """The noise of pull_particle_update(noise=...) and StatusStretchParticles.predict(noise=...): fp32 of `shape` = (3, B, P), normal
    with standard deviation sigma_xy [m] in rows x and y and sigma_theta [rad] in row theta.  On the generator's device, or `device`."""
    import torch

    sigma_xy, sigma_theta = float(sigma_xy), float(sigma_theta)
    if not (np.isfinite(sigma_xy) and sigma_xy >= 0 and np.isfinite(sigma_theta) and sigma_theta >= 0):
        raise ValueError("sigma_xy and sigma_theta: finite and >= 0")
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or shape[0] != 3:
        raise ValueError("shape = (3, num_envs, num_particles)")
    if device is None and generator is not None:
        device = generator.device
    n = torch.randn(shape, dtype=torch.float32, device=device, generator=generator)
    return n * torch.tensor([sigma_xy, sigma_xy, sigma_theta], dtype=torch.float32, device=n.device).reshape(3, 1, 1)


def unicycle_pose(v, w, t):
    """Pose (x, y, theta) of a unicycle that starts at the origin facing +x and drives (v, w) for t seconds, fp64, arrays alike:
    (v/w sin(wt), v/w (1 - cos(wt)), wt), written as v t sinc(a) and v t (a/2) sinc(a/2)^2 with a = wt and sinc(a) = sin(a) / a,
    which is the same closed form for every w and the straight line at w = 0: nothing blows up near it."""
    v, w, t = (np.asarray(q, np.float64) for q in (v, w, t))
    a = w * t
    sinc = lambda z: np.sinc(z / np.pi)      # numpy's sinc is sin(pi z) / (pi z)
    return v * t * sinc(a), v * t * 0.5 * a * sinc(0.5 * a) ** 2, a


def arc_candidates(v=None, w=None, horizon: float = 1.5, samples: int = 12, lookahead: float = 0.3, footprint=None, bias=None, turn_bias: int = 0, device=None) -> BaseCandidates:
    """Candidate arcs for pull_base_command(): for each pair (v[k], w[k]) the poses of the unicycle at t = horizon (i + 1) / samples,
    i = 0 .. samples - 1, built in fp64 on the host (unicycle_pose) and stored as fp32 tensors on `device`.
    footprint None: one swept point per sample, the pose's position -- the costmap's inflation stands for the body, as in
    pull_navigation_field.  footprint [(x, y), ..] in the robot's frame: those points at every sample pose, sample after sample.
    The scoring point lies `lookahead` metres ahead of the final pose along its heading.  So P = samples * F + 1.
    v, w None: the default set, v in (0.25, 0.16, 0.08, 0) m/s by nine w evenly in [-1, 1] rad/s, without (0, 0): 35 candidates,
    the fastest first, so that among equal scores the faster one wins.  bias: None or K integers; turn_bias is added to the bias of
    the candidates with v = 0 (turning in place): with a scoring point ahead of the arc's end a robot that faces a goal closer than
    that point would otherwise rather turn than drive the last stretch.
    Limits of the entry: K <= 1024, P <= 256, K P <= 32768 (ValueError)."""
    import torch

    if (v is None) != (w is None):
        raise ValueError("v and w: both None (the default set) or two sequences of equal length")
    if v is None:
        vs, ws = np.meshgrid(np.array([0.25, 0.16, 0.08, 0.0]), np.linspace(-1.0, 1.0, 9), indexing="ij")
        keep = (vs != 0) | (ws != 0)
        v, w = vs[keep], ws[keep]
    v, w = np.atleast_1d(np.asarray(v, np.float64)), np.atleast_1d(np.asarray(w, np.float64))
    samples = int(samples)
    horizon, lookahead = float(horizon), float(lookahead)
    if v.ndim != 1 or v.shape != w.shape or v.size < 1 or not (np.isfinite(v).all() and np.isfinite(w).all()):
        raise ValueError("v and w: two finite sequences of equal length >= 1")
    if samples < 1 or not (np.isfinite(horizon) and horizon > 0) or not np.isfinite(lookahead):
        raise ValueError("samples >= 1, horizon > 0 and finite, lookahead finite")
    if footprint is None:
        fp = np.zeros((1, 2))
    else:
        fp = np.asarray(footprint, np.float64)
        if fp.ndim != 2 or fp.shape[1] != 2 or fp.shape[0] < 1 or not np.isfinite(fp).all():
            raise ValueError("footprint: None or [(x, y), ..] in the robot's frame, finite")
    K, P = v.size, samples * fp.shape[0] + 1
    if K > 1024 or P > 256 or K * P > 32768:
        raise ValueError(f"{K} candidates of {P} points: K <= 1024, P <= 256 and K P <= 32768")
    t = horizon * (np.arange(samples) + 1.0) / samples
    x, y, th = unicycle_pose(v[:, None], w[:, None], t[None, :])                      # [K, samples]
    c, s = np.cos(th)[..., None], np.sin(th)[..., None]
    sx = x[..., None] + c * fp[:, 0] - s * fp[:, 1]                                     # [K, samples, F]
    sy = y[..., None] + s * fp[:, 0] + c * fp[:, 1]
    swept = np.stack((sx, sy), -1).reshape(K, P - 1, 2)
    score = np.stack((x[:, -1] + lookahead * np.cos(th[:, -1]), y[:, -1] + lookahead * np.sin(th[:, -1])), -1)
    points = np.concatenate((swept, score[:, None, :]), 1)
    turn_bias = int(turn_bias)
    if bias is not None or turn_bias:
        b = np.zeros(K, np.int64) if bias is None else np.asarray(bias)
        if b.shape != (K,) or not np.issubdtype(b.dtype, np.integer):
            raise ValueError(f"bias: None or {K} int32 values")
        b = b.astype(np.int64) + turn_bias * (v == 0)
        if np.abs(b).max(initial=0) >= 1 << 31:
            raise ValueError(f"bias: None or {K} int32 values")
        bias = torch.tensor(b.astype(np.int32), dtype=torch.int32, device=device)
    return BaseCandidates(command=torch.tensor(np.stack((v, w), 1), dtype=torch.float32, device=device),
                          points=torch.tensor(points, dtype=torch.float32, device=device), bias=bias)
