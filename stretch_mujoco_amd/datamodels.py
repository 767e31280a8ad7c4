"""Batched counterparts of the reference dataclasses (stretch_mujoco/datamodels/*.py).

Field names and units are the reference's; every scalar becomes a tensor with a leading batch dimension [B].
Tensors returned by `pull_*` are fresh copies (the reference returns fresh pickled copies as well).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional


@dataclass
class PositionVelocity:  # status_stretch_joints.py:5-12
    pos: Any
    vel: Any


@dataclass
class BaseStatus:  # status_stretch_joints.py:14-24
    x: Any
    y: Any
    theta: Any
    x_vel: Any
    theta_vel: Any


@dataclass
class StatusStretchJoints:  # status_stretch_joints.py:26-74
    time: Any
    fps: float
    sim_to_real_time_ratio_msg: str
    base: BaseStatus
    lift: PositionVelocity
    arm: PositionVelocity
    head_pan: PositionVelocity
    head_tilt: PositionVelocity
    wrist_yaw: PositionVelocity
    wrist_pitch: PositionVelocity
    wrist_roll: PositionVelocity
    gripper: PositionVelocity

    def __getitem__(self, name: str):
        """Backward compatibility: square-bracket access (status_stretch_joints.py:41-43)."""
        return getattr(self, name)


@dataclass
class StatusStretchSensors:  # status_stretch_sensors.py:10-77
    time: Any
    fps: float
    base_gyro: Optional[Any] = None
    base_imu: Optional[Any] = None  # the accelerometer lives in the field named base_imu (status_stretch_sensors.py:53-55)
    lidar: Optional[Any] = None

    def get_data(self, sensor):
        from .enums import StretchSensors

        data = {StretchSensors.base_gyro: self.base_gyro, StretchSensors.base_accel: self.base_imu,
                StretchSensors.base_lidar: self.lidar}[sensor]
        if data is None:
            raise ValueError(f"Tried to get {sensor} data, but it is empty.")
        return data


@dataclass
class StatusStretchCameras:  # status_stretch_camera.py:10-125 (depth only on this path)
    """Batched: every image is a torch tensor [B, H, W] (fp32 metres), K is the 3x3 intrinsic matrix shared by all envs.
    The depth tensors are views of simulator-owned buffers that the next pull_camera_data() overwrites: .clone() to keep."""
    time: Any
    fps: float
    cam_d405_rgb: Optional[Any] = None
    cam_d405_depth: Optional[Any] = None
    cam_d405_K: Optional[Any] = None
    cam_d435i_rgb: Optional[Any] = None
    cam_d435i_depth: Optional[Any] = None
    cam_d435i_K: Optional[Any] = None
    cam_nav_rgb: Optional[Any] = None

    def get_camera_data(self, camera, *, auto_rotate: bool = True, auto_correct_rgb: bool = True, **_ignored):
        """status_stretch_camera.py:48-86: the d435i frames come out of the (physically rotated) optical frame and are
        turned upright with rot90(-1) when auto_rotate is set, the nav camera's with rot90(+1); colour images [..., H, W, 3]
        come back in BGR channel order when auto_correct_rgb is set (the reference's cv2.COLOR_RGB2BGR); ValueError when the
        image is empty."""
        from .enums import StretchCameras
        import torch

        data = None
        turn = 0
        if camera == StretchCameras.cam_d405_depth and self.cam_d405_depth is not None:
            data = self.cam_d405_depth
        elif camera == StretchCameras.cam_d435i_depth and self.cam_d435i_depth is not None:
            data = self.cam_d435i_depth
            data = torch.rot90(data, -1, dims=(-2, -1)) if auto_rotate else data
        elif camera in (StretchCameras.cam_d405_rgb, StretchCameras.cam_d435i_rgb, StretchCameras.cam_nav_rgb) and getattr(self, camera.name) is not None:
            data = getattr(self, camera.name)
            turn = {StretchCameras.cam_d405_rgb: 0, StretchCameras.cam_d435i_rgb: -1, StretchCameras.cam_nav_rgb: 1}[camera]
            if auto_rotate and turn:
                data = torch.rot90(data, turn, dims=(-3, -2))
            if auto_correct_rgb:
                data = data.flip(-1)
        if data is None:
            raise ValueError(f"Tried to get {camera} data, but it is empty or not implemented.")
        return data

    def get_all(self, *, auto_rotate: bool = True, **kw) -> dict:
        from .enums import StretchCameras

        data = {}
        for camera in StretchCameras.all():
            try:
                data[camera] = self.get_camera_data(camera, auto_rotate=auto_rotate, **kw)
            except ValueError:
                ...
        return data

    def set_camera_data(self, camera, data):
        from .enums import StretchCameras

        if camera not in list(StretchCameras):
            raise NotImplementedError(f"Camera {camera} is not implemented.")
        setattr(self, camera.name, data)

    @staticmethod
    def default():
        return StatusStretchCameras(time=0, fps=0)


@dataclass
class StatusStretchHeightMap:
    """New, without a reference counterpart: the egocentric 2.5-D grid of pull_height_map() (smj_depth_to_heightmap).  Cell
    (iy, ix) covers [origin[0] + ix cell, origin[0] + (ix + 1) cell) x [origin[1] + iy cell, origin[1] + (iy + 1) cell) of `frame`;
    rows follow y.  Device tensors, simulator-owned, not synchronised to the host.  The map holds whatever the cameras see,
    the robot's own arm included."""
    time: Any
    height: Any         # [B, ny, nx] float32: largest z of the cell's points inside z_range, NaN for a cell with none
    count: Any          # [B, ny, nx] int32: number of those points
    origin: Any         # (x0, y0): the corner of cell (0, 0)
    cell: float
    frame: str          # "base", "world" or "camera"


@dataclass
class StatusStretchOccupancyGrid:
    """New, without a reference counterpart: the ray-traced 2-D grid of pull_occupancy_grid() (smj_lidar_to_occupancy).  Cell
    (iy, ix) covers [origin[0] + ix cell, origin[0] + (ix + 1) cell) x [origin[1] + iy cell, origin[1] + (iy + 1) cell) of the xy
    plane of `frame`; rows follow y.  Device tensors, simulator-owned, not synchronised to the host.  A cell with neither a hit
    nor a miss was not seen."""
    time: Any
    hit: Any            # [B, ny, nx] int32: rays that ended in the cell on something
    miss: Any           # [B, ny, nx] int32: rays that passed through the cell (or ended in it on nothing)
    origin: Any         # (x0, y0): the corner of cell (0, 0)
    cell: float
    frame: str          # "base" or "world"

    def occupancy(self, min_hits: int = 1):
        """int8 [B, ny, nx] by the ROS convention (nav_msgs/OccupancyGrid): 100 where hit >= min_hits, else 0 where miss > 0,
        else -1 (unknown)."""
        import torch

        out = torch.where(self.miss > 0, 0, -1).to(torch.int8)
        return torch.where(self.hit >= int(min_hits), torch.tensor(100, dtype=torch.int8, device=out.device), out)

    def log_odds(self, l_hit: float = 0.85, l_miss: float = -0.4):
        """fp32 [B, ny, nx]: l_hit hit + l_miss miss, the log odds of "occupied" under an inverse sensor model that adds l_hit
        per ray ending in the cell and l_miss per ray passing through; 0 where the cell was not seen."""
        import torch

        return float(l_hit) * self.hit.to(torch.float32) + float(l_miss) * self.miss.to(torch.float32)


@dataclass
class StatusStretchDistanceField:
    """New, without a reference counterpart: the exact distance field of pull_distance_field() (smj_occupancy_to_distance) over a
    grid laid out as StatusStretchOccupancyGrid's.  `dist2` and `nearest` are exact integers in cells; the helpers turn them into
    metres and costs in torch.  Device tensors, simulator-owned, not synchronised to the host."""
    time: Any
    dist2: Any          # [B, ny, nx] int32: squared distance in cells to the nearest obstacle cell, 0 on one, NONE where there is none in reach
    nearest: Any        # [B, ny, nx] int32 or None: linear index iy nx + ix of that obstacle (the smallest among equally near ones), -1 where none
    origin: Any         # (x0, y0): the corner of cell (0, 0)
    cell: float
    frame: str          # "base" or "world" ("grid" for a bare mask)

    NONE = 1 << 30      # SMJ_DIST_NONE

    def distance(self):
        """fp32 [B, ny, nx]: sqrt(dist2) cell in metres, inf where there is no obstacle in reach."""
        import torch

        return _inf_where_none(torch.sqrt(self.dist2.to(torch.float32)) * float(self.cell), self.dist2, self.NONE)

    def nearest_offset(self):
        """int32 [B, ny, nx, 2]: (dy, dx) in cells from each cell to its nearest obstacle, zeros where there is none.  Needs
        pull_distance_field(nearest=True)."""
        if self.nearest is None:
            raise ValueError("nearest_offset() needs pull_distance_field(nearest=True)")
        return offsets_of_cells(self.nearest)

    def inflated_cost(self, inscribed_radius: float, inflation_radius: float, cost_scaling_factor: float = 10.0):
        """uint8 [B, ny, nx] by the costmap convention (costmap_2d's inflation layer): 254 on an obstacle, 253 within
        inscribed_radius of one, floor(252 exp(-cost_scaling_factor (d - inscribed_radius))) out to inflation_radius, 0 beyond;
        radii and d in metres."""
        import torch

        r_ins, r_inf, k = float(inscribed_radius), float(inflation_radius), float(cost_scaling_factor)
        if not (0 <= r_ins <= r_inf < float("inf")) or not k >= 0:
            raise ValueError("inflated_cost: 0 <= inscribed_radius <= inflation_radius, both finite; cost_scaling_factor >= 0")
        d = self.distance()
        cost = torch.floor(252.0 * torch.exp(-k * (d - r_ins)))
        cost = torch.where(d <= r_ins, torch.full_like(cost, 253.0), cost)
        cost = torch.where(self.dist2 == 0, torch.full_like(cost, 254.0), cost)
        cost = torch.where(d > r_inf, torch.zeros_like(cost), cost)
        return cost.to(torch.uint8)

    def likelihood(self, sigma: float = 0.10):
        """uint8 [B, ny, nx]: the likelihood field of pull_scan_match() -- what a scan point that lands in the cell is worth,
        floor(255 exp(-d^2 / (2 sigma^2)) + 0.5) with d = sqrt(dist2) cell in metres (evaluated in fp64), 255 on an obstacle, 0 where
        there is no obstacle in reach; sigma in metres."""
        import torch

        sigma = float(sigma)
        if not (0 < sigma < float("inf")):
            raise ValueError("likelihood: sigma in metres, finite and > 0")
        k = float(self.cell) ** 2 / (2.0 * sigma * sigma)
        field = torch.floor(255.0 * torch.exp(-k * self.dist2.to(torch.float64)) + 0.5)
        return torch.where(self.dist2 >= self.NONE, torch.zeros_like(field), field).to(torch.uint8)


def offsets_of_cells(index):
    """int32 [B, ny, nx, 2]: (dy, dx) in cells from each cell (iy, ix) of a grid [B, ny, nx] to the cell its entry names as a linear
    index iy nx + ix; zeros where the entry is negative (none).  On the index's device, no host synchronisation."""
    import torch

    ny, nx = index.shape[-2:]
    iy = torch.arange(ny, dtype=torch.int32, device=index.device).view(1, ny, 1)
    ix = torch.arange(nx, dtype=torch.int32, device=index.device).view(1, 1, nx)
    n = index.clamp(min=0)
    off = torch.stack((torch.div(n, nx, rounding_mode="floor") - iy, n % nx - ix), -1)
    return torch.where((index >= 0).unsqueeze(-1), off, 0).to(torch.int32)


def _inf_where_none(metres, raw, none):
    """`metres` (fp32) with inf where the integer field `raw` holds its NONE or more: no obstacle in reach, no path."""
    return metres.masked_fill(raw >= none, float("inf"))


def cells_of_points(points, origin, cell, ny, nx):
    """int32 linear cell indices iy nx + ix of points [..., 2] (metres, x then y) in a grid laid out as StatusStretchOccupancyGrid's:
    floor((p - origin) / cell); -1 for a point outside the grid or not finite.  On the points' device, no host synchronisation."""
    import torch

    p = points.to(torch.float32)
    o = torch.tensor([float(origin[0]), float(origin[1])], dtype=torch.float32, device=p.device)
    ij = torch.floor((p - o) / float(cell))
    inside = torch.isfinite(ij).all(-1) & (ij[..., 0] >= 0) & (ij[..., 0] < nx) & (ij[..., 1] >= 0) & (ij[..., 1] < ny)
    ij = torch.where(inside.unsqueeze(-1), ij, torch.zeros_like(ij)).to(torch.int32)
    return torch.where(inside, ij[..., 1] * nx + ij[..., 0], torch.full_like(ij[..., 0], -1))


@dataclass
class StatusStretchFrontiers:
    """New, without a reference counterpart: the frontier regions of pull_frontiers() (smj_occupancy_to_frontiers) over a grid laid
    out as StatusStretchOccupancyGrid's -- the free cells that border unseen space, grouped into 8-connected regions, the largest
    first.  Exact integers; the helpers turn them into metres and masks in torch.  `goal` is what pull_navigation_field takes as
    its goal.  Device tensors, simulator-owned, not synchronised to the host."""
    time: Any
    goal: Any           # [B, G] int32: per kept region its representative cell (the region's cell nearest its centroid) as a linear index iy nx + ix; -1 = unused
    label: Any          # [B, ny, nx] int32: the smallest linear index of the cell's region, -1 off the frontier (small regions are labelled too)
    region: Any         # [B, G, 4] int32: label, size, sum of x, sum of y per kept region; -1, 0, 0, 0 on unused rows
    count: Any          # [B, 2] int32: regions of at least min_size cells (may exceed G), frontier cells
    origin: Any         # (x0, y0): the corner of cell (0, 0)
    cell: float
    frame: str          # "base" or "world" ("grid" for a bare tensor)

    def size(self):
        """int32 [B, G]: the cells per kept region, 0 on unused rows."""
        return self.region[..., 1]

    def centroid(self):
        """fp32 [B, G, 2]: the regions' centroids (x, y) in metres, origin + (sum / size + 0.5) cell; NaN on unused rows.  The
        centroid of a curved frontier need not be free: drive to goal_xy()."""
        import torch

        size = self.region[..., 1:2].to(torch.float32)
        o = torch.tensor([float(self.origin[0]), float(self.origin[1])], dtype=torch.float32, device=self.region.device)
        xy = o + (self.region[..., 2:4].to(torch.float32) / size + 0.5) * float(self.cell)      # 0 / 0 on an unused row
        return torch.where(size > 0, xy, torch.full_like(xy, float("nan")))

    def goal_xy(self):
        """fp32 [B, G, 2]: the centres (x, y) of the goal cells in metres; NaN where the goal is -1."""
        import torch

        nx = self.label.shape[-1]
        g = self.goal.clamp(min=0)
        ij = torch.stack((g % nx, torch.div(g, nx, rounding_mode="floor")), -1).to(torch.float32)
        o = torch.tensor([float(self.origin[0]), float(self.origin[1])], dtype=torch.float32, device=self.goal.device)
        xy = o + (ij + 0.5) * float(self.cell)
        return torch.where((self.goal >= 0).unsqueeze(-1), xy, torch.full_like(xy, float("nan")))

    def mask(self):
        """bool [B, ny, nx]: the cells of the kept, reported regions (those with a row in `region`)."""
        import torch

        B, ny, nx = self.label.shape
        kept = torch.zeros(B, ny * nx + 1, dtype=torch.bool, device=self.label.device)      # the last slot takes the unused rows
        rows = self.region[..., 0].to(torch.int64)
        kept.scatter_(1, torch.where(rows >= 0, rows, torch.full_like(rows, ny * nx)), True)
        kept[:, ny * nx] = False
        flat = self.label.reshape(B, ny * nx).to(torch.int64)
        return (kept.gather(1, flat.clamp(min=0)) & (flat >= 0)).view(B, ny, nx)


@dataclass
class StatusStretchBaseCommand:
    """New, without a reference counterpart: the base command of pull_base_command() (smj_navigation_to_velocity), the best of a
    table of candidate arcs judged on a navigation field and its costmap.  `v` and `w` are what set_base_velocity takes.  Device
    tensors, simulator-owned, not synchronised to the host."""
    time: Any
    cmd: Any            # [2, B] fp32: rows v [m/s] and w [rad/s]; the chosen candidate's command bit for bit, (0, 0) unless status is 0
    best: Any           # [B, 2] int32: the chosen candidate (-1 unless status is 0) and the status
    score: Any          # [B, K] int64 or None: every candidate's score, NO_SCORE for a blocked one
    cells: Any          # [B, K, P] int32 or None: the linear cell iy nx + ix of every point of the table, -1 outside the grid
    frame: str          # the navigation field's: "base", "world" or "grid"

    OK, ARRIVED, BLOCKED, OFF_GRID = 0, 1, 2, 3      # SMJ_DRIVE_*
    NO_SCORE = (1 << 63) - 1                          # SMJ_DRIVE_NO_SCORE

    @property
    def v(self):
        """fp32 [B]: a view of cmd's first row."""
        return self.cmd[0]

    @property
    def w(self):
        """fp32 [B]: a view of cmd's second row."""
        return self.cmd[1]

    @property
    def chosen(self):
        """int32 [B]: the chosen candidate's index, -1 unless status is 0."""
        return self.best[:, 0]

    @property
    def status(self):
        """int32 [B]: 0 ok, 1 arrived, 2 every candidate blocked, 3 the robot is off the grid or its pose is not finite."""
        return self.best[:, 1]

    def ok(self):
        return self.best[:, 1] == self.OK

    def arrived(self):
        return self.best[:, 1] == self.ARRIVED

    def blocked(self):
        return self.best[:, 1] == self.BLOCKED


@dataclass
class StatusStretchScanMatch:
    """New, without a reference counterpart: the pose estimate of pull_scan_match() (smj_scan_to_pose), the best of a window of
    rotations and whole-cell shifts round a prior, judged by the sum of a likelihood field under the scan's returns.  `pose` is what
    pull_base_command(pose=...) takes.  Device tensors, simulator-owned, not synchronised to the host."""
    time: Any
    pose: Any           # [3, B] fp32: rows x, y, theta in the field's frame; the winner's pose with status 0, the prior bit for bit otherwise
    best: Any           # [B, 4] int32: the winner's index (-1 unless status is 0), its score J (0 unless status is 0), the counted returns n, the status
    score: Any          # [B, T, 2 wy + 1, 2 wx + 1] int32 or None: J of every candidate
    cells: Any          # [B, T, nlidar, 2] int32 or None: (ix, iy) of every ray and rotation, NO_CELL twice where it has none
    angles: Any         # [T] fp32: the rotation offsets searched
    window: Any         # (wx, wy): the shifts searched, in cells on either side
    origin: Any         # (x0, y0): the corner of cell (0, 0)
    cell: float
    frame: str          # "world" or "grid"
    bias: Any = None    # [T] int32 or None: what a rotation costs (utils.scan_angles(weight=...))
    shift_weight: int = 0

    OK, FEW, OFF = 0, 1, 2      # SMJ_MATCH_*
    NO_CELL = -32768            # SMJ_MATCH_NO_CELL

    @property
    def status(self):
        """int32 [B]: 0 ok, 1 fewer returns than min_points, 2 the prior is not finite."""
        return self.best[:, 3]

    def ok(self):
        return self.best[:, 3] == self.OK

    def offset(self):
        """int32 [B, 3]: (dx, dy, t) of the winner -- shifts in cells and the row of `angles` -- from its index; zeros unless ok()."""
        import torch

        wx, wy = self.window
        i = self.best[:, 0].clamp(min=0)
        row = torch.div(i, 2 * wx + 1, rounding_mode="floor")
        off = torch.stack((i % (2 * wx + 1) - wx, row % (2 * wy + 1) - wy, torch.div(row, 2 * wy + 1, rounding_mode="floor")), 1)
        return torch.where(self.ok().unsqueeze(1), off, torch.zeros_like(off)).to(torch.int32)

    def fit(self):
        """fp32 [B]: S / (255 n), the mean reward of a counted return at the winner, 1 for a scan that lies on the map's obstacles;
        0 unless ok().  S is the winner's J with the rotation's bias and the shift's weight taken out again."""
        import torch

        off = self.offset().to(torch.int64)
        S = self.best[:, 1].to(torch.int64) + int(self.shift_weight) * (off[:, 0] ** 2 + off[:, 1] ** 2)
        if self.bias is not None:
            S = S + self.bias.to(torch.int64).clamp(0, 1 << 20)[off[:, 2]]
        n = self.best[:, 2].clamp(min=1).to(torch.float32)
        return torch.where(self.ok(), S.to(torch.float32) / (255.0 * n), torch.zeros_like(n))

    def refined(self):
        """fp32 [3, B]: `pose` moved to the vertex of the parabola through the winner's J and its two neighbours' along each of x, y
        (in cells) and theta (the neighbours in angle, whatever their rows in `angles`).  Along an axis on which the winner lies on
        the border of the window, or whose three scores are no proper maximum, the winner itself stays; so do envs that are not
        ok().  Needs pull_scan_match(scores=True)."""
        import torch

        if self.score is None:
            raise ValueError("refined() needs pull_scan_match(scores=True)")
        B, T, WY, WX = self.score.shape
        off = self.offset().to(torch.int64)
        ix, iy, t = off[:, 0] + self.window[0], off[:, 1] + self.window[1], off[:, 2]
        J = self.score.to(torch.float64)
        e = torch.arange(B, device=J.device)

        def vertex(j0, j1, j2, a0, a1, a2, inner):
            """The abscissa, relative to a1, of the vertex of the parabola through (a0, j0), (a1, j1), (a2, j2); 0 where not inner."""
            u, v = a1 - a0, a1 - a2
            num = u * u * (j1 - j2) - v * v * (j1 - j0)
            den = u * (j1 - j2) - v * (j1 - j0)
            good = inner & (den != 0) & (j1 >= j0) & (j1 >= j2)
            return torch.where(good, -0.5 * num / torch.where(den != 0, den, torch.ones_like(den)), torch.zeros_like(num))

        one = torch.ones(B, dtype=torch.float64, device=J.device)
        xin, yin = (ix > 0) & (ix < WX - 1), (iy > 0) & (iy < WY - 1)
        sx = vertex(J[e, t, iy, (ix - 1).clamp(min=0)], J[e, t, iy, ix], J[e, t, iy, (ix + 1).clamp(max=WX - 1)], -one, 0 * one, one, xin)
        sy = vertex(J[e, t, (iy - 1).clamp(min=0), ix], J[e, t, iy, ix], J[e, t, (iy + 1).clamp(max=WY - 1), ix], -one, 0 * one, one, yin)
        ang = self.angles.to(torch.float64)
        order = torch.argsort(ang)
        rank = torch.argsort(order)[t]                                   # the winner's place among the sorted angles
        lo, hi = order[(rank - 1).clamp(min=0)], order[(rank + 1).clamp(max=T - 1)]
        st = vertex(J[e, lo, iy, ix], J[e, t, iy, ix], J[e, hi, iy, ix], ang[lo], ang[t], ang[hi], (rank > 0) & (rank < T - 1))
        ok = self.ok()
        delta = torch.stack((sx * float(self.cell), sy * float(self.cell), st), 0)
        return torch.where(ok.unsqueeze(0), (self.pose.to(torch.float64) + delta).to(torch.float32), self.pose)


@dataclass
class StatusStretchMapUpdate:
    """New, without a reference counterpart: what pull_map_update() (smj_scan_to_map) did with the lidar scan of the last step -- the
    map it was added to, as a StatusStretchOccupancyGrid that pull_distance_field(), pull_scan_match(), pull_frontiers() and
    pull_navigation_field() take as it is, and per env whether and how much was integrated.  Device tensors, simulator-owned, not
    synchronised to the host."""
    time: Any
    grid: Any           # StatusStretchOccupancyGrid: the map after the update; its tensors are the ones handed in, or the simulator's
    info: Any           # [B, 4] int32: the status, the returns kept, the clearing rays kept, the rays a guard dropped (0, 0, 0 unless the status is 0)
    cells: Any          # [B, nlidar, 4] int32 or None: (ax, ay, bx, by) of every kept ray, NO_CELL four times where it has none

    OK, GATED, OFF = 0, 1, 2      # SMJ_MAP_*
    NO_CELL = -(1 << 30)          # SMJ_MAP_NO_CELL

    @property
    def status(self):
        """int32 [B]: 0 integrated, 1 held back by the gate, 2 the pose is not finite."""
        return self.info[:, 0]

    def integrated(self):
        return self.info[:, 0] == self.OK

    def gated(self):
        return self.info[:, 0] == self.GATED

    def returns(self):
        """int32 [B]: the returns that went into the map, 0 for an env that was not integrated."""
        return self.info[:, 1]


@dataclass
class StatusStretchParticles:
    """New, without a reference counterpart: one measurement update of a particle filter, pull_particle_update()
    (smj_scan_to_particles) -- per env P pose hypotheses weighted by the lidar scan of the last step against a likelihood field,
    and resampled.  `particles` goes into the next call (after predict(), when the robot has moved); `pose`, the best particle, is
    what pull_scan_match(prior=...), pull_map_update() and pull_base_command(pose=...) take; `stat[:, 3]` gates pull_map_update()
    where it lies.  Everything after the weights is integers, so two calls give identical tensors.  Device tensors,
    simulator-owned, not synchronised to the host."""
    time: Any
    particles: Any      # [3, B, P] fp32: rows x, y, theta in the field's frame AFTER the update: resampled (plus noise) with status 0 and resample, the input bit for bit otherwise
    weights: Any        # [B, P] int32: S of every INPUT particle, the sum of the field under the scan's returns laid out from it, whatever the status
    ancestors: Any      # [B, P] int32 or None: the input particle slot k was drawn from; k itself where nothing was resampled
    stat: Any           # [B, 8] int32: the best particle (-1 unless status 0), its S, the counted returns n, the status, total, the effective sample size, cut, the distinct ancestors
    pose: Any           # [3, B] fp32: the best INPUT particle with status 0, NaN otherwise
    prior: Any          # [3, B, P] fp32: the particles that were weighed (the input of the call, as the kernel read it)
    origin: Any         # (x0, y0): the corner of cell (0, 0)
    cell: float
    frame: str          # "world" or "grid"

    OK, FEW, LOST = 0, 1, 2      # SMJ_MCL_*

    @property
    def status(self):
        """int32 [B]: 0 ok, 1 fewer returns than min_points, 2 no particle puts a return on a rewarded cell."""
        return self.stat[:, 3]

    def ok(self):
        return self.stat[:, 3] == self.OK

    def few(self):
        return self.stat[:, 3] == self.FEW

    def lost(self):
        return self.stat[:, 3] == self.LOST

    def best(self):
        """int32 [B]: the input particle with the largest S, the smallest index among equal S; -1 unless ok()."""
        return self.stat[:, 0]

    def ess(self):
        """int32 [B]: the effective sample size floor(total^2 / sum of w^2) of the input particles, between 1 and P; 0 unless ok()."""
        return self.stat[:, 5]

    def total(self):
        """int32 [B]: the sum of w; 0 unless ok()."""
        return self.stat[:, 4]

    def w(self):
        """int32 [B, P]: w_j = max(S_j - cut, 0), what the resampling drew by, recomputed from `weights` and the cut in `stat`."""
        return (self.weights - self.stat[:, 6:7]).clamp(min=0)

    def _moments(self):
        import torch

        w = self.w().to(torch.float64)                                     # [B, P]
        live = w > 0                                                       # a particle of weight 0 may be anything, NaN included
        p = torch.where(live.unsqueeze(0), self.prior.to(torch.float64), torch.zeros((), dtype=torch.float64, device=w.device))
        return w, p, w.sum(1)

    def mean(self):
        """fp32 [3, B]: the mean pose of the INPUT particles weighted by w (summed in fp64), theta as the direction of the mean unit
        vector; NaN for an env whose weights sum to 0.  With few particles left far from the best one this is the smoother estimate;
        `pose` is the one that is exact."""
        import torch

        w, p, tot = self._moments()
        x, y = (w * p[0]).sum(1) / tot, (w * p[1]).sum(1) / tot
        th = torch.atan2((w * torch.sin(p[2])).sum(1) / tot, (w * torch.cos(p[2])).sum(1) / tot)
        return torch.stack((x, y, th), 0).to(torch.float32)

    def spread(self):
        """fp32 [3, B]: the weighted standard deviations of x and y [m] about mean(), and the circular standard deviation of theta
        [rad], sqrt(-2 ln R) with R the length of the mean unit vector; NaN for an env whose weights sum to 0."""
        import torch

        w, p, tot = self._moments()
        mx, my = (w * p[0]).sum(1) / tot, (w * p[1]).sum(1) / tot
        sx = torch.sqrt((w * (p[0] - mx.unsqueeze(1)) ** 2).sum(1) / tot)
        sy = torch.sqrt((w * (p[1] - my.unsqueeze(1)) ** 2).sum(1) / tot)
        R = torch.hypot((w * torch.sin(p[2])).sum(1) / tot, (w * torch.cos(p[2])).sum(1) / tot).clamp(max=1.0)
        return torch.stack((sx, sy, torch.sqrt(-2.0 * torch.log(R))), 0).to(torch.float32)

    def predict(self, delta, noise=None):
        """fp32 [3, B, P], a new tensor: every particle of `particles` moved by the odometry increment delta = (dx, dy, dtheta), given
        in the robot's frame (x forward, y left) as three numbers or a tensor [3] or [3, B], plus noise [3, B, P] (None: none;
        utils.particle_noise).  Elementwise torch: the motion update between two pull_particle_update() calls."""
        import torch

        part = self.particles
        d = torch.as_tensor(delta, dtype=torch.float32, device=part.device)
        if d.dim() not in (1, 2) or d.shape[0] != 3 or (d.dim() == 2 and d.shape[1] != part.shape[1]):
            raise ValueError(f"delta: (dx, dy, dtheta) as [3] or [3, num_envs = {part.shape[1]}]")
        d = d.reshape(3, -1, 1)
        c, s = torch.cos(part[2]), torch.sin(part[2])
        out = torch.stack((part[0] + c * d[0] - s * d[1], part[1] + s * d[0] + c * d[1], part[2] + d[2]), 0)
        if noise is not None:
            if tuple(noise.shape) != tuple(part.shape):
                raise ValueError(f"noise: None or a tensor {tuple(part.shape)}")
            out = out + noise.to(out.dtype)
        return out


@dataclass
class StatusStretchNavigationField:
    """New, without a reference counterpart: the exact cost-to-goal field of pull_navigation_field() (smj_costmap_to_navigation) over
    a grid laid out as StatusStretchOccupancyGrid's.  `potential` and `next` are exact integers; the helpers turn them into metres,
    offsets, headings and paths in torch.  Device tensors, simulator-owned, not synchronised to the host."""
    time: Any
    potential: Any      # [B, ny, nx] int32: cheapest path cost to a goal (axial move 5 (w(a) + w(b)), diagonal 7 (w(a) + w(b)), w = neutral + cost), 0 on a goal, NONE where there is no path
    next: Any           # [B, ny, nx] int32 or None: linear index iy nx + ix of the neighbour to step to (the smallest among equally good ones), the cell itself on a goal, -1 where none
    goal: Any           # [B, G] int32: the goal cells used, as linear indices; -1 = unused
    origin: Any         # (x0, y0): the corner of cell (0, 0)
    cell: float
    frame: str          # "base" or "world" ("grid" for a bare cost tensor)
    neutral: int        # the weight of a zero-cost cell

    NONE = 1 << 30      # SMJ_NAV_NONE

    def distance(self):
        """fp32 [B, ny, nx]: potential cell / (10 neutral) -- on a zero-cost map the octile path length to the goal in metres; inf
        where there is no path."""
        import torch

        return _inf_where_none(self.potential.to(torch.float32) * (float(self.cell) / (10.0 * float(self.neutral))), self.potential, self.NONE)

    def next_offset(self):
        """int32 [B, ny, nx, 2]: (dy, dx) in cells from each cell to the neighbour to step to, zeros on goals and where there is no
        path.  Needs pull_navigation_field(next=True)."""
        if self.next is None:
            raise ValueError("next_offset() needs pull_navigation_field(next=True)")
        return offsets_of_cells(self.next)

    def heading(self):
        """fp32 [B, ny, nx]: atan2(dy, dx) of next_offset(), the direction to drive in the grid's frame; NaN on goals and where there
        is no path."""
        import torch

        off = self.next_offset().to(torch.float32)
        h = torch.atan2(off[..., 0], off[..., 1])
        still = (off[..., 0] == 0) & (off[..., 1] == 0)
        return torch.where(still, torch.tensor(float("nan"), dtype=torch.float32, device=h.device), h)

    def path(self, start, max_steps: int):
        """int64 [B, max_steps + 1]: the cells visited from `start` along next, the start first; once the goal is reached the path
        stays on it.  start, one per env: (x, y) in metres, a tensor [B, 2] in metres, or an int tensor [B] of cell indices.  -1
        throughout for a start outside the grid or without a path.  Needs pull_navigation_field(next=True)."""
        import torch

        if self.next is None:
            raise ValueError("path() needs pull_navigation_field(next=True)")
        max_steps = int(max_steps)
        if max_steps < 0:
            raise ValueError("max_steps must be >= 0")
        B, ny, nx = self.next.shape
        dev = self.next.device
        if not isinstance(start, torch.Tensor):
            try:
                x, y = (float(v) for v in start)
            except (TypeError, ValueError):
                raise ValueError("start: (x, y) in metres, a tensor [B, 2], or an int tensor [B] of cell indices") from None
            start = torch.tensor([[x, y]], dtype=torch.float32, device=dev).expand(B, 2)
        start = start.to(dev)
        if start.is_floating_point():
            if tuple(start.shape) != (B, 2):
                raise ValueError(f"start in metres: [B = {B}, 2]")
            cur = cells_of_points(start, self.origin, self.cell, ny, nx).to(torch.int64)
        else:
            if tuple(start.shape) != (B,):
                raise ValueError(f"start as cell indices: [B = {B}]")
            cur = start.to(torch.int64)
            cur = torch.where((cur >= 0) & (cur < ny * nx), cur, torch.full_like(cur, -1))
        flat = self.next.reshape(B, ny * nx).to(torch.int64)
        step = lambda c: torch.where(c >= 0, flat.gather(1, c.clamp(min=0).unsqueeze(1)).squeeze(1), c)
        cur = torch.where(step(cur) >= 0, cur, torch.full_like(cur, -1))      # a start without a path
        out = [cur]
        for _ in range(max_steps):
            cur = step(cur)
            out.append(cur)
        return torch.stack(out, 1)


@dataclass
class StatusStretchContacts:
    """New, without a reference counterpart (like `step` / `reset`): the contact list of every env's last physics step and its
    constraint forces -- what MuJoCo users read from MjData.contact and mj_contactForce after mj_step.  Every field is a device
    tensor, not synchronised to the host; C is the record capacity (SMJ_DIM_CONTACT_CAP), entries past `count` are masked off
    by `valid` and zero.  The order is the kernel's, not MuJoCo's."""
    time: Any
    count: Any          # [B] int32: contacts of the last step (INFO[1])
    valid: Any          # [B, C] bool: contact index < count
    geom: Any           # [B, C, 2] int32: geom1, geom2 (fused model)
    body: Any           # [B, C, 2] int64: original MJCF body ids of the geoms (names["body"])
    dist: Any           # [B, C]
    pos: Any            # [B, C, 3] world
    frame: Any          # [B, C, 3, 3] row 0 the normal from geom1 to geom2, rows 1-2 tangents
    force: Any          # [B, C, 6] contact frame: normal, tangent 1, tangent 2, torsional, rolling 1, rolling 2
    force_world: Any    # [B, C, 3] linear force on geom2's body, world frame (frame' force[:3]); geom1's body gets the opposite
    condim: Any = None  # [B, C] int32: condim used
    efc_adr: Any = None  # [B, C] int32: first constraint row, -1 when the contact entered no rows

    @staticmethod
    def from_records(records, count, geom_body, time=None) -> "StatusStretchContacts":
        """Decode the env-major records [B, C, 24] of SMJ_SLOT_CONTACTS (lib.CON word offsets; the int words are int32 bit
        patterns) with the per-env contact counts [B] and the geom -> MJCF body map [ngeom] (int64), on the records' device."""
        import torch

        from .lib import CON

        B, C, _ = records.shape
        ints = records.view(torch.int32)
        valid = torch.arange(C, device=records.device).unsqueeze(0) < count.to(records.device).long().unsqueeze(1)
        vf = valid.unsqueeze(-1)
        zf, zi = torch.zeros((), dtype=records.dtype, device=records.device), torch.zeros((), dtype=torch.int32, device=records.device)
        geom = torch.where(vf, ints[:, :, CON["GEOM1"]:CON["GEOM2"] + 1], zi)
        nb = geom_body.shape[0]
        body = geom_body[geom.long().clamp(0, nb - 1)]
        frame = torch.where(vf, records[:, :, CON["FRAME"]:CON["FRAME"] + 9], zf).reshape(B, C, 3, 3)
        force = torch.where(vf, records[:, :, CON["FORCE"]:CON["FORCE"] + 6], zf)
        fw = (frame.transpose(-1, -2) @ force[..., :3].unsqueeze(-1)).squeeze(-1)
        return StatusStretchContacts(
            time=time, count=count, valid=valid, geom=geom, body=body,
            dist=torch.where(valid, records[:, :, CON["DIST"]], zf), pos=torch.where(vf, records[:, :, CON["POS"]:CON["POS"] + 3], zf),
            frame=frame, force=force, force_world=fw,
            condim=torch.where(valid, ints[:, :, CON["CONDIM"]], zi), efc_adr=torch.where(valid, ints[:, :, CON["EFC_ADR"]], zi - 1))

    def _sides(self, body_ids, other_ids=None):
        """[B, C] masks: the contact's geom2 body is in `body_ids` and its geom1 body in `other_ids` (any when None), and the
        same with geom1 / geom2 exchanged.  Ids already on the records' device are used as they are (no copy, no host sync)."""
        import torch

        S = torch.as_tensor(body_ids, dtype=self.body.dtype, device=self.body.device).reshape(-1)
        b1, b2 = self.body[..., 0], self.body[..., 1]
        in1, in2 = torch.isin(b1, S), torch.isin(b2, S)
        if other_ids is None:
            o1 = o2 = torch.ones_like(in1)
        else:
            O = torch.as_tensor(other_ids, dtype=self.body.dtype, device=self.body.device).reshape(-1)
            o1, o2 = torch.isin(b1, O), torch.isin(b2, O)
        return in2 & o1 & self.valid, in1 & o2 & self.valid

    def net_force(self, body_ids, other_ids=None):
        """[B, 3] world-frame net contact force on the bodies `body_ids` from `other_ids` (from everything when None): each
        contact counts + on geom2's body and - on geom1's, so contacts inside the set cancel."""
        on2, on1 = self._sides(body_ids, other_ids)
        sgn = on2.to(self.force_world.dtype) - on1.to(self.force_world.dtype)
        return (sgn.unsqueeze(-1) * self.force_world).sum(1)

    def touching(self, body_ids, other_ids=None):
        """[B] bool: a contact between the two sets entered the constraint system (efc_adr >= 0)."""
        on2, on1 = self._sides(body_ids, other_ids)
        return ((on2 | on1) & (self.efc_adr >= 0)).any(1)
