"""StretchBatchSimulator -- the reference's StretchMujocoSimulator API with a leading batch dimension.

Reference: stretch_mujoco/stretch_mujoco_simulator.py:34-534 (client) + stretch_mujoco/mujoco_server.py (server).
The server process, proxies, locks and the realtime sleep (mujoco_server.py:381-384) have no place in a batched
throughput simulator: one Python object owns PyTorch-ROCm tensors (batch-major, [dim, B]) and drives the HIP
library through the ctypes C-ABI (lib.py, include/smj.h).  New, without a reference counterpart: `step(n)`,
`reset(env_ids)`, with `contacts=True` the contact readout `pull_contact_data()`, `contact_force()`, `in_contact()`, and the organised
point clouds of the depth cameras, `pull_point_cloud()`.

Ordering contract kept from `_ctrl_callback` (mujoco_server.py:450-463): commands issued between steps are
folded into ctrl before the next physics step; status is the post-step readout.
"""
from __future__ import annotations

import ctypes
import json
import math
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import lib as _lib
from . import model_blob
from .datamodels import StatusStretchBaseCommand, StatusStretchCameras,StatusStretchContacts, StatusStretchDistanceField, StatusStretchFrontiers, StatusStretchHeightMap, StatusStretchJoints, StatusStretchMapUpdate, StatusStretchNavigationField, StatusStretchOccupancyGrid, StatusStretchParticles, StatusStretchScanMatch, StatusStretchSensors, cells_of_points
from .enums import Actuators, StretchCameras, StretchSensors
from .glue import Glue

_MODELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "models")


def vp(t):
    """The device pointer of a tensor as the C-ABI takes it; None stays None (an optional buffer left out)."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _check_range_limits(r_min, r_max, cell):
    """What every entry that reads the scan asks of its range limits once they are floats."""
    if not (np.isfinite(r_min) and np.isfinite(r_max) and 0 <= r_min <= r_max):
        raise ValueError("range_limits: finite, 0 <= r_min <= r_max")
    if np.float32(r_max) / np.float32(cell) > 8192:
        raise ValueError("range_limits[1] / cell must not exceed 8192")


def _require_connection(fn):
    def wrapper(self, *a, **k):
        if not self.is_running():
            raise ConnectionError("The Stretch Mujoco Simulator is not running. Use the start() method to start it.")
        return fn(self, *a, **k)

    wrapper.__name__ = fn.__name__
    wrapper.__doc__ = fn.__doc__
    return wrapper


class StretchBatchSimulator:
    def __init__(self, num_envs: int = 1, device: str = "cuda:0", scene: str = "stretch_empty",
                 model_blob_bytes: Optional[bytes] = None, sensors_to_use: Sequence[StretchSensors] = (),
                 cameras_to_use: Sequence[StretchCameras] = (), start_translation=None, start_rotation_quat=None,
                 debug: bool = False, solver: str = "newton", contacts: bool = False):
        self.num_envs = int(num_envs)
        self.device = torch.device(device)
        if model_blob_bytes is None:
            if scene.endswith(".xml"):
                # any MJCF scene that includes stretch.xml (the reference's `scene_xml_path`, stretch_mujoco_simulator.py:47-55):
                # compiled here with the build's own MJCF compiler; needs the mesh assets next to the XML
                from . import mjcf_compiler, model_fuse

                # (a scene beyond the dense builds' 64 dofs / 32 bodies / 128 collision geoms -- a kitchen -- is prepared for the satellite builds)
                model_blob_bytes = model_blob.dumps(model_fuse.prepare_for_kernels(mjcf_compiler.compile_file(scene), satellites="auto"))
            else:
                with open(os.path.join(_MODELS, scene + ".smjb"), "rb") as f:
                    model_blob_bytes = f.read()
        self._blob = model_blob_bytes
        self.model = model_blob.loads(model_blob_bytes)
        self.names = json.loads(model_blob.get_str(self.model, "names_json"))
        self._sensors = list(sensors_to_use)
        self._cameras = list(cameras_to_use)
        # depth cameras: metric depth (smj_render_depth).  RGB cameras: an unlit-albedo STAND-IN (smj_render_rgb: geom / material
        # rgba of the first geom each pixel ray meets, uint8 [B, H, W, 3]) -- MuJoCo's lighting, textures and shadows are not on
        # this path (scope)
        self._start_translation = start_translation
        self._start_rotation_quat = start_rotation_quat
        self._debug = debug
        self._contacts = bool(contacts)   # contact list + forces of the last step (SMJ_SLOT_CONTACTS), read by pull_contact_data()
        if solver not in ("pgs", "newton"):
            raise ValueError("solver must be 'pgs' (north_star) or 'newton' (the reference model's default)")
        self.solver = solver
        self._ctx = None
        self._L = None
        self.timestep = float(self.model["opt_timestep"][0])

    # ------------------------------------------------------------------ lifecycle
    def start(self, headless: bool = True, home: bool = True, **_ignored) -> None:
        """Allocate, reset and (like the reference, stretch_mujoco_simulator.py:136) send the robot home."""
        if self._ctx is not None:
            return
        if self.device.type != "cuda":
            raise _lib.SmjError("the physics path runs on the ROCm device only; there is no CPU fallback")
        L = self._L = _lib.load()
        ctx = ctypes.c_void_p()
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        rc = L.smj_create(self._blob, len(self._blob), self.num_envs, dev_index, ctypes.byref(ctx))
        if rc != 0:
            msg = L.smj_last_error(ctx).decode() if ctx else "smj_create failed"
            if ctx:
                L.smj_destroy(ctx)
            raise _lib.SmjError(f"smj_create failed ({rc}): {msg}")
        self._ctx = ctx
        dims = (ctypes.c_int * 16)()
        _lib.check(L, ctx, L.smj_dims(ctx, dims), "smj_dims")
        D = _lib.DIM
        self.nq, self.nv, self.nu = dims[D["NQ"]], dims[D["NV"]], dims[D["NU"]]
        self.nlidar = dims[D["NLIDAR"]]
        # capacities of the kernel variant smj_create chose for this model (standard: 32 dofs / 80 rows / 16 contacts; big: 64 / 160 / 48)
        self.nv_max, self.nefc_max, self.ncon_max = dims[D["NV_MAX"]], dims[D["NEFC_MAX"]], dims[D["NCON_MAX"]]
        self.nsat_max = dims[D["NSAT_MAX"]]   # > 0: the model runs on a satellite build of the step kernel (csrc/smj_sat.h)
        self.debug_layout = _lib.debug_layout(self.nv_max, self.ncon_max, self.nsat_max)
        B, f = self.num_envs, dict(dtype=torch.float32, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        self.qpos = torch.zeros(self.nq, B, **f); self.qvel = torch.zeros(self.nv, B, **f)
        nu1 = max(self.nu, 1)   # (a model without actuators -- a scene of objects only -- still binds every slot: zero-row views of real storage)
        store = {k: torch.zeros(nu1, B, **f) for k in ("ctrl", "actlen", "actvel")}
        self.ctrl = store["ctrl"][: self.nu]; self.qacc_warmstart = torch.zeros(self.nv, B, **f)
        self.nstep = torch.zeros(B, **i32)
        self.actuator_length = store["actlen"][: self.nu]; self.actuator_velocity = store["actvel"][: self.nu]
        self._store = store
        self.base_pose = torch.zeros(3, B, **f)
        self.gyro = torch.zeros(3, B, **f); self.accel = torch.zeros(3, B, **f)
        self.lidar = torch.zeros(max(self.nlidar, 1), B, **f)
        self.info = torch.zeros(4, B, **i32)
        S = _lib.SLOT
        binds = [("QPOS", self.qpos), ("QVEL", self.qvel), ("CTRL", store["ctrl"]), ("WARMSTART", self.qacc_warmstart),
                 ("NSTEP", self.nstep), ("ACT_LENGTH", store["actlen"]), ("ACT_VELOCITY", store["actvel"]),
                 ("BASE_POSE", self.base_pose), ("GYRO", self.gyro), ("ACCEL", self.accel), ("LIDAR", self.lidar),
                 ("INFO", self.info)]
        if self._debug:
            self.debug = torch.zeros(dims[D["DEBUG_FLOATS"]], B, **f)
            self.prof = torch.zeros(48, B, **f)
            binds.append(("DEBUG", self.debug))
            binds.append(("PROF", self.prof))
        for name, t in binds:
            _lib.check(L, ctx, L.smj_bind(ctx, S[name], ctypes.c_void_p(t.data_ptr()), B), f"smj_bind({name})")
        key_ctrl = torch.tensor(np.asarray(self.model["key_ctrl"], np.float32)[:, : self.nu])
        self.glue = Glue(B, self.nu, key_ctrl, self.names["key"], self.device)
        # the relative base moves (BaseController) advance inside the step kernel: its per-env state is the glue's tensor
        _lib.check(L, ctx, L.smj_bind(ctx, S["BASECTL"], ctypes.c_void_p(self.glue.bctl.data_ptr()), B), "smj_bind(BASECTL)")
        self.launches = 0   # smj_step launches so far (tests: a base move in flight must not multiply them)
        self.set_option("solver", {"pgs": 0, "newton": 2}[self.solver])
        self._read_flags = 0
        if StretchSensors.base_gyro in self._sensors or StretchSensors.base_accel in self._sensors:
            self._read_flags |= _lib.READ_IMU
        if StretchSensors.base_lidar in self._sensors:
            self._read_flags |= _lib.READ_LIDAR
        self._depth = {}
        self._depth_valid = set()   # depth cameras whose image has been rendered (pull_point_cloud(render=False) needs one)
        self._hmaps = {}            # (frame, (ny, nx)) -> the simulator-owned (height, count) of pull_height_map
        self._occ = {}              # (frame, (ny, nx)) -> the simulator-owned (hit, miss) of pull_occupancy_grid
        self._nav = {}              # (ny, nx, G) -> the simulator-owned [potential, next or None, goal] of pull_navigation_field
        self._front = {}            # (ny, nx, G) -> the simulator-owned [label, goal, region, count, hit, miss] of pull_frontiers
        self._drive = {}            # (K, P, ny, nx) -> the simulator-owned cmd, best, score, cells, twist and pose of pull_base_command
        self._drive_default = None  # arc_candidates() on the device, made by the first pull_base_command without a table
        self._match = {}            # (T, wx, wy, ny, nx) -> the simulator-owned pose, best, score, cells and prior of pull_scan_match
        self._maps = {}             # (ny, nx) -> the simulator-owned hit, miss, info and cells of pull_map_update
        self._match_default = None  # scan_angles() on the device, made by the first pull_scan_match without a table
        self._particles = {}        # (P, ny, nx) -> the simulator-owned tensors of pull_particle_update: two particle sets that take turns, weights, ancestors, stat, pose, draw
        self._draw_generator = None # the torch.Generator on the device that pull_particle_update(draw=None) draws its random words from
        self._dist = {}             # (ny, nx) -> the simulator-owned [dist2, nearest or None] of pull_distance_field
        self._points = {}           # (camera, stride) -> the simulator-owned point cloud of pull_point_cloud
        # body poses of the last step: input of the depth renderer and of get_link_pose (240 floats per env, always on)
        self.xpose = torch.zeros(dims[D["NBODY"]] * 12, B, **f)
        _lib.check(L, ctx, L.smj_bind(ctx, S["XPOSE"], ctypes.c_void_p(self.xpose.data_ptr()), B), "smj_bind(XPOSE)")
        self._read_flags |= _lib.READ_POSES
        if self._contacts:
            # env-major records [B, cap, 24] (include/smj.h SMJ_CON_*), cap = the largest contact capacity a step can end in
            self.contact_cap = dims[D["CONTACT_CAP"]]
            self.contact_records = torch.zeros(B, self.contact_cap, _lib.CONTACT_WORDS, **f)
            _lib.check(L, ctx, L.smj_bind(ctx, S["CONTACTS"], ctypes.c_void_p(self.contact_records.data_ptr()), B), "smj_bind(CONTACTS)")
            self._read_flags |= _lib.READ_CONTACTS
            # geom -> original MJCF body (names["body"]): a fused blob keeps the body each geom was declared in
            gb = self.model["geom_origbody"] if "geom_origbody" in self.model else self.model["geom_bodyid"]
            self._geom_body = torch.as_tensor(np.asarray(gb, np.int64).reshape(-1), device=self.device)
            self._id_cache = {}   # body-name sets of contact_force / in_contact -> device id tensors
        if self._cameras:
            if dims[D["NCAM"]] == 0:
                raise _lib.SmjError("the model blob carries no render tables: depth cameras are unavailable for this scene")
            for cam in self._cameras:
                st = cam.initial_camera_settings
                if cam.is_depth:
                    self._depth[cam] = torch.zeros(B, st.height, st.width, **f)
                else:
                    self._depth[cam] = torch.zeros(B, st.height, st.width, 3, dtype=torch.uint8, device=self.device)
        self.reset()
        if home:
            self.home()

    def stop(self) -> None:
        if self._ctx is not None:
            torch.cuda.synchronize(self.device)
            self._L.smj_destroy(self._ctx)
            self._ctx = None

    def is_running(self) -> bool:
        return self._ctx is not None

    def __del__(self):
        try:
            self.stop()
        except Exception:
            pass

    def set_option(self, name: str, value: float) -> None:
        """mjOption-style knobs: iterations, tolerance, warmstart, pgs_fixed_iter, max_contacts_per_pair, solver."""
        _lib.check(self._L, self._ctx, self._L.smj_set_option(self._ctx, name.encode(), float(value)), f"smj_set_option({name})")

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ new: reset / step
    @_require_connection
    def reset(self, env_ids=None) -> None:
        """mj_resetData for the selected envs, then the start pose (change_start_pose, mujoco_server.py:206-229)."""
        if env_ids is None:
            mask_ptr = None
            ids = slice(None)
        else:
            ids = torch.as_tensor(env_ids, device=self.device, dtype=torch.long)
            mask = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device)
            mask[ids] = 1
            mask_ptr = ctypes.c_void_p(mask.data_ptr())
        _lib.check(self._L, self._ctx, self._L.smj_reset(self._ctx, mask_ptr, self._stream()), "smj_reset")
        if self._start_translation is not None:  # [3] for every env or [B,3]
            t = torch.as_tensor(self._start_translation, dtype=torch.float32, device=self.device).reshape(-1, 3)
            self.qpos[0:3, ids] = t.expand(self.num_envs, 3).t()[:, ids]
        if self._start_rotation_quat is not None:  # wxyz, [4] or [B,4]
            q = torch.as_tensor(self._start_rotation_quat, dtype=torch.float32, device=self.device).reshape(-1, 4)
            self.qpos[3:7, ids] = q.expand(self.num_envs, 4).t()[:, ids]
        self.glue.reset(env_ids)
        # readout of the reset state (one zero-length update is not available: refresh by a cheap kinematic fill)
        self.actuator_length[:, ids] = 0
        self.actuator_velocity[:, ids] = 0
        self.base_pose[0:2, ids] = self.qpos[0:2, ids]
        qw, qx, qy, qz = self.qpos[3, ids], self.qpos[4, ids], self.qpos[5, ids], self.qpos[6, ids]
        self.base_pose[2, ids] = torch.atan2(2 * (qx * qy + qw * qz), qw * qw + qx * qx - qy * qy - qz * qz)

    @_require_connection
    def step(self, n: int = 1) -> None:
        """Advance every env by n physics steps (n x `_physics_step`, mujoco_server.py:371-384, without the sleep)."""
        n = int(n)
        if n <= 0:
            return
        self._push_command()
        _lib.check(self._L, self._ctx, self._L.smj_step(self._ctx, n, self._read_flags, self._stream()), "smj_step")
        self.launches += 1

    def _push_command(self) -> None:
        """`_ctrl_callback` -> push_command (mujoco_server.py:450-463, :527-578): commands issued since the last step are folded
        into ctrl / the base-controller state on the device (masked ops, no host synchronisation); when one of them concerns
        the base (or a keyframe overwrote the wheel ctrl) one BaseController.update() runs as a HIP tick -- every later
        update happens inside the step kernel, after each physics step."""
        if self.glue.push_command(self.ctrl, self.actuator_length, self.base_pose, tick_base=False):
            _lib.check(self._L, self._ctx, self._L.smj_base_controller_tick(self._ctx, self._stream()), "smj_base_controller_tick")

    # ------------------------------------------------------------------ reference API
    @_require_connection
    def home(self, env_ids=None, settle: bool = True) -> None:
        """Keyframe 'home' then wait until the lift stops (stretch_mujoco_simulator.py:213-221)."""
        self.glue.set_keyframe("home", env_ids)
        if settle:
            self.wait_while_is_moving(Actuators.lift)

    @_require_connection
    def stow(self, env_ids=None, settle: bool = True) -> None:
        """Keyframe 'stow' then wait on wrist_pitch (stretch_mujoco_simulator.py:224-233)."""
        self.glue.set_keyframe("stow", env_ids)
        if settle:
            self.wait_while_is_moving(Actuators.wrist_pitch)

    @_require_connection
    def move_to(self, actuator, pos, env_ids=None) -> None:
        self.glue.move_to(actuator, pos, env_ids)

    @_require_connection
    def move_by(self, actuator, pos, env_ids=None) -> None:
        self.glue.move_by(actuator, pos, env_ids)

    @_require_connection
    def set_base_velocity(self, v_linear, omega, env_ids=None) -> None:
        self.glue.set_base_velocity(v_linear, omega, env_ids)

    @_require_connection
    def pull_status(self) -> StatusStretchJoints:
        return Glue.pull_status(self._time(), self.actuator_length, self.actuator_velocity, self.base_pose)

    @_require_connection
    def pull_sensor_data(self) -> StatusStretchSensors:
        """gyro [B,3], accel (field base_imu) [B,3], lidar [B,360]; values of the last physics step of the last launch.
        The reference refreshes these at 15 Hz wall clock (mujoco_server.py:271); here the cadence is the caller's step(n)."""
        out = StatusStretchSensors(time=self._time(), fps=0.0)
        if self._read_flags & _lib.READ_IMU:
            out.base_gyro = self.gyro.t().clone()
            out.base_imu = self.accel.t().clone()
        if self._read_flags & _lib.READ_LIDAR:
            out.lidar = self.lidar[: self.nlidar].t().clone()
        return out

    @_require_connection
    def pull_camera_data(self) -> StatusStretchCameras:
        """Depth images [B, H, W] (fp32 metres) and RGB stand-in images [B, H, W, 3] (uint8 unlit albedo, see __init__) of the
        cameras in cameras_to_use, rendered from the body poses of the last physics step
        (what Renderer.update_scene sees, mujoco_server_camera_manager.py:127-143), limited like
        StretchCameras.post_processing_callback; K as get_camera_params (:168-183: fovy with the SENSOR resolution).
        The reference renders at 30 Hz wall clock (mujoco_server.py:272); here the cadence is the caller's.
        The image tensors are simulator-owned and overwritten by the next call."""
        from .utils import compute_K

        out = StatusStretchCameras(time=self._time(), fps=0.0)
        for cam in self._cameras:
            if cam.is_depth:
                img = self._depth_image(cam, True)
            else:
                img = self._depth[cam]
                rc = self._L.smj_render_rgb(self._ctx, *self._camera_args(cam), ctypes.c_void_p(img.data_ptr()), None, self._stream())
                _lib.check(self._L, self._ctx, rc, "smj_render_rgb")
            out.set_camera_data(cam, img)
        for attr, cam in (("cam_d405_K", StretchCameras.cam_d405_rgb), ("cam_d435i_K", StretchCameras.cam_d435i_rgb)):
            st = cam.initial_camera_settings
            setattr(out, attr, compute_K(st.field_of_view_vertical_in_degrees, st.sensor_resolution[0], st.sensor_resolution[1]))
        return out

    # ------------------------------------------------------------------ shared by the pull_* of the perception entries
    def _time(self) -> torch.Tensor:
        return self.nstep.to(torch.float64) * self.timestep

    def _camera_args(self, cam):
        """(index, width, height, fovy): the leading arguments of every C entry that takes a camera."""
        st = cam.initial_camera_settings
        return self.names["camera"].index(cam.camera_name_in_mjcf), st.width, st.height, float(st.field_of_view_vertical_in_degrees)

    def _render_depth_into(self, cam, img) -> None:
        rc = self._L.smj_render_depth(self._ctx, *self._camera_args(cam), cam.depth_limit, ctypes.c_void_p(img.data_ptr()), self._stream())
        _lib.check(self._L, self._ctx, rc, "smj_render_depth")

    def _depth_image(self, cam, render: bool) -> torch.Tensor:
        """The camera's depth image: rendered now (and marked valid), or the one of an earlier call, which there must have been."""
        img = self._depth[cam]
        if render:
            self._render_depth_into(cam, img)
            self._depth_valid.add(cam)
        elif cam not in self._depth_valid:
            raise _lib.SmjError(f"render=False: {cam.name} has not been rendered yet (pull_camera_data() or pull_point_cloud() first)")
        return img

    def _base_frame(self):
        """(fused body base_link lives in, its fixed pose there as (r, R) or None where that pose is the identity)."""
        i = self.names["body"].index("base_link")
        rp = np.asarray(self.model["link_relpos"][i], np.float64)
        Rl = self._quat_mat(self.model["link_relquat"][i], self.device)
        identity = not np.any(rp != 0) and torch.equal(Rl, torch.eye(3, device=self.device))
        return int(self.model["link_fused"][i]), None if identity else (torch.tensor(rp, dtype=torch.float32, device=self.device), Rl)

    def _frame_id(self, frame, allowed):
        """Frame name -> (the C entries' frame id, base_link's fixed offset inside that body or None)."""
        if frame not in allowed:
            quoted = [f'"{a}"' for a in allowed]
            raise ValueError(f'frame must be {", ".join(quoted[:-1])} or {quoted[-1]}')
        if frame == "base":
            return self._base_frame()
        return (_lib.FRAME_CAMERA if frame == "camera" else _lib.FRAME_WORLD), None

    def _need_lidar(self):
        if not self._read_flags & _lib.READ_LIDAR:
            raise _lib.SmjError("the lidar readout is off: put StretchSensors.base_lidar into sensors_to_use")

    def _need_scan(self, entry):
        """The head of the entries that take the scan in the robot's frame: the readout is on, the scan is one `entry` takes."""
        self._need_lidar()
        if self.nlidar > 1024:
            raise _lib.SmjError(f"the model has {self.nlidar} lidar rays: {entry} takes 1024")

    def _robot_body(self, what):
        """The body whose frame is the robot's, for the same entries; `what` of the scan cannot be formed when base_link is offset in it."""
        body, offset = self._base_frame()
        if offset is not None:
            raise ValueError(f"base_link sits at a non-identity fixed pose inside its fused body: the scan's {what} cannot be formed in "
                             "the robot's frame")
        return body

    @staticmethod
    def _grid_args(shape, origin, cell, pair, pair_doc):
        """(ny, nx, x0, y0, cell, lo, hi) of a binned map, checked; `pair` is the entry's own interval (z_range, range_limits)."""
        try:
            ny, nx = (int(v) for v in shape)
            x0, y0 = (float(v) for v in origin)
            lo, hi = (float(v) for v in pair)
        except (TypeError, ValueError):
            raise ValueError(f"shape = (ny, nx), origin = (x0, y0), {pair_doc}") from None
        if ny < 1 or nx < 1 or ny * nx > 65536:
            raise ValueError("shape: ny, nx >= 1 and ny * nx <= 65536")
        cell = float(cell)
        if not (np.isfinite(cell) and cell > 0):
            raise ValueError("cell must be finite and > 0")
        if not (np.isfinite(x0) and np.isfinite(y0)):
            raise ValueError("origin must be finite")
        return ny, nx, x0, y0, cell, lo, hi

    @staticmethod
    def _cached(cache, key, make):
        """The simulator-owned buffers of `key`, made on first use."""
        bufs = cache.get(key)
        if bufs is None:
            bufs = cache[key] = make()
        return bufs

    def _cached_int_pair(self, cache, key, ny, nx, second, *extra):
        """The int32 buffers [first, second, *extra] of `key`: [B, ny, nx] twice, the second made by the first call that asks for it
        (`second`), and [B, *shape] per shape in `extra`.  Returns the list and this call's second buffer or None."""
        new = lambda *shape: torch.empty(self.num_envs, *shape, dtype=torch.int32, device=self.device)
        bufs = self._cached(cache, key, lambda: [new(ny, nx), None, *(new(*shape) for shape in extra)])
        if second and bufs[1] is None:
            bufs[1] = new(ny, nx)
        return bufs, bufs[1] if second else None

    @staticmethod
    def _upstream_kwargs(kwargs, upstream, called, cell, origin):
        """The keywords of the pull a grid entry runs when handed no input (`called`): cell and origin join them; an entry that
        was handed its input takes none.  `upstream`: that pull's name and the argument whose None triggers it."""
        if called:
            kwargs.update({k: v for k, v in (("cell", cell), ("origin", origin)) if v is not None})
        elif kwargs:
            raise ValueError(f"{sorted(kwargs)}: keywords of {upstream[0]}, which is called only for {upstream[1]}=None")

    @staticmethod
    def _origin_cell(status, origin, cell):
        """((x0, y0), cell) of a grid entry's input, cell checked: those of the Status* object `status` (the keywords are refused
        then) or, for a bare tensor (status None), the keywords, (0, 0) and 1.0 if absent."""
        if status is not None:
            if cell is not None or origin is not None:
                raise ValueError(f"cell and origin come from the {type(status).__name__}")
            x0y0, cell = tuple(status.origin), float(status.cell)
        else:
            try:
                x0y0 = (0.0, 0.0) if origin is None else tuple(float(v) for v in origin)
                cell = 1.0 if cell is None else float(cell)
            except (TypeError, ValueError):
                raise ValueError("origin = (x0, y0), cell a number") from None
            if len(x0y0) != 2 or not (np.isfinite(x0y0[0]) and np.isfinite(x0y0[1])):
                raise ValueError("origin = (x0, y0), finite")
        if not (np.isfinite(cell) and cell > 0):
            raise ValueError("cell must be finite and > 0")
        return x0y0, cell

    @staticmethod
    def _check_cell_count(what, ny, nx):
        """The limit of the integer-grid kernels (SMJ_EDT_MAX_*, SMJ_NAV_MAX_*)."""
        if ny < 1 or nx < 1 or ny > 4096 or nx > 4096 or ny * nx > 65536:
            raise ValueError(f"{what}: 1 <= ny, nx <= 4096 and ny * nx <= 65536")

    @_require_connection
    def pull_point_cloud(self, camera: StretchCameras, frame: str = "camera", stride: int = 1, render: bool = True,
                         auto_rotate: bool = False) -> torch.Tensor:
        """Organised point cloud [B, H', W', 3] (fp32 metres) of a depth camera of cameras_to_use, one fused pass over its depth
        image (smj_depth_to_points, include/smj_pointcloud.h).  New, without a reference counterpart: users of the reference deproject
        pull_camera_data() by hand -- and the cam_*_K fields do not fit the images (they follow get_camera_params: the sensor
        resolution); utils.render_K is the matrix that does.

        frame: "camera" -- the optical frame, x right, y down, z forward (OpenCV / ROS), of the image as rendered (for the d435i:
        the sideways image, before get_camera_data turns it); "world"; or "base" -- the simulated base_link body frame, as
        get_link_pose("base_link", simulated=True) places it.  stride = s keeps the pixels (s j, s i): H' = ceil(H / s),
        W' = ceil(W / s).  Pixels without a depth (0: beyond the camera's depth_limit) are NaN rows.
        render=True renders the depth first, into the image pull_camera_data() uses and with the camera's depth_limit;
        render=False deprojects the image of the last pull_camera_data() / pull_point_cloud().
        auto_rotate=True turns the GRID as get_camera_data turns the image (rot90(-1) over the grid axes for the d435i): a view,
        the xyz values are untouched.  The tensor is simulator-owned and overwritten by the next call with the same (camera, stride)."""
        if not isinstance(camera, StretchCameras) or not camera.is_depth or camera not in self._cameras:
            raise ValueError(f"{camera} is not a depth camera of cameras_to_use")
        fr, offset = self._frame_id(frame, ("camera", "world", "base"))
        stride = int(stride)
        if stride < 1:
            raise ValueError("stride must be >= 1")
        st = camera.initial_camera_settings
        img = self._depth_image(camera, render)
        pts = self._cached(self._points, (camera, stride), lambda: torch.zeros(
            self.num_envs, -(-st.height // stride), -(-st.width // stride), 3, dtype=torch.float32, device=self.device))
        rc = self._L.smj_depth_to_points(self._ctx, *self._camera_args(camera), ctypes.c_void_p(img.data_ptr()), stride, fr,
                                         ctypes.c_void_p(pts.data_ptr()), self._stream())
        _lib.check(self._L, self._ctx, rc, "smj_depth_to_points")
        if offset is not None:
            # base_link welded into a larger fused body (no shipped model does this): the constant link pose in that body, applied
            # exactly -- p_link = R_l' (p_body - r_l) -- as a second pass over the cloud; NaN rows stay NaN
            torch.matmul(pts - offset[0], offset[1], out=pts)
        if auto_rotate and camera == StretchCameras.cam_d435i_depth:
            return torch.rot90(pts, -1, (1, 2))
        return pts

    @_require_connection
    def pull_height_map(self, cameras: Optional[Sequence[StretchCameras]] = None, frame: str = "base", origin=(-1.6, -1.6),
                        cell: float = 0.05, shape=(64, 64), z_range=(-float("inf"), float("inf")), stride: int = 1,
                        render: bool = True) -> StatusStretchHeightMap:
        """Egocentric 2.5-D grid around the robot, fused over depth cameras in one HIP pass per camera (smj_depth_to_heightmap,
        include/smj_heightmap.h): per cell the largest z of the points that fall into it with z_range[0] <= z <= z_range[1]
        (`height`, NaN where there is none) and their number (`count`).  New, without a reference counterpart.

        cameras: depth cameras of cameras_to_use; None means all of them.  The first camera overwrites the map, the others
        accumulate into it; max and count do not depend on the order.  frame: "base" (the simulated base_link body frame), "world"
        or "camera" (the optical frame of each camera: meaningful for one camera).  Cell (iy, ix) covers origin + [ix, ix + 1) cell
        in x and origin + [iy, iy + 1) cell in y; shape = (ny, nx), ny nx <= 65536.  stride = s keeps the pixels (s j, s i).
        render as in pull_point_cloud: True renders each camera's depth first (with its depth_limit), False uses the image of the
        last pull_camera_data() / pull_point_cloud() / pull_height_map().
        The map includes the robot's own arm and gripper where a camera sees them: there is no self-filter.
        The tensors are simulator-owned and overwritten by the next call with the same (frame, shape)."""
        depth_cams = [c for c in self._cameras if c.is_depth]
        cams = depth_cams if cameras is None else ([cameras] if isinstance(cameras, StretchCameras) else list(cameras))
        if not cams:
            raise ValueError("no depth camera in cameras_to_use")
        for c in cams:
            if not isinstance(c, StretchCameras) or c not in depth_cams:
                raise ValueError(f"{c} is not a depth camera of cameras_to_use")
        fr, offset = self._frame_id(frame, ("camera", "world", "base"))
        ny, nx, x0, y0, cell, lo, hi = self._grid_args(shape, origin, cell, z_range, "z_range = (lo, hi)")
        if not lo <= hi:
            raise ValueError("z_range: lo <= hi, neither NaN")
        stride = int(stride)
        if stride < 1:
            raise ValueError("stride must be >= 1")
        if offset is not None:
            raise ValueError('frame "base": base_link sits at a non-identity fixed pose inside its fused body; a binned map cannot be '
                             'corrected afterwards (use frame="world", or pull_point_cloud)')
        if not render:   # every camera, before anything is allocated or launched
            for c in cams:
                self._depth_image(c, False)
        bufs = self._cached(self._hmaps, (frame, (ny, nx)), lambda: (
            torch.full((self.num_envs, ny, nx), float("nan"), dtype=torch.float32, device=self.device),
            torch.zeros(self.num_envs, ny, nx, dtype=torch.int32, device=self.device)))
        for k, c in enumerate(cams):
            img = self._depth_image(c, render)
            rc = self._L.smj_depth_to_heightmap(self._ctx, *self._camera_args(c), ctypes.c_void_p(img.data_ptr()), stride, fr,
                                                x0, y0, cell, nx, ny, lo, hi, int(k > 0), ctypes.c_void_p(bufs[0].data_ptr()),
                                                ctypes.c_void_p(bufs[1].data_ptr()), self._stream())
            _lib.check(self._L, self._ctx, rc, "smj_depth_to_heightmap")
        return StatusStretchHeightMap(time=self._time(), height=bufs[0], count=bufs[1], origin=(x0, y0),
                                      cell=cell, frame=frame)

    @_require_connection
    def pull_occupancy_grid(self, frame: str = "base", origin=(-3.2, -3.2), cell: float = 0.05, shape=(128, 128),
                            range_limits=(0.2, 5.0), no_return_clears: bool = True, accumulate: bool = False) -> StatusStretchOccupancyGrid:
        """Ray-traced 2-D occupancy counts around the robot from the lidar scan of the last step, in one HIP pass
        (smj_lidar_to_occupancy, include/smj_occupancy.h): per cell the rays that end in it on something (`hit`) and the rays
        that pass through it (`miss`); a cell with neither was not seen.  New, without a reference counterpart: the reference's
        examples/laser_scan.py turns the ranges into x/y points and stops there.

        frame: "base" (the simulated base_link body frame) or "world".  Cell (iy, ix) covers origin + [ix, ix + 1) cell in x and
        origin + [iy, iy + 1) cell in y; shape = (ny, nx), ny nx <= 65536.  range_limits = (r_min, r_max), the bounds laser_scan.py
        filters by: a range below r_min is the robot itself and is dropped, one in [r_min, r_max] is a return, one above r_max or
        -1 (nothing hit) is no return -- with no_return_clears such a ray is free over r_max, without it the ray is dropped.
        r_max / cell <= 8192.  accumulate=True adds to the buffers instead of overwriting them: in the world frame that maps across
        steps.  Needs StretchSensors.base_lidar in sensors_to_use.
        The tensors are simulator-owned and overwritten (or added to) by the next call with the same (frame, shape)."""
        self._need_lidar()
        fr, offset = self._frame_id(frame, ("world", "base"))
        ny, nx, x0, y0, cell, r_min, r_max = self._grid_args(shape, origin, cell, range_limits, "range_limits = (r_min, r_max)")
        _check_range_limits(r_min, r_max, cell)
        if offset is not None:
            raise ValueError('frame "base": base_link sits at a non-identity fixed pose inside its fused body; a binned grid cannot be '
                             'corrected afterwards (use frame="world")')
        bufs = self._cached(self._occ, (frame, (ny, nx)), lambda: (
            torch.zeros(self.num_envs, ny, nx, dtype=torch.int32, device=self.device),
            torch.zeros(self.num_envs, ny, nx, dtype=torch.int32, device=self.device)))
        rc = self._L.smj_lidar_to_occupancy(self._ctx, ctypes.c_void_p(self.lidar.data_ptr()), self.num_envs, fr, x0, y0, cell, nx, ny,
                                            r_min, r_max, int(bool(no_return_clears)), int(bool(accumulate)),
                                            ctypes.c_void_p(bufs[0].data_ptr()), ctypes.c_void_p(bufs[1].data_ptr()), self._stream())
        _lib.check(self._L, self._ctx, rc, "smj_lidar_to_occupancy")
        return StatusStretchOccupancyGrid(time=self._time(), hit=bufs[0], miss=bufs[1], origin=(x0, y0),
                                          cell=cell, frame=frame)

    @_require_connection
    def pull_distance_field(self, grid=None, *, min_hits: int = 1, unknown_is_obstacle: bool = False, max_distance=None,
                            nearest: bool = False, cell=None, origin=None, **occupancy_kwargs) -> StatusStretchDistanceField:
        """Exact Euclidean distance field of an occupancy grid in one HIP pass (smj_occupancy_to_distance, include/smj_distance.h):
        per cell the squared distance in cells to the nearest obstacle cell (`dist2`) and, with nearest=True, that obstacle's linear
        index, the smallest one among equally near obstacles.  Integers only: two calls give identical tensors.  New, without a
        reference counterpart; StatusStretchDistanceField turns it into metres and an inflated costmap.

        grid: None -- pull_occupancy_grid(**occupancy_kwargs) is called and transformed; a StatusStretchOccupancyGrid (a
        world-frame map accumulated over steps, say), whose frame, origin and cell are taken over; or a bool / integer tensor
        [B, ny, nx] of obstacles, e.g. pull_distance_field(hm.height > 0.10, cell=hm.cell, origin=hm.origin) -- then cell and origin
        are these keywords (1.0 and (0, 0) if absent), min_hits is 1 and there is no miss layer.
        A cell is an obstacle when hit >= min_hits, or, with unknown_is_obstacle, when no ray has seen it (hit == miss == 0).
        max_distance (metres) bounds the search at R = ceil(max_distance / cell) cells: a cell further than R cells from every
        obstacle gets StatusStretchDistanceField.NONE and -1, like every cell of a grid without obstacles.  None: no bound.
        The tensors are simulator-owned and overwritten by the next call with the same shape."""
        min_hits = int(min_hits)
        if min_hits < 1:
            raise ValueError("min_hits must be >= 1")
        miss = None
        self._upstream_kwargs(occupancy_kwargs, ("pull_occupancy_grid", "grid"), grid is None, cell, origin)
        if grid is None:
            grid = self.pull_occupancy_grid(**occupancy_kwargs)
            cell = origin = None
        if isinstance(grid, StatusStretchOccupancyGrid):
            x0y0, cell = self._origin_cell(grid, origin, cell)
            hit, miss, frame = grid.hit, grid.miss, grid.frame
        else:
            if not isinstance(grid, torch.Tensor) or grid.dtype not in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
                raise ValueError("grid: None, a StatusStretchOccupancyGrid, or a bool / integer tensor [B, ny, nx]")
            if min_hits != 1 or unknown_is_obstacle:
                raise ValueError("a mask has no counts and no miss layer: min_hits = 1, unknown_is_obstacle = False")
            x0y0, cell = self._origin_cell(None, origin, cell)
            hit, frame = (grid != 0).to(device=self.device, dtype=torch.int32).contiguous(), "grid"
        for t in (hit, miss):
            if t is not None and (t.dim() != 3 or t.shape[0] != self.num_envs or t.dtype != torch.int32 or not t.is_contiguous()
                                  or t.device != self.device or (miss is not None and t.shape != hit.shape)):
                raise ValueError(f"grid: contiguous int32 [num_envs = {self.num_envs}, ny, nx] on {self.device}")
        ny, nx = int(hit.shape[1]), int(hit.shape[2])
        self._check_cell_count("grid", ny, nx)
        if unknown_is_obstacle and miss is None:
            raise ValueError("unknown_is_obstacle needs a miss layer")
        R = 0
        if max_distance is not None:
            max_distance = float(max_distance)
            if not (np.isfinite(max_distance) and max_distance > 0):
                raise ValueError("max_distance: metres, finite and > 0 (None = no bound)")
            R = int(min(math.ceil(max_distance / cell), 8192))   # beyond the longest diagonal every bound is none
        bufs, near = self._cached_int_pair(self._dist, (ny, nx), ny, nx, nearest)
        rc = self._L.smj_occupancy_to_distance(self._ctx, ctypes.c_void_p(hit.data_ptr()), ctypes.c_void_p(miss.data_ptr()) if miss is not None else None,
                                               nx, ny, min_hits, int(bool(unknown_is_obstacle)), R, ctypes.c_void_p(bufs[0].data_ptr()),
                                               ctypes.c_void_p(near.data_ptr()) if near is not None else None, self._stream())
        _lib.check(self._L, self._ctx, rc, "smj_occupancy_to_distance")
        return StatusStretchDistanceField(time=self._time(), dist2=bufs[0], nearest=near, origin=x0y0, cell=cell,
                                          frame=frame)

    @_require_connection
    def pull_navigation_field(self, goal, cost=None, *, lethal: int = 253, neutral: int = 50, next: bool = False,
                              inscribed_radius: float = 0.17, inflation_radius: float = 0.56, cost_scaling_factor: float = 10.0,
                              cell=None, origin=None, **distance_kwargs) -> StatusStretchNavigationField:
        """Exact cost-to-goal field (navigation function) of a costmap in one HIP pass (smj_costmap_to_navigation,
        include/smj_navigation.h): per cell the cheapest path cost to a goal (`potential`) and, with next=True, the neighbour to
        step to, the smallest linear index among equally good ones.  Integers only: two calls give identical tensors.  New, without
        a reference counterpart; StatusStretchNavigationField turns it into metres, headings and paths.

        goal, in metres in the grid's frame: (x, y) for every env, a tensor [B, 2], or [B, G, 2] with G <= 64; turned into cell
        indices on the device (floor((g - origin) / cell); a goal outside the grid or not finite is unused).  An int tensor [B] or
        [B, G] is taken as linear cell indices iy nx + ix directly (-1 = unused).  A goal on an impassable cell is skipped.
        cost: None -- pull_distance_field(max_distance=inflation_radius, **distance_kwargs) is called and inflated by
        .inflated_cost(inscribed_radius, inflation_radius, cost_scaling_factor); a StatusStretchDistanceField, inflated the same way,
        whose frame, origin and cell are taken over; or a uint8 tensor [B, ny, nx] used as it is -- then cell and origin are these
        keywords (1.0 and (0, 0) if absent) and the frame is "grid".
        A cell is passable iff cost < lethal (1 .. 256; the default 253 keeps inscribed, lethal and unknown cells out, the
        costmap convention) and weighs neutral + cost (neutral 1 .. 255).  An axial move between cells a, b costs
        5 (w(a) + w(b)), a diagonal one 7 (w(a) + w(b)) and must not cut the corner of an impassable cell.
        The tensors are simulator-owned and overwritten by the next call with the same (shape, G)."""
        lethal, neutral = int(lethal), int(neutral)
        if not 1 <= lethal <= 256:
            raise ValueError("lethal must be in [1, 256]")
        if not 1 <= neutral <= 255:
            raise ValueError("neutral must be in [1, 255]")
        B, dev = self.num_envs, self.device
        # the goal's form, before anything runs; metres become cells once the grid is known
        if isinstance(goal, torch.Tensor):
            g = goal.to(dev)
            if g.is_floating_point():
                if g.dim() == 2:
                    g = g.unsqueeze(1)
                if g.dim() != 3 or g.shape[0] != B or g.shape[2] != 2 or not 1 <= g.shape[1] <= 64:
                    raise ValueError(f"goal in metres: (x, y), a tensor [B = {B}, 2] or [B, G, 2] with 1 <= G <= 64")
            elif g.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
                if g.dim() == 1:
                    g = g.unsqueeze(1)
                if g.dim() != 2 or g.shape[0] != B or not 1 <= g.shape[1] <= 64:
                    raise ValueError(f"goal as cell indices: an int tensor [B = {B}] or [B, G] with 1 <= G <= 64")
            else:
                raise ValueError("goal: a float tensor of metres or an int tensor of cell indices")
        else:
            try:
                gx, gy = (float(v) for v in goal)
            except (TypeError, ValueError):
                raise ValueError(f"goal: (x, y) in metres, a tensor [B = {B}, 2] / [B, G, 2], or an int tensor [B] / [B, G]") from None
            g = torch.tensor([[[gx, gy]]], dtype=torch.float32, device=dev).expand(B, 1, 2)
        if cost is None or isinstance(cost, StatusStretchDistanceField):
            r_ins, r_inf, k = float(inscribed_radius), float(inflation_radius), float(cost_scaling_factor)
            if not (0 <= r_ins <= r_inf < float("inf")) or not r_inf > 0 or not k >= 0:
                raise ValueError("0 <= inscribed_radius <= inflation_radius, inflation_radius > 0, both finite; cost_scaling_factor >= 0")
        if cost is None and "max_distance" in distance_kwargs:
            raise ValueError("max_distance is the inflation_radius here")
        self._upstream_kwargs(distance_kwargs, ("pull_distance_field", "cost"), cost is None, cell, origin)
        if cost is None:
            cost = self.pull_distance_field(max_distance=r_inf, **distance_kwargs)
            cell = origin = None
        if isinstance(cost, StatusStretchDistanceField):
            df = cost
            x0y0, cell = self._origin_cell(df, origin, cell)
            frame = df.frame
            if df.dist2.dim() != 3 or df.dist2.shape[0] != B or df.dist2.device != dev:
                raise ValueError(f"cost: a distance field [num_envs = {B}, ny, nx] on {dev}")
            cost = df.inflated_cost(r_ins, r_inf, k)
        else:
            if not isinstance(cost, torch.Tensor) or cost.dtype != torch.uint8 or cost.dim() != 3 or cost.shape[0] != B:
                raise ValueError(f"cost: None, a StatusStretchDistanceField, or a uint8 tensor [num_envs = {B}, ny, nx]")
            x0y0, cell = self._origin_cell(None, origin, cell)
            frame = "grid"
        ny, nx = int(cost.shape[1]), int(cost.shape[2])
        self._check_cell_count("cost", ny, nx)
        cost = cost.to(device=dev).contiguous()
        G = int(g.shape[1])
        bufs, nxt = self._cached_int_pair(self._nav, (ny, nx, G), ny, nx, next, (G,))
        if g.is_floating_point():
            bufs[2].copy_(cells_of_points(g, x0y0, cell, ny, nx))
        else:
            g = g.to(torch.int64)
            bufs[2].copy_(torch.where((g >= 0) & (g < ny * nx), g, torch.full_like(g, -1)))
        rc = self._L.smj_costmap_to_navigation(self._ctx, ctypes.c_void_p(cost.data_ptr()), ctypes.c_void_p(bufs[2].data_ptr()), G, nx, ny,
                                               lethal, neutral, ctypes.c_void_p(bufs[0].data_ptr()),
                                               ctypes.c_void_p(nxt.data_ptr()) if nxt is not None else None, self._stream())
        _lib.check(self._L, self._ctx, rc, "smj_costmap_to_navigation")
        return StatusStretchNavigationField(time=self._time(), potential=bufs[0], next=nxt, goal=bufs[2], origin=x0y0, cell=cell,
                                            frame=frame, neutral=neutral)

    @_require_connection
    def pull_frontiers(self, grid=None, *, min_hits: int = 1, min_size: int = 4, max_regions: int = 16, cost=None, lethal: int = 253,
                       cell=None, origin=None, **occupancy_kwargs) -> StatusStretchFrontiers:
        """Frontier regions of an occupancy grid in one HIP pass (smj_occupancy_to_frontiers, include/smj_frontier.h): the free
        cells with an unseen 4-neighbour, grouped into 8-connected regions (`label`), and for the max_regions largest regions of at
        least min_size cells a goal cell each (`goal`: the region's cell nearest its centroid), their sizes and coordinate sums
        (`region`) and the totals (`count`).  Integers only: two calls give identical tensors.  New, without a reference
        counterpart.  fr.goal is the goal of pull_navigation_field(fr.goal, cost): exploration without leaving the device.

        grid: None -- pull_occupancy_grid(**occupancy_kwargs) is called; a StatusStretchOccupancyGrid (a world-frame map
        accumulated over steps, say), whose frame, origin and cell are taken over; or an int8 tensor [B, ny, nx] in the convention
        of occupancy() (> 0 occupied, 0 free, < 0 unknown) -- then cell and origin are these keywords (1.0 and (0, 0) if absent),
        min_hits is 1 and the frame is "grid".
        A cell is occupied when hit >= min_hits, else free when miss > 0, else unknown.
        cost: None or a uint8 tensor [B, ny, nx], e.g. the df.inflated_cost(..) handed to pull_navigation_field: a frontier cell
        must then have cost < lethal (1 .. 256), so that no goal lies where the robot does not fit.
        1 <= min_size, 1 <= max_regions <= 64.  The tensors are simulator-owned and overwritten by the next call with the same
        (shape, max_regions)."""
        min_hits, min_size, G, lethal = int(min_hits), int(min_size), int(max_regions), int(lethal)
        if min_hits < 1:
            raise ValueError("min_hits must be >= 1")
        if not 1 <= min_size < 1 << 31:
            raise ValueError("min_size must be >= 1")
        if not 1 <= G <= 64:
            raise ValueError("max_regions must be in [1, 64]")
        if not 1 <= lethal <= 256:
            raise ValueError("lethal must be in [1, 256]")
        B, dev = self.num_envs, self.device
        if cost is not None and (not isinstance(cost, torch.Tensor) or cost.dtype != torch.uint8 or cost.dim() != 3 or cost.shape[0] != B):
            raise ValueError(f"cost: None or a uint8 tensor [num_envs = {B}, ny, nx]")
        if grid is not None and not isinstance(grid, StatusStretchOccupancyGrid):
            if not isinstance(grid, torch.Tensor) or grid.dtype != torch.int8 or grid.dim() != 3 or grid.shape[0] != B:
                raise ValueError(f"grid: None, a StatusStretchOccupancyGrid, or an int8 tensor [num_envs = {B}, ny, nx] as occupancy() gives")
            if min_hits != 1:
                raise ValueError("an occupancy() tensor has no counts: min_hits = 1")
        self._upstream_kwargs(occupancy_kwargs, ("pull_occupancy_grid", "grid"), grid is None, cell, origin)
        if grid is None:
            grid = self.pull_occupancy_grid(**occupancy_kwargs)
            cell = origin = None
        states = None
        if isinstance(grid, StatusStretchOccupancyGrid):
            x0y0, cell = self._origin_cell(grid, origin, cell)
            hit, miss, frame = grid.hit, grid.miss, grid.frame
            for t in (hit, miss):
                if (not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[0] != B or t.dtype != torch.int32 or not t.is_contiguous()
                        or t.device != dev or t.shape != hit.shape):
                    raise ValueError(f"grid: contiguous int32 hit and miss [num_envs = {B}, ny, nx] on {dev}")
            ny, nx = int(hit.shape[1]), int(hit.shape[2])
        else:
            x0y0, cell = self._origin_cell(None, origin, cell)
            states, frame = grid, "grid"
            ny, nx = int(grid.shape[1]), int(grid.shape[2])
        self._check_cell_count("grid", ny, nx)
        if cost is not None and tuple(cost.shape) != (B, ny, nx):
            raise ValueError(f"cost: the grid's shape [{B}, {ny}, {nx}]")
        new = lambda *shape: torch.empty(B, *shape, dtype=torch.int32, device=dev)
        bufs = self._cached(self._front, (ny, nx, G), lambda: [new(ny, nx), new(G), new(G, 4), new(2), None, None])
        if states is not None:
            if bufs[4] is None:
                bufs[4], bufs[5] = new(ny, nx), new(ny, nx)
            states = states.to(dev)
            bufs[4].copy_(states > 0)
            bufs[5].copy_(states == 0)
            hit, miss = bufs[4], bufs[5]
        if cost is not None:
            cost = cost.to(device=dev).contiguous()
        rc = self._L.smj_occupancy_to_frontiers(self._ctx, vp(hit), vp(miss), vp(cost) if cost is not None else None, nx, ny, min_hits, lethal,
                                                min_size, G, vp(bufs[0]), vp(bufs[1]), vp(bufs[2]), vp(bufs[3]), self._stream())
        _lib.check(self._L, self._ctx, rc, "smj_occupancy_to_frontiers")
        return StatusStretchFrontiers(time=self._time(), goal=bufs[1], label=bufs[0], region=bufs[2], count=bufs[3], origin=x0y0, cell=cell,
                                      frame=frame)

    @_require_connection
    def pull_base_command(self, nav, cost=None, *, candidates=None, lethal: int = 253, goal_weight: int = 1, obstacle_weight: int = 20,
                          arrive_radius: float = 0.10, twist=None, max_accel=None, period=None, outside_is_free: bool = False, pose=None,
                          scores: bool = False, cells: bool = False) -> StatusStretchBaseCommand:
        """The base command that follows a navigation field, in one HIP pass (smj_navigation_to_velocity, include/smj_drive.h): a
        trajectory-rollout local planner.  Per env every candidate arc of a table is laid over the grid from the robot's pose; arcs
        that touch a cell with cost >= lethal (or leave the grid, unless outside_is_free), whose scoring point has no path to the
        goal, or that the base cannot reach from its current velocity are dropped; the rest are scored
        goal_weight * potential[scoring point] + obstacle_weight * (largest swept cost) + bias, and the smallest score wins, the
        smallest index among equal ones.  Everything after the points have their cells is integers: two calls give identical
        tensors.  cmd.v and cmd.w go into set_base_velocity as they are; nothing is read back to the host.  New, without a
        reference counterpart.

        nav: a StatusStretchNavigationField, whose frame, origin and cell are taken over.  cost: None (0 everywhere) or the uint8
        tensor [B, ny, nx] the field was planned on.  The pose: sim.base_pose for a "world" field, zero for a "base" one (the grid
        moves with the robot); pose= ([3, B] float: x, y, theta in the grid's frame) replaces either and is required for "grid".
        candidates: a utils.BaseCandidates (utils.arc_candidates(...)); None is arc_candidates() with its defaults.
        Status per env (cmd.status): 0 ok; 1 arrived -- potential at the robot's cell <= floor(arrive_radius / cell) * 10 * neutral,
        i.e. about arrive_radius of path left; 2 every candidate dropped; 3 the robot is off the grid.  v = w = 0 unless 0.
        max_accel = (a_v, a_w) with period [s]: only candidates within a_v * period, a_w * period of the current velocity are
        kept; that velocity is twist ([2, B] float) or, by default, the last one commanded through set_base_velocity.
        scores, cells: also return every candidate's score [B, K] and every point's cell [B, K, P].
        The weights: with neutral 50 a cell of path costs 500, so a swept cost of 252 trades against about ten cells of detour.
        The tensors are simulator-owned and overwritten by the next call with the same (K, P, shape)."""
        from .utils import BaseCandidates, arc_candidates

        B, dev = self.num_envs, self.device
        if not isinstance(nav, StatusStretchNavigationField):
            raise ValueError("nav: the StatusStretchNavigationField of pull_navigation_field()")
        pot = nav.potential
        if (not isinstance(pot, torch.Tensor) or pot.dim() != 3 or pot.shape[0] != B or pot.dtype != torch.int32 or not pot.is_contiguous()
                or pot.device != dev):
            raise ValueError(f"nav: a contiguous int32 potential [num_envs = {B}, ny, nx] on {dev}")
        ny, nx = int(pot.shape[1]), int(pot.shape[2])
        self._check_cell_count("nav", ny, nx)
        x0y0, cell = self._origin_cell(nav, None, None)
        if cost is not None and (not isinstance(cost, torch.Tensor) or cost.dtype != torch.uint8 or tuple(cost.shape) != (B, ny, nx)):
            raise ValueError(f"cost: None or a uint8 tensor of the field's shape [{B}, {ny}, {nx}]")
        lethal, goal_weight, obstacle_weight = int(lethal), int(goal_weight), int(obstacle_weight)
        if not 1 <= lethal <= 256:
            raise ValueError("lethal must be in [1, 256]")
        if not (0 <= goal_weight <= 65535 and 0 <= obstacle_weight <= 65535):
            raise ValueError("goal_weight and obstacle_weight must be in [0, 65535]")
        arrive_radius = float(arrive_radius)
        if not (np.isfinite(arrive_radius) and arrive_radius >= 0):
            raise ValueError("arrive_radius must be finite and >= 0")
        arrive = int(np.floor(arrive_radius / cell)) * 10 * int(nav.neutral)
        if not 0 <= arrive < _lib.NAV_NONE:
            raise ValueError("arrive_radius: more cells than a potential can hold")
        if candidates is not None and not isinstance(candidates, BaseCandidates):
            raise ValueError("candidates: None or the BaseCandidates of utils.arc_candidates()")
        if candidates is None:
            if self._drive_default is None:
                self._drive_default = arc_candidates(device=dev)
            candidates = self._drive_default
        command, points, bias = candidates
        if (not isinstance(command, torch.Tensor) or not isinstance(points, torch.Tensor) or command.dtype != torch.float32 or points.dtype != torch.float32
                or command.dim() != 2 or command.shape[1] != 2 or points.dim() != 3 or points.shape[0] != command.shape[0] or points.shape[2] != 2):
            raise ValueError("candidates: command fp32 [K, 2] and points fp32 [K, P, 2]")
        K, P = int(points.shape[0]), int(points.shape[1])
        if not (1 <= K <= 1024 and 1 <= P <= 256 and K * P <= 32768):
            raise ValueError("candidates: 1 <= K <= 1024, 1 <= P <= 256 and K P <= 32768")
        if bias is not None and (not isinstance(bias, torch.Tensor) or bias.dtype != torch.int32 or tuple(bias.shape) != (K,)):
            raise ValueError(f"candidates: bias None or int32 [K = {K}]")
        if nav.frame not in ("world", "base", "grid"):
            raise ValueError('nav.frame must be "world", "base" or "grid"')
        if pose is None and nav.frame == "grid":
            raise ValueError('a "grid" field has no pose of its own: pose = [3, B] (x, y, theta in the grid\'s frame)')
        if pose is not None and (not isinstance(pose, torch.Tensor) or not pose.is_floating_point() or tuple(pose.shape) != (3, B)):
            raise ValueError(f"pose: a float tensor [3, num_envs = {B}]")
        max_dv = max_dw = float("inf")
        if max_accel is None:
            if twist is not None or period is not None:
                raise ValueError("twist and period belong to the dynamic window: give max_accel = (a_v, a_w) and period")
        else:
            try:
                a_v, a_w = (float(q) for q in max_accel)
                period = float(period)
            except (TypeError, ValueError):
                raise ValueError("max_accel = (a_v, a_w) with period in seconds") from None
            if not (a_v >= 0 and a_w >= 0 and np.isfinite(period) and period > 0):
                raise ValueError("max_accel >= 0, period > 0 and finite")
            max_dv, max_dw = a_v * period, a_w * period
            if twist is not None and (not isinstance(twist, torch.Tensor) or not twist.is_floating_point() or tuple(twist.shape) != (2, B)):
                raise ValueError(f"twist: None or a float tensor [2, num_envs = {B}]")
        new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=dev)
        bufs = self._cached(self._drive, (K, P, ny, nx), lambda: dict(cmd=new(torch.float32, 2, B), best=new(torch.int32, B, 2), score=None, cells=None,
                                                                       twist=None, pose=None))
        if scores and bufs["score"] is None:
            bufs["score"] = new(torch.int64, B, K)
        if cells and bufs["cells"] is None:
            bufs["cells"] = new(torch.int32, B, K, P)
        if pose is not None or nav.frame == "base":
            if bufs["pose"] is None:
                bufs["pose"] = torch.zeros(3, B, dtype=torch.float32, device=dev)
            if pose is not None:
                bufs["pose"].copy_(pose)
            else:
                bufs["pose"].zero_()
            pose_t = bufs["pose"]
        else:
            pose_t = self.base_pose
        twist_t = None
        if max_accel is not None:
            if bufs["twist"] is None:
                bufs["twist"] = new(torch.float32, 2, B)
            twist_t = bufs["twist"]
            if twist is not None:
                twist_t.copy_(twist)
            else:
                twist_t[0].copy_(self.glue.bv_v)
                twist_t[1].copy_(self.glue.bv_w)
        if cost is not None:
            cost = cost.to(device=dev).contiguous()
        command, points = command.to(dev).contiguous(), points.to(dev).contiguous()
        bias = bias.to(dev).contiguous() if bias is not None else None
        score_t, cells_t = (bufs["score"] if scores else None), (bufs["cells"] if cells else None)
        rc = self._L.smj_navigation_to_velocity(self._ctx, vp(pose_t), vp(twist_t), vp(cost), vp(pot), nx, ny, x0y0[0], x0y0[1], cell, vp(command), vp(points),
                                                vp(bias), K, P, lethal, int(bool(outside_is_free)), goal_weight, obstacle_weight, arrive, max_dv, max_dw,
                                                vp(bufs["cmd"]), vp(bufs["best"]), vp(score_t), vp(cells_t), self._stream())
        _lib.check(self._L, self._ctx, rc, "smj_navigation_to_velocity")
        return StatusStretchBaseCommand(time=self._time(), cmd=bufs["cmd"], best=bufs["best"], score=score_t, cells=cells_t, frame=nav.frame)

    def _match_field(self, field, sigma, origin, cell):
        """The field argument of pull_scan_match() and pull_particle_update(), checked: (field, grid, sigma, (x0, y0), cell, frame,
        ny, nx).  `grid` is the StatusStretchOccupancyGrid a field is still to be made of (then field is None); nothing is launched."""
        B, dev = self.num_envs, self.device
        grid = None
        if isinstance(field, (StatusStretchDistanceField, StatusStretchOccupancyGrid)):
            src = field.dist2 if isinstance(field, StatusStretchDistanceField) else field.hit
            if not isinstance(src, torch.Tensor) or src.dim() != 3 or src.shape[0] != B or src.dtype != torch.int32 or src.device != dev:
                raise ValueError(f"field: int32 tensors [num_envs = {B}, ny, nx] on {dev}")
            x0y0, cell = self._origin_cell(field, origin, cell)
            frame, (ny, nx) = field.frame, (int(v) for v in src.shape[1:])
            sigma = float(sigma)
            if not (0 < sigma < float("inf")):
                raise ValueError("sigma: metres, finite and > 0")
            if isinstance(field, StatusStretchOccupancyGrid):
                grid, field = field, None
        else:
            if not isinstance(field, torch.Tensor) or field.dtype != torch.uint8 or field.dim() != 3 or field.shape[0] != B:
                raise ValueError(f"field: a StatusStretchDistanceField, a StatusStretchOccupancyGrid, or a uint8 tensor [num_envs = {B}, ny, nx]")
            if origin is None or cell is None:
                raise ValueError("a bare field needs origin = (x0, y0) and cell")
            x0y0, cell = self._origin_cell(None, origin, cell)
            frame, (ny, nx) = "grid", (int(v) for v in field.shape[1:])
        if frame not in ("world", "grid"):
            raise ValueError('the field\'s frame must be "world" or "grid": a "base" grid moves with the robot and is no map')
        self._check_cell_count("field", ny, nx)
        return field, grid, sigma, x0y0, cell, frame, ny, nx

    def _match_field_tensor(self, field, grid, sigma):
        """The uint8 field on the device, after every ValueError has been raised: the distance field of `grid` and its likelihood
        where the caller handed in a map."""
        if grid is not None:
            field = self.pull_distance_field(grid)
        if isinstance(field, StatusStretchDistanceField):
            field = field.likelihood(sigma)
        return field.to(device=self.device).contiguous()

    @_require_connection
    def pull_scan_match(self, field, prior=None, *, sigma: float = 0.10, window=(0.5, 0.5), angles=None, range_limits=(0.2, 5.0),
                        min_points: int = 30, shift_weight: int = 0, scores: bool = False, cells: bool = False, origin=None,
                        cell=None) -> StatusStretchScanMatch:
        """Where in a map the lidar scan of the last step was taken, in one HIP pass (smj_scan_to_pose, include/smj_scanmatch.h): a
        correlative scan matcher.  Per env the scan's returns are laid over a likelihood field from every pose of a window round a
        prior -- the rotations of a table by whole-cell shifts -- and the pose under which they collect the largest sum wins, the
        smallest index among equal sums.  Everything after the points have their cells is integers: two calls give identical
        tensors.  match.pose goes into pull_base_command(pose=...) as it is; nothing is read back to the host.  New, without a
        reference counterpart: it stands where a user of the real robot runs AMCL or slam_toolbox.

        field: a StatusStretchDistanceField (of a world-frame map, say), whose likelihood(sigma) is matched against and whose frame,
        origin and cell are taken over; a StatusStretchOccupancyGrid, which goes through pull_distance_field() first (and so
        overwrites that call's tensors); or a uint8 tensor [B, ny, nx], the reward of a point per cell, with origin= and cell=.
        The frame is "world" or "grid"; a "base" grid moves with the robot and is no map (ValueError).
        prior: [3, B] float (x, y, theta in the field's frame); None is sim.base_pose, the simulator's own.
        window = (metres in x, metres in y) searched on either side of the prior, in whole cells: round(window / cell) <= 32 each.
        angles: a utils.ScanAngles (utils.scan_angles(...)); None is scan_angles() with its defaults, 21 rotations.
        range_limits = (r_min, r_max) as in pull_occupancy_grid: only ranges inside count.  Status per env (match.status): 0 ok;
        1 fewer than min_points returns; 2 the prior is not finite.  The pose is the prior unless 0.
        shift_weight: taken from a candidate's sum per squared cell of shift (0 .. 1024), to prefer the prior among near-equal poses.
        scores, cells: also return every candidate's score [B, T, 2 wy + 1, 2 wx + 1] (refined() needs it) and every ray's cell.
        Needs StretchSensors.base_lidar in sensors_to_use.
        The tensors are simulator-owned and overwritten by the next call with the same (T, window, shape)."""
        from .utils import ScanAngles, scan_angles

        B, dev = self.num_envs, self.device
        self._need_scan("smj_scan_to_pose")
        field, grid, sigma, x0y0, cell, frame, ny, nx = self._match_field(field, sigma, origin, cell)
        try:
            r_min, r_max = (float(v) for v in range_limits)
            wx, wy = (int(round(float(v) / cell)) for v in window)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("range_limits = (r_min, r_max), window = (metres in x, metres in y)") from None
        _check_range_limits(r_min, r_max, cell)
        if not (0 <= wx <= 32 and 0 <= wy <= 32):
            raise ValueError("window: 0 <= round(window / cell) <= 32 cells on either side")
        min_points, shift_weight = int(min_points), int(shift_weight)
        if not 1 <= min_points <= 1024:
            raise ValueError("min_points must be in [1, 1024]")
        if not 0 <= shift_weight <= 1024:
            raise ValueError("shift_weight must be in [0, 1024]")
        if angles is not None and not isinstance(angles, ScanAngles):
            raise ValueError("angles: None or the ScanAngles of utils.scan_angles()")
        if angles is None:
            if self._match_default is None:
                self._match_default = scan_angles(device=dev)
            angles = self._match_default
        ang, bias = angles
        if not isinstance(ang, torch.Tensor) or ang.dtype != torch.float32 or ang.dim() != 1 or not 1 <= ang.shape[0] <= 64:
            raise ValueError("angles: fp32 [T], 1 <= T <= 64")
        T = int(ang.shape[0])
        if bias is not None and (not isinstance(bias, torch.Tensor) or bias.dtype != torch.int32 or tuple(bias.shape) != (T,)):
            raise ValueError(f"angles: bias None or int32 [T = {T}]")
        if prior is not None and (not isinstance(prior, torch.Tensor) or not prior.is_floating_point() or tuple(prior.shape) != (3, B)):
            raise ValueError(f"prior: None or a float tensor [3, num_envs = {B}]")
        body = self._robot_body("points")
        # every ValueError has been raised: from here on the device works
        field = self._match_field_tensor(field, grid, sigma)
        new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=dev)
        bufs = self._cached(self._match, (T, wx, wy, ny, nx), lambda: dict(pose=new(torch.float32, 3, B), best=new(torch.int32, B, 4), score=None,
                                                                            cells=None, prior=None))
        if scores and bufs["score"] is None:
            bufs["score"] = new(torch.int32, B, T, 2 * wy + 1, 2 * wx + 1)
        if cells and bufs["cells"] is None:
            bufs["cells"] = new(torch.int32, B, T, self.nlidar, 2)
        if prior is not None:
            if bufs["prior"] is None:
                bufs["prior"] = new(torch.float32, 3, B)
            bufs["prior"].copy_(prior)
            prior_t = bufs["prior"]
        else:
            prior_t = self.base_pose
        ang = ang.to(dev).contiguous()
        bias = bias.to(dev).contiguous() if bias is not None else None
        score_t, cells_t = (bufs["score"] if scores else None), (bufs["cells"] if cells else None)
        rc = self._L.smj_scan_to_pose(self._ctx, vp(self.lidar), B, body, r_min, r_max, vp(field), nx, ny, x0y0[0], x0y0[1], cell, vp(prior_t), vp(ang),
                                      vp(bias), T, wx, wy, shift_weight, min_points, vp(bufs["pose"]), vp(bufs["best"]), vp(score_t), vp(cells_t),
                                      self._stream())
        _lib.check(self._L, self._ctx, rc, "smj_scan_to_pose")
        return StatusStretchScanMatch(time=self._time(), pose=bufs["pose"], best=bufs["best"], score=score_t, cells=cells_t, angles=ang,
                                      window=(wx, wy), origin=x0y0, cell=cell, frame=frame, bias=bias, shift_weight=shift_weight)

    @_require_connection
    def pull_map_update(self, pose, grid=None, gate=None, *, origin=(-3.2, -3.2), cell: float = 0.05, shape=(128, 128), range_limits=(0.2, 5.0),
                        no_return_clears: bool = True, accumulate: bool = True, cells: bool = False) -> StatusStretchMapUpdate:
        """The lidar scan of the last step ray-traced into a map at a pose that is handed in, in one HIP pass (smj_scan_to_map,
        include/smj_mapping.h): what pull_occupancy_grid(frame="world", accumulate=True) does with the simulator's own pose, done with
        the pose an estimator believes in.  With pull_scan_match() before it and pull_distance_field() after it this closes the loop
        -- match, integrate, distance field, match again -- per env on the device, nothing read back.  Integer sums: two calls give
        identical tensors.  New, without a reference counterpart: it stands where a user of the real robot runs slam_toolbox.

        pose: float [3, B] on the device (x, y, theta in the map's frame); match.pose goes in as it is.
        grid: a StatusStretchOccupancyGrid to add into -- its tensors, origin, cell and frame are taken over (origin, cell and shape
        of this call are not looked at); the first scan may have been mapped by pull_occupancy_grid(frame="world"), say.  A "base"
        grid moves with the robot and is no map (ValueError).  None: simulator-owned buffers of `shape` at origin and cell, zeroed
        when first used, in the frame "world".
        gate: None; an int32 [B] tensor on the device -- env e is integrated iff gate[e] == 0; or a StatusStretchScanMatch, whose
        status column is read where it lies (only envs whose match is ok are integrated).  An env whose pose is not finite is never
        integrated.  An env that is not integrated keeps its map (accumulate=True) or gets zeros (accumulate=False).
        range_limits, no_return_clears: as in pull_occupancy_grid.  cells: also return (ax, ay, bx, by) of every ray.
        update.grid goes into pull_distance_field(), pull_scan_match(), pull_frontiers() and pull_navigation_field() as it is.
        Needs StretchSensors.base_lidar in sensors_to_use.
        The tensors are simulator-owned and overwritten (the map: added to) by the next call with the same shape."""
        B, dev = self.num_envs, self.device
        self._need_scan("smj_scan_to_map")
        if not isinstance(pose, torch.Tensor) or not pose.is_floating_point() or tuple(pose.shape) != (3, B) or pose.device != dev:
            raise ValueError(f"pose: a float tensor [3, num_envs = {B}] on {dev}")
        if grid is None:
            ny, nx, x0, y0, cell, r_min, r_max = self._grid_args(shape, origin, cell, range_limits, "range_limits = (r_min, r_max)")
            frame, hit, miss = "world", None, None
        else:
            if not isinstance(grid, StatusStretchOccupancyGrid):
                raise ValueError("grid: None or a StatusStretchOccupancyGrid")
            (x0, y0), cell = self._origin_cell(grid, None, None)
            frame, hit, miss = grid.frame, grid.hit, grid.miss
            for t in (hit, miss):
                if t is not None and (not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[0] != B or t.dtype != torch.int32 or not t.is_contiguous()
                                      or t.device != dev or (hit is not None and t.shape != hit.shape)):
                    raise ValueError(f"grid: contiguous int32 [num_envs = {B}, ny, nx] on {dev}")
            if hit is None:
                raise ValueError("grid: a map has a hit layer")
            ny, nx, x0, y0, cell, r_min, r_max = self._grid_args(hit.shape[1:], (x0, y0), cell, range_limits, "range_limits = (r_min, r_max)")
        if frame not in ("world", "grid"):
            raise ValueError('the grid\'s frame must be "world" or "grid": a "base" grid moves with the robot and is no map')
        _check_range_limits(r_min, r_max, cell)
        gate_t, gate_at, gate_ld = None, None, 1
        if isinstance(gate, StatusStretchScanMatch):
            gate_t = gate.best
            if not isinstance(gate_t, torch.Tensor) or gate_t.dtype != torch.int32 or tuple(gate_t.shape) != (B, 4) or not gate_t.is_contiguous() or gate_t.device != dev:
                raise ValueError(f"gate: the match's best must be a contiguous int32 [num_envs = {B}, 4] on {dev}")
            gate_at, gate_ld = gate_t.data_ptr() + 12, 4      # the status column, where it lies
        elif gate is not None:
            if not isinstance(gate, torch.Tensor) or gate.dtype != torch.int32 or tuple(gate.shape) != (B,) or gate.device != dev or (B > 1 and gate.stride(0) < 1):
                raise ValueError(f"gate: None, an int32 tensor [num_envs = {B}] on {dev}, or a StatusStretchScanMatch")
            gate_t, gate_at, gate_ld = gate, gate.data_ptr(), max(int(gate.stride(0)), 1)
        body = self._robot_body("rays")
        # every ValueError has been raised: from here on the device works
        new = lambda *shape: torch.empty(B, *shape, dtype=torch.int32, device=dev)
        bufs = self._cached(self._maps, (ny, nx), lambda: dict(hit=None, miss=None, info=new(4), cells=None))
        if grid is None:
            if bufs["hit"] is None:
                bufs["hit"], bufs["miss"] = torch.zeros(B, ny, nx, dtype=torch.int32, device=dev), torch.zeros(B, ny, nx, dtype=torch.int32, device=dev)
            hit, miss = bufs["hit"], bufs["miss"]
        if cells and bufs["cells"] is None:
            bufs["cells"] = new(self.nlidar, 4)
        cells_t = bufs["cells"] if cells else None
        pose_t = pose if pose.dtype == torch.float32 and pose.is_contiguous() else pose.to(torch.float32).contiguous()
        rc = self._L.smj_scan_to_map(self._ctx, vp(self.lidar), B, body, r_min, r_max, vp(pose_t), ctypes.c_void_p(gate_at) if gate_at is not None else None, gate_ld,
                                     x0, y0, cell, nx, ny, int(bool(no_return_clears)), int(bool(accumulate)), vp(hit), vp(miss), vp(bufs["info"]), vp(cells_t),
                                     self._stream())
        _lib.check(self._L, self._ctx, rc, "smj_scan_to_map")
        out = StatusStretchOccupancyGrid(time=self._time(), hit=hit, miss=miss, origin=(x0, y0), cell=cell, frame=frame)
        return StatusStretchMapUpdate(time=out.time, grid=out, info=bufs["info"], cells=cells_t)

    @_require_connection
    def pull_particle_update(self, field, particles, noise=None, draw=None, span: int = 4096, min_points: int = 30, resample: bool = True,
                             range_limits=(0.2, 5.0), ancestors: bool = False, origin=None, cell=None, *, sigma: float = 0.10) -> StatusStretchParticles:
        """One measurement update of a particle filter for every env, in one HIP pass (smj_scan_to_particles, include/smj_localize.h):
        Monte Carlo localisation.  Per env P pose hypotheses -- anywhere on the map, each with its own heading, no lattice -- are
        weighted by the sum S of a likelihood field under the returns of the lidar scan of the last step, laid out from the particle,
        and resampled (systematic resampling, one random word per env) by w = max(S - cut, 0), cut = max(S_max - span, 0).  Where
        pull_scan_match() searches +-0.5 m and +-5 degrees round one prior, this finds a robot whose pose is unknown by metres; its
        best particle is then the prior the matcher refines to the cell.  Everything after the weights is integers: two calls give
        identical tensors.  Nothing is read back to the host.  New, without a reference counterpart: it stands where a user of the
        real robot runs AMCL.

        field: as pull_scan_match() takes it -- a StatusStretchDistanceField, whose likelihood(sigma) is used and whose frame, origin
        and cell are taken over; a StatusStretchOccupancyGrid, which goes through pull_distance_field() first; or a uint8 tensor
        [B, ny, nx] with origin= and cell=.
        particles: float [3, B, P] on the device, rows x, y, theta in the field's frame, 1 <= P <= 4096 (utils.spread_particles for
        a first set; update.particles, or update.predict(odometry) when the robot has moved, for the next call).  A particle that is
        not finite weighs nothing and dies out.
        noise: None or float [3, B, P], added to the resampled particles (utils.particle_noise): without it the set collapses onto
        copies of few ancestors.
        draw: None or an integer tensor [B] on the device, one random word in [0, 2^32) per env (int32 is read as its bits); None
        draws them from a torch.Generator the simulator owns, on the device.
        span: how far below the best S a particle still gets weight, in units of the field (255 per return on an obstacle);
        1 .. 2^18.  A small span concentrates faster, a large one keeps more hypotheses.
        Status per env (update.status): 0 ok; 1 fewer than min_points returns; 2 lost -- no particle puts a return on a rewarded
        cell.  Unless 0 (and with resample=False) the particles come back as they went in and update.pose is NaN.
        ancestors: also return the input particle every slot was drawn from.
        Needs StretchSensors.base_lidar in sensors_to_use.
        The tensors are simulator-owned; update.particles is overwritten by the call after the next one with the same (P, shape)
        (two sets take turns, so that it can go straight into the next call), the others by the next call."""
        B, dev = self.num_envs, self.device
        self._need_scan("smj_scan_to_particles")
        field, grid, sigma, x0y0, cell, frame, ny, nx = self._match_field(field, sigma, origin, cell)
        try:
            r_min, r_max = (float(v) for v in range_limits)
        except (TypeError, ValueError, OverflowError):
            raise ValueError("range_limits = (r_min, r_max)") from None
        _check_range_limits(r_min, r_max, cell)
        if (not isinstance(particles, torch.Tensor) or not particles.is_floating_point() or particles.dim() != 3 or particles.shape[0] != 3 or particles.shape[1] != B
                or not 1 <= particles.shape[2] <= 4096 or particles.device != dev):
            raise ValueError(f"particles: a float tensor [3, num_envs = {B}, P] on {dev}, 1 <= P <= 4096")
        P = int(particles.shape[2])
        if noise is not None and (not isinstance(noise, torch.Tensor) or not noise.is_floating_point() or tuple(noise.shape) != (3, B, P) or noise.device != dev):
            raise ValueError(f"noise: None or a float tensor [3, num_envs = {B}, P = {P}] on {dev}")
        if draw is not None and (not isinstance(draw, torch.Tensor) or draw.is_floating_point() or draw.dtype == torch.bool or tuple(draw.shape) != (B,) or draw.device != dev):
            raise ValueError(f"draw: None or an integer tensor [num_envs = {B}] on {dev}")
        span, min_points = int(span), int(min_points)
        if not 1 <= span <= 1 << 18:
            raise ValueError("span must be in [1, 2^18]")
        if not 1 <= min_points <= 1024:
            raise ValueError("min_points must be in [1, 1024]")
        body = self._robot_body("points")
        # every ValueError has been raised: from here on the device works
        field = self._match_field_tensor(field, grid, sigma)
        new = lambda dtype, *shape: torch.empty(*shape, dtype=dtype, device=dev)
        bufs = self._cached(self._particles, (P, ny, nx), lambda: dict(out=[new(torch.float32, 3, B, P), new(torch.float32, 3, B, P)], weights=new(torch.int32, B, P),
                                                                       ancestors=None, stat=new(torch.int32, B, 8), pose=new(torch.float32, 3, B),
                                                                       draw=new(torch.int32, B)))
        part_t = particles if particles.dtype == torch.float32 and particles.is_contiguous() else particles.to(torch.float32).contiguous()
        noise_t = None if noise is None else noise if noise.dtype == torch.float32 and noise.is_contiguous() else noise.to(torch.float32).contiguous()
        out = bufs["out"][1] if part_t.untyped_storage().data_ptr() == bufs["out"][0].untyped_storage().data_ptr() else bufs["out"][0]   # never the set that goes in
        if ancestors and bufs["ancestors"] is None:
            bufs["ancestors"] = new(torch.int32, B, P)
        anc_t = bufs["ancestors"] if ancestors else None
        if draw is None:
            if self._draw_generator is None:
                self._draw_generator = torch.Generator(device=dev)
                self._draw_generator.manual_seed(0x5EED)
            bufs["draw"].copy_(torch.randint(-(1 << 31), 1 << 31, (B,), dtype=torch.int64, device=dev, generator=self._draw_generator))   # the low 32 bits
        else:
            bufs["draw"].copy_(draw.to(torch.int64) & 0xFFFFFFFF if draw.dtype != torch.int32 else draw)   # int64 -> int32 keeps the low 32 bits
        rc = self._L.smj_scan_to_particles(self._ctx, vp(self.lidar), B, body, r_min, r_max, vp(field), nx, ny, x0y0[0], x0y0[1], cell, vp(part_t), P, vp(noise_t),
                                           vp(bufs["draw"]), span, min_points, int(bool(resample)), vp(out), vp(bufs["weights"]), vp(anc_t), vp(bufs["stat"]),
                                           vp(bufs["pose"]), self._stream())
        _lib.check(self._L, self._ctx, rc, "smj_scan_to_particles")
        return StatusStretchParticles(time=self._time(), particles=out, weights=bufs["weights"], ancestors=anc_t, stat=bufs["stat"], pose=bufs["pose"], prior=part_t,
                                      origin=x0y0, cell=cell, frame=frame)

    @_require_connection
    def pull_contact_data(self) -> StatusStretchContacts:
        """The contacts of every env's last physics step and their forces (MjData.contact + mj_contactForce after mj_step), as
        device tensors without a host synchronisation.  Stale after reset() until the next step().  Needs contacts=True."""
        if not self._contacts:
            raise _lib.SmjError("the contact readout is off: construct StretchBatchSimulator(..., contacts=True)")
        return StatusStretchContacts.from_records(self.contact_records, self.info[1], self._geom_body,
                                                  time=self._time())

    def _body_ids(self, bodies) -> torch.Tensor:
        """MJCF body name(s) -> their ids as a device tensor, cached per name set: a per-step query copies nothing to the device (a
        pageable host -> device copy would synchronise the stream)."""
        key = (bodies,) if isinstance(bodies, str) else tuple(bodies)
        ids = self._id_cache.get(key)
        if ids is None:
            names = self.names["body"]
            for b in key:
                if b not in names:
                    raise KeyError(b)
            ids = torch.tensor([names.index(b) for b in key], dtype=torch.int64).to(self.device)
            self._id_cache[key] = ids
        return ids

    @_require_connection
    def contact_force(self, body, other=None) -> torch.Tensor:
        """[B, 3] net world-frame contact force on the MJCF body (or bodies) `body` from `other` (body name(s); None: from
        everything), summed over the last step's contacts: + on geom2's body, - on geom1's."""
        return self.pull_contact_data().net_force(self._body_ids(body), None if other is None else self._body_ids(other))

    @_require_connection
    def in_contact(self, body, other=None) -> torch.Tensor:
        """[B] bool: a contact between `body` and `other` (None: anything) entered the constraint system at the last step."""
        return self.pull_contact_data().touching(self._body_ids(body), None if other is None else self._body_ids(other))

    @_require_connection
    def pull_joint_limits(self) -> dict:
        """{Actuators: (lo, hi)} from jnt_range, later joints of one actuator overwrite earlier (mujoco_server.py:281-291)."""
        out = {}
        for j, name in enumerate(self.names["joint"]):
            try:
                act = Actuators.get_actuator_by_joint_names_in_mjcf(name)
            except NotImplementedError:
                continue
            r = self.model["jnt_range"][j]
            out[act] = (float(r[0]), float(r[1]))
        return out

    @_require_connection
    def get_base_pose(self):
        s = self.pull_status()
        return (s.base.x, s.base.y, s.base.theta)

    # ------------------------------------------------------------------ wait helpers as batched predicates
    @_require_connection
    def get_link_pose(self, link_name: str, simulated: bool = False) -> torch.Tensor:
        """World pose [B, 4, 4] of a link (a body name of stretch.xml, e.g. "link_grasp_center").

        Default = the reference's semantics (stretch_mujoco_simulator.py:468-486): forward kinematics of the link relative to
        `base_link` at the STATUS joint positions -- lift, arm (a quarter of the extension on each of the four telescope
        joints, utils.py:209-212), wrist yaw / pitch / roll, head pan / tilt; every other joint (gripper, fingers) at zero --
        placed at the planar base pose Rz(theta), (x, y, 0).  The reference evaluates its URDF for this; the URDF is not in
        the checkout, the same kinematic chain is read from the compiled MJCF model (stretch.xml carries the URDF's link
        names and frames).  simulated=True returns the simulated body pose of the last physics step instead, base roll /
        pitch / height, finger and rubber-tip joints included."""
        names = self.names["body"]
        if link_name not in names:
            raise KeyError(link_name)
        i = names.index(link_name)
        fb = int(self.model["link_fused"][i])
        rp = torch.tensor(np.asarray(self.model["link_relpos"][i], np.float32), device=self.device)
        Rl = self._quat_mat(self.model["link_relquat"][i], self.device)
        B = self.num_envs
        T = torch.zeros(B, 4, 4, dtype=torch.float32, device=self.device)
        T[:, 3, 3] = 1.0
        if simulated:
            P = self.xpose[12 * fb: 12 * fb + 3].t()                       # [B, 3]
            Rb = self.xpose[12 * fb + 3: 12 * fb + 12].t().reshape(-1, 3, 3)
            T[:, :3, :3] = Rb @ Rl
            T[:, :3, 3] = P + (Rb @ rp)
            return T
        st = self.pull_status()
        q = {"joint_lift": st.lift.pos, "joint_wrist_yaw": st.wrist_yaw.pos, "joint_wrist_pitch": st.wrist_pitch.pos,
             "joint_wrist_roll": st.wrist_roll.pos, "joint_head_pan": st.head_pan.pos, "joint_head_tilt": st.head_tilt.pos}
        for k in range(4):
            q[f"joint_arm_l{k}"] = st.arm.pos / 4
        m = self.model
        base = self.names["body"].index("base_link")
        base = int(m["link_fused"][base])
        path, b = [], fb
        while b != base and b > 0:
            path.append(b)
            b = int(m["body_parentid"][b])
        if b != base:
            raise KeyError(f"{link_name} is not part of the robot")
        R = torch.eye(3, device=self.device).expand(B, 3, 3).clone()
        p = torch.zeros(B, 3, device=self.device)
        f32 = lambda a: torch.tensor(np.asarray(a, np.float32), device=self.device)
        for b in reversed(path):     # [MJ] mj_kinematics: body frame in the parent, then the body's joints about their anchors
            p = p + (R @ f32(m["body_pos"][b]))
            R = R @ self._quat_mat(m["body_quat"][b], self.device)
            for j in range(int(m["body_jntadr"][b]), int(m["body_jntadr"][b]) + int(m["body_jntnum"][b])):
                val = q.get(self.names["joint"][j])
                if val is None:
                    continue
                val = val.float() - float(m["qpos0"][int(m["jnt_qposadr"][j])])
                axis, jpos = f32(m["jnt_axis"][j]), f32(m["jnt_pos"][j])
                if int(m["jnt_type"][j]) == 2:       # slide
                    p = p + (R @ axis) * val.unsqueeze(1)
                else:                                 # hinge: rotate about the anchor
                    anchor = p + (R @ jpos)
                    R = R @ self._axis_angle_mat(axis, val)
                    p = anchor - (R @ jpos)
        x, y, th = st.base.x.float(), st.base.y.float(), st.base.theta.float()
        Rz = torch.zeros(B, 3, 3, device=self.device)
        Rz[:, 0, 0] = torch.cos(th); Rz[:, 0, 1] = -torch.sin(th); Rz[:, 1, 0] = torch.sin(th); Rz[:, 1, 1] = torch.cos(th); Rz[:, 2, 2] = 1.0
        Rw = Rz @ R
        pw = (Rz @ p.unsqueeze(2)).squeeze(2)
        pw[:, 0] += x; pw[:, 1] += y
        T[:, :3, :3] = Rw @ Rl
        T[:, :3, 3] = pw + (Rw @ rp)
        return T

    @staticmethod
    def _quat_mat(qt, device) -> torch.Tensor:
        w, x, y, z = [float(v) for v in np.asarray(qt)]
        return torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                             [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                             [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=torch.float32, device=device)

    @staticmethod
    def _axis_angle_mat(axis: torch.Tensor, ang: torch.Tensor) -> torch.Tensor:
        """Rotation matrices [B, 3, 3] about a fixed axis by per-env angles (Rodrigues)."""
        a = (axis / axis.norm()).tolist()
        K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float32, device=axis.device)
        s, c = torch.sin(ang).view(-1, 1, 1), torch.cos(ang).view(-1, 1, 1)
        return torch.eye(3, device=axis.device) + s * K + (1 - c) * (K @ K)

    @_require_connection
    def get_ee_pose(self) -> torch.Tensor:
        """stretch_mujoco_simulator.py:464-466"""
        return self.get_link_pose("link_grasp_center")

    @_require_connection
    def is_reached_set_position(self, actuator, position_tolerance: float = 0.05) -> torch.Tensor:
        """[B] bool: the joint is within `position_tolerance` of its last `move_to` target; envs whose command holds no
        move_to entry for the actuator count as reached (stretch_mujoco_simulator.py:235-265, which warns and returns
        True).  Base and wheel actuators are not supported, as in the reference."""
        if isinstance(actuator, str):
            actuator = Actuators[actuator]
        if actuator in (Actuators.base_rotate, Actuators.base_translate, Actuators.left_wheel_vel, Actuators.right_wheel_vel):
            raise NotImplementedError(f"Check joint reached is not supported for {actuator}.")
        from .enums import CTRL_INDEX

        i = CTRL_INDEX[actuator.name]
        cur = actuator.get_position(self.pull_status())
        target = self.glue.mt_val[i].to(cur.dtype)
        return (~self.glue.mt_has[i]) | ((cur - target).abs() <= position_tolerance)

    @_require_connection
    def wait_until_at_setpoint(self, actuator, timeout: float = 5.0, position_tolerance: float = 0.05) -> torch.Tensor:
        """Step until every env has reached the actuator's last move_to target or `timeout` SIM-seconds elapse; returns the
        [B] bool mask of envs that got there (stretch_mujoco_simulator.py:267-297: wall clock there, sim clock here)."""
        if isinstance(actuator, str):
            actuator = Actuators[actuator]
        budget = int(round(timeout / self.timestep))
        chunk = max(1, int(round(0.05 / self.timestep)))
        self.step(1)        # fold the pending command into ctrl before the first check
        done_steps = 1
        ok = self.is_reached_set_position(actuator, position_tolerance)
        while not bool(ok.all()) and done_steps < budget:
            self.step(chunk)
            done_steps += chunk
            ok = self.is_reached_set_position(actuator, position_tolerance)
        return ok

    @_require_connection
    def wait_while_is_moving(self, actuator, timeout: Optional[float] = 5.0, check_interval: float = 0.1,
                             position_tolerance: float = 0.0005) -> torch.Tensor:
        """Step until the actuator stops moving in every env (|dpos| <= tol over check_interval of SIM time) or
        `timeout` sim-seconds elapse.  Returns a [B] bool mask of envs that came to rest.
        Reference semantics: stretch_mujoco_simulator.py:299-358 (wall-clock there, sim-clock here)."""
        if isinstance(actuator, str):
            actuator = Actuators[actuator]
        chunk = max(1, int(round(check_interval / self.timestep)))
        budget = int(round((timeout if timeout is not None else 1e9) / self.timestep))

        def position():
            st = self.pull_status()
            if actuator in (Actuators.left_wheel_vel, Actuators.base_translate):
                return st.base.x
            if actuator == Actuators.right_wheel_vel:
                return st.base.y
            if actuator == Actuators.base_rotate:
                return st.base.theta
            return actuator.get_position(st)

        last = position()
        still = torch.zeros(self.num_envs, dtype=torch.bool, device=self.device)
        done_steps = 0
        while done_steps < budget:
            self.step(chunk)
            done_steps += chunk
            cur = position()
            still = (cur - last).abs() <= position_tolerance
            last = cur
            if bool(still.all()):
                break
        return still
