"""The scene the GPU tests of the perception entries share (tests/test_gpu_{point_cloud,height_map,occupancy,distance,navigation}.py):
stretch_scene, three envs driven apart, 200 steps.  Each test module keeps its own module-scoped fixture, which calls build() with
its cameras and sensors (lidar_rig() for the lidar's entries), adds what only it needs and stops the simulator after its yield;
bare_context() is the whole body of the `bare` fixtures.  scan_rig() is lidar_rig() with what the modules of the scan entries share
(tests/test_gpu_{scanmatch,mapping,localize}.py), which also import the `bare` fixture from here.  Below those: the small helpers of
the C calls, the guarded output buffers."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

B = 3
DEV = "cuda:0"
# per env: base x, y, yaw; lift; wrist pitch (down: the wrist camera sees the floor inside its 1 m limit); head pan
POSES = [(0.0, 0.0, 0.0, 0.6, -0.8, 0.0), (-0.3, 0.2, 0.5, 0.3, -0.6, -0.8), (-0.5, -0.3, -0.7, 0.45, -0.7, 0.6)]


def f32(v):
    return float(np.float32(v))


def to32(v):
    """fp64 of the fp32 value: the library rounds the model tables to fp32."""
    return np.asarray(v, np.float64).astype(np.float32).astype(np.float64)


class Rig:
    pass


def build(cameras=(), sensors=(), pose_arm_and_head=False):
    """The started simulator after 200 steps, with the host copies every module reads.  pose_arm_and_head: the arm, the wrist pitch
    and the head pan are set per env too (what the cameras look at); without it only the base pose and the lift differ."""
    from stretch_mujoco_amd import StretchBatchSimulator, lib
    from stretch_mujoco_amd.enums import StretchCameras

    sim = StretchBatchSimulator(num_envs=B, device="cuda:0", cameras_to_use=list(cameras), sensors_to_use=list(sensors), solver="newton",
                                scene="stretch_scene")
    sim.start(home=False)
    jn = {n: i for i, n in enumerate(sim.names["joint"])}
    an = {n: i for i, n in enumerate(sim.names["actuator"])}
    adr = sim.model["jnt_qposadr"]
    q = np.stack([np.asarray(sim.model["qpos0"], np.float64)] * B, 1)
    ctrl = np.zeros((sim.nu, B))
    for e, (x, y, yaw, lift, pitch, pan) in enumerate(POSES):
        q[0:2, e] = [x, y]
        q[3:7, e] = [np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]
        q[adr[jn["joint_lift"]], e] = lift
        ctrl[an["lift"], e] = lift
        if pose_arm_and_head:
            for k in range(4):
                q[adr[jn[f"joint_arm_l{k}"]], e] = 0.025
            q[adr[jn["joint_wrist_pitch"]], e] = pitch
            q[adr[jn["joint_head_pan"]], e] = pan
            ctrl[an["arm"], e], ctrl[an["wrist_pitch"], e], ctrl[an["head_pan"], e] = 0.1, pitch, pan
    sim.qpos[:] = torch.tensor(q, dtype=torch.float32, device=sim.device)
    sim.ctrl[:] = torch.tensor(ctrl, dtype=torch.float32, device=sim.device)
    sim.step(200)
    torch.cuda.synchronize()
    assert int((sim.info[3] & 4).max()) == 0, "an env was reset for a non-finite state"
    r = Rig()
    r.sim, r.L, r.lib, r.cams = sim, lib.load(), lib, StretchCameras
    r.xpose = sim.xpose.cpu().numpy().astype(np.float64)
    r.cam_names = sim.names["camera"]
    r.cam_pos = to32(sim.model["cam_pos"])
    r.cam_mat = to32(sim.model["k_cam_mat"])
    r.cam_bodyid = np.asarray(sim.model["cam_bodyid"]).reshape(-1)
    r.base = int(sim.model["link_fused"][sim.names["body"].index("base_link")])
    r.cache = {}
    return r


def lidar_rig():
    """The rig with the lidar on and no camera."""
    from stretch_mujoco_amd.enums import StretchSensors

    return build(sensors=[StretchSensors.base_lidar])


def scan_rig(nlidar):
    """lidar_rig() with the inputs of the scan entries: .geoms, per env (o, d, So, Sd) of the rays in the robot's frame, from the XPOSE
    array and the site tables; the synthetic scan of scanmatch_ref.float_stage_inputs on them (.scan_host, .pts, .mar) and its device
    copy .scan.  Computed once per module and left unchanged."""
    import occupancy_ref
    import scanmatch_ref
    from point_cloud_ref import body_pose

    r = lidar_rig()
    sim = r.sim
    assert sim.nlidar == nlidar
    sites = np.asarray(sim.model["sensor_lidar_site"]).reshape(-1)
    site_body = np.asarray(sim.model["site_bodyid"]).reshape(-1)[sites]
    site_pos = to32(np.asarray(sim.model["site_pos"]).reshape(-1, 3)[sites])
    lz = to32(np.asarray(sim.model["k_site_mat"]).reshape(-1, 3, 3)[sites][:, :, 2])
    poses = {b: body_pose(r.xpose, int(b)) for b in set(site_body.tolist()) | {r.base}}
    r.geoms = []
    for e in range(B):
        bp = np.stack([poses[int(b)][0][e] for b in site_body])
        bm = np.stack([poses[int(b)][1][e] for b in site_body])
        r.geoms.append(occupancy_ref.ray_geometry(bp, bm, site_pos, lz, poses[r.base][0][e], poses[r.base][1][e]))
    r.scan_host, r.pts, r.mar = scanmatch_ref.float_stage_inputs(r.geoms)
    r.scan = dev(r.scan_host)
    return r


def rig_scans(r, poses):
    """fp32 scans [K, B] cast in the room of scanmatch_ref along the scan rig's own rays from poses [B, 3]."""
    import scanmatch_ref

    return np.stack([scanmatch_ref.room_scan(poses[e], r.geoms[e][0], r.geoms[e][1]) for e in range(B)], 1).astype(np.float32)


def bare_context():
    """Fixture body: smj_create on the stretch_scene blob, B envs, NOTHING bound; .cache is the module's.  Destroyed at teardown."""
    from stretch_mujoco_amd import lib

    b = Rig()
    b.L, b.ctx, b.cache = lib.load(), ctypes.c_void_p(), {}
    with open(os.path.join(ROOT, "stretch_mujoco_amd", "models", "stretch_scene.smjb"), "rb") as f:
        blob = f.read()
    assert b.L.smj_create(blob, len(blob), B, 0, ctypes.byref(b.ctx)) == 0
    yield b
    torch.cuda.synchronize()
    b.L.smj_destroy(b.ctx)


@pytest.fixture(scope="module")
def bare():
    yield from bare_context()


def dev(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def same(tag, got, want):
    got = got.cpu().numpy()
    assert np.array_equal(got, want), (tag, int((got != want).sum()), np.argwhere(got != want)[:5].tolist())


def sentinels(ny, nx, fill=-7):
    """A pair of int32 outputs [B, ny, nx] full of a value no entry writes there."""
    return (torch.full((B, ny, nx), fill, dtype=torch.int32, device=DEV), torch.full((B, ny, nx), fill, dtype=torch.int32, device=DEV))


class Guarded:
    """An int32 output [B, ny, nx] as .view, `pad` words into a buffer of -12345 with 37 more behind it (pad 36: on a 16-byte boundary,
    37: four bytes past one); Guarded.of(pad, dtype, *shape) for an output of another type and shape.  check(): the guards are
    untouched and the view equals `want` (floats byte for byte, so a NaN equals itself and -0 is not +0)."""

    def __init__(self, pad, ny, nx, dtype=torch.int32, shape=None):
        shape = (B, ny, nx) if shape is None else shape
        self.pad, self.cells = pad, int(np.prod(shape))
        self.big = torch.full((pad + self.cells + 37,), -12345, dtype=dtype, device=DEV)
        self.view = self.big[pad:pad + self.cells].view(*shape)
        assert self.view.data_ptr() % 16 == (self.big.element_size() * pad) % 16

    @classmethod
    def of(cls, pad, dtype, *shape):
        return cls(pad, None, None, dtype, shape)

    def check(self, want):
        assert (self.big[:self.pad] == -12345).all() and (self.big[self.pad + self.cells:] == -12345).all()
        assert self.view.cpu().numpy().tobytes() == want.cpu().numpy().tobytes() if self.view.is_floating_point() else torch.equal(self.view, want)


def frame_id(r, frame):
    """The C entries' frame id; the fused body of base_link goes by "body" in the camera tests and by "base" in the lidar tests."""
    return {"camera": r.lib.FRAME_CAMERA, "world": r.lib.FRAME_WORLD, "body": r.base, "base": r.base}[frame]


def render(r, ci, W, H, fovy, limit):
    """(device image, host copy), rendered once per (camera, size, limit) and left unchanged."""
    key = ("img", ci, W, H, fovy, limit)
    if key not in r.cache:
        img = torch.zeros(B, H, W, dtype=torch.float32, device=r.sim.device)
        assert r.L.smj_render_depth(r.sim._ctx, ci, W, H, float(fovy), float(limit), ctypes.c_void_p(img.data_ptr()), r.sim._stream()) == 0
        torch.cuda.synchronize()
        r.cache[key] = (img, img.cpu().numpy())
    return r.cache[key]
