"""Cost of the organised point clouds (smj_depth_to_points) at 4096 envs in scene.xml: per depth camera and stride (1 and 4), world
frame, the time of (a) the new entry, (b) the depth render it follows, (c) a torch composition of the same arithmetic on the same
depth tensor (strided view, broadcast multiplies, einsum, add, mask -- written below).  Device events around `reps` back-to-back
calls after a warm-up of every shape; the three alternate round by round so that drift of the device affects them alike; the
median of the rounds is printed with its spread.  Beside the times: the bytes the pass has to move -- 4 B of depth in and 12 B of
point out per kept pixel, derived from the shapes, not measured -- and the rate that makes of the measured time.
Usage: python tools/gpu_point_cloud_cost.py [--envs 4096] [--rounds 5] [--reps 10]"""
import argparse
import ctypes
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stretch_mujoco_amd import StretchBatchSimulator  # noqa: E402
from stretch_mujoco_amd.enums import StretchCameras  # noqa: E402
from cost_common import timed  # noqa: E402


def torch_points(depth, W, H, fovy, stride, cpos, cmat):
    """The same arithmetic as a torch composition: [B, H, W] depth -> [B, H', W', 3] world points."""
    th = math.tan(fovy * math.pi / 360)
    d = depth[:, ::stride, ::stride]
    u = torch.arange(0, W, stride, device=depth.device, dtype=torch.float32)
    v = torch.arange(0, H, stride, device=depth.device, dtype=torch.float32)
    xn = (((u + 0.5) / W * 2 - 1) * th * W / H)[None, None, :]
    yn = ((1 - (v + 0.5) / H * 2) * th)[None, :, None]
    pc = torch.stack((d * xn, d * yn, -d), -1)
    pts = torch.einsum("bij,bhwj->bhwi", cmat, pc) + cpos[:, None, None, :]
    valid = torch.isfinite(d) & (d > 0)
    return torch.where(valid[..., None], pts, torch.full_like(pts, float("nan")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    B = a.envs
    sim = StretchBatchSimulator(num_envs=B, device="cuda:0", scene="stretch_scene", solver="newton", cameras_to_use=StretchCameras.depth())
    sim.start(home=False)
    g = torch.Generator(device="cuda:0").manual_seed(7)
    cr = torch.tensor(np.asarray(sim.model["actuator_ctrlrange"], np.float32), device="cuda:0")
    sim.ctrl.copy_(cr[:, 0:1] + (cr[:, 1:2] - cr[:, 0:1]) * torch.rand(sim.nu, B, generator=g, device="cuda:0"))   # every env at its own pose
    sim.step(300)
    torch.cuda.synchronize()
    print(f"point cloud cost: {B} envs, stretch_scene, world frame; ms per call from device events, {a.reps} calls per window, "
          f"median [min .. max] of {a.rounds} alternating rounds")
    names = sim.names["camera"]
    cam_pos = torch.tensor(np.asarray(sim.model["cam_pos"], np.float32), device="cuda:0")
    cam_mat = torch.tensor(np.asarray(sim.model["k_cam_mat"], np.float32).reshape(-1, 3, 3), device="cuda:0")
    for cam in StretchCameras.depth():
        st = cam.initial_camera_settings
        W, H, fovy = st.width, st.height, float(st.field_of_view_vertical_in_degrees)
        ci = names.index(cam.camera_name_in_mjcf)
        cb = int(np.asarray(sim.model["cam_bodyid"]).reshape(-1)[ci])
        bp = sim.xpose[12 * cb: 12 * cb + 3].t()
        bm = sim.xpose[12 * cb + 3: 12 * cb + 12].t().reshape(-1, 3, 3)
        cpos, cmat = bp + bm @ cam_pos[ci], bm @ cam_mat[ci]
        depth = sim._depth[cam]

        def render():
            sim._render_depth_into(cam, depth)

        render()
        torch.cuda.synchronize()
        print(f"  {cam.name}: {W} x {H}, fovy {fovy:g}, depth limit {cam.depth_limit:g} m, pixels with a depth {100 * float((depth > 0).float().mean()):.1f} %")
        for stride in (1, 4):
            hp, wp = -(-H // stride), -(-W // stride)
            pts = torch.empty(B, hp, wp, 3, dtype=torch.float32, device="cuda:0")

            def entry():
                rc = sim._L.smj_depth_to_points(sim._ctx, ci, W, H, fovy, ctypes.c_void_p(depth.data_ptr()), stride, -2,
                                                ctypes.c_void_p(pts.data_ptr()), sim._stream())
                assert rc == 0

            def composed():
                return torch_points(depth, W, H, fovy, stride, cpos, cmat)

            fns = {"entry": entry, "render": render, "torch": composed}
            for f in fns.values():      # warm-up of every shape
                f(); f()
            ref = composed()
            torch.cuda.synchronize()
            diff = float(torch.nan_to_num(pts - ref, nan=0.0).abs().max())
            same_nan = bool(torch.equal(torch.isnan(pts), torch.isnan(ref)))
            del ref
            res = {k: [] for k in fns}
            order = list(fns)
            for r in range(a.rounds):
                for k in order[r % 3:] + order[:r % 3]:
                    res[k].append(timed(fns[k], a.reps))
            med = {k: float(np.median(v)) for k, v in res.items()}
            kept = B * hp * wp
            need = 16.0 * kept
            line = "  ".join(f"{k} {med[k]:8.3f} [{min(res[k]):.3f} .. {max(res[k]):.3f}]" for k in order)
            print(f"    stride {stride}: {line}")
            print(f"      {kept / 1e6:.1f} M points, 16 B each = {need / 2**30:.2f} GiB to move: the entry reaches {need / (med['entry'] * 1e-3) / 1e12:.2f} TB/s "
                  f"of that traffic; torch / entry = {med['torch'] / med['entry']:.1f} x, entry / render = {100 * med['entry'] / med['render']:.1f} %; "
                  f"max |entry - torch| {diff:.2e} m, NaN pattern equal: {same_nan}")
            del pts
    sim.stop()


if __name__ == "__main__":
    main()
