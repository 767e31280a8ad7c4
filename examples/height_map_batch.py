"""Egocentric height maps, fused over both depth cameras, for a batch of robots in the default scene (floor, table, two objects).

    python examples/height_map_batch.py [num_envs]

pull_height_map() bins the depth images on the device, one fused pass per camera: per cell of a grid around the robot the highest
point and the number of points inside a height band.  Here: the base frame, 64 x 64 cells of 5 cm (3.2 m square, robot in the
middle), heights from 5 cm below the floor to 2 m; the robots are driven apart first, so every env sees the table from its own pose.
The map holds whatever the cameras see, the robot's own arm and gripper included.
"""
import sys

import torch

sys.path.insert(0, ".")
from stretch_mujoco_amd import StretchBatchSimulator, StretchCameras  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
sim = StretchBatchSimulator(num_envs=B, device="cuda:0", scene="stretch_scene", cameras_to_use=StretchCameras.depth())
sim.start()                                            # home pose: the wrist camera looks over the table
sim.move_to("head_pan", -1.57)                         # the head camera along the arm, down at the table
sim.move_to("head_tilt", -0.8)
for e in range(B):                                     # every env its own turn of the base
    sim.set_base_velocity(0.0, 0.3 * (e - (B - 1) / 2), env_ids=[e])
sim.step(500)
sim.set_base_velocity(0.0, 0.0)
sim.step(100)
hm = sim.pull_height_map(frame="base", origin=(-1.6, -1.6), cell=0.05, shape=(64, 64), z_range=(-0.05, 2.0))
print("height", tuple(hm.height.shape), hm.height.dtype, "count", tuple(hm.count.shape), hm.count.dtype, "frame", hm.frame)
occupied = hm.count > 0
for e in range(B):
    h = hm.height[e][occupied[e]]
    floor = int((h.abs() < 0.02).sum())
    print(f"  env {e}: occupied cells {int(occupied[e].sum())} of {occupied[e].numel()} ({int(hm.count[e].sum())} points), "
          f"{floor} of them floor, highest point {float(h.max()):.3f} m" if h.numel() else f"  env {e}: nothing in view")
for cam in StretchCameras.depth():                     # one camera at a time: render=False reuses the images of the call above
    one = sim.pull_height_map(cameras=[cam], frame="base", origin=(-1.6, -1.6), shape=(64, 64), z_range=(-0.05, 2.0), render=False)
    print(f"  {cam.name} alone: occupied cells per env {[int(v) for v in (one.count > 0).sum((1, 2))]}")
sim.stop()
