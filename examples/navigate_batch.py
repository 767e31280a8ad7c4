"""Drive a batch of robots to a goal each, around the kitchen stand-in's furniture, with every layer on the device: lidar scan ->
world-frame occupancy accumulated over the drive -> exact distance field -> inflated costmap -> exact cost-to-goal field -> the base
follows heading().

    python examples/navigate_batch.py [num_envs]

pull_navigation_field() gives per cell the cheapest path cost to the goal (potential) and the neighbour to step to (next), integers
only, one HIP pass per call.  Here: the world frame, 128 x 128 cells of 5 cm, the map accumulated across steps so that what the lidar
saw earlier stays an obstacle; every 250 steps (half a second) the field is rebuilt from the grown map and the base turns towards
heading() at its own cell, driving forward when it roughly faces that way.  distance() at the robot's cell is the path length that
remains; it can grow when the map does.
"""
import math
import sys

import torch

sys.path.insert(0, ".")
from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
sim = StretchBatchSimulator(num_envs=B, device="cuda:0", scene="stretch_kitchen_standin", sensors_to_use=[StretchSensors.base_lidar])
sim.start()
dev = sim.device
grid = dict(frame="world", origin=(-3.2, -3.2), cell=0.05, shape=(128, 128))
angle = torch.linspace(0.0, 2.0 * math.pi, B + 1, device=dev)[:B]
goal = torch.stack((1.5 * torch.cos(angle), 1.5 * torch.sin(angle)), 1)             # [B, 2] metres, one goal per env on a circle
sim.step(20)
for it in range(60):
    og = sim.pull_occupancy_grid(accumulate=it > 0, **grid)                          # the map grows across steps
    df = sim.pull_distance_field(og, max_distance=0.56)
    nf = sim.pull_navigation_field(goal, df, next=True)                               # inflated with the default radii, then relaxed
    pose = sim.base_pose                                                              # [3, B]: x, y, theta
    here = torch.stack((pose[0], pose[1]), 1)
    cells = nf.path(here, 0)[:, 0]                                                    # the robot's own cell, -1 where it has no path
    ok = cells >= 0
    flat = cells.clamp(min=0).unsqueeze(1)
    want = nf.heading().reshape(B, -1).gather(1, flat).squeeze(1)                     # NaN on the goal cell
    left = nf.distance().reshape(B, -1).gather(1, flat).squeeze(1)
    turn = torch.atan2(torch.sin(want - pose[2]), torch.cos(want - pose[2]))
    go = ok & torch.isfinite(want)
    v = torch.where(go & (turn.abs() < 0.5), 0.25, 0.0)
    w = torch.where(go, turn.clamp(-1.0, 1.0), torch.zeros_like(turn))
    for e, (ve, we) in enumerate(zip(v.tolist(), w.tolist())):                         # the host loop is the example's, not the pipeline's
        sim.set_base_velocity(ve, we, env_ids=[e])
    if it % 10 == 0:
        print(f"iteration {it}: path left per env [m] " + " ".join(f"{d:.2f}" if math.isfinite(d) else "none" for d in torch.where(ok, left, torch.full_like(left, float('inf'))).tolist()))
    sim.step(250)
sim.set_base_velocity(0.0, 0.0)
sim.step(10)
torch.cuda.synchronize()
print("potential", tuple(nf.potential.shape), nf.potential.dtype, "next", tuple(nf.next.shape), "frame", nf.frame, "goal cells", nf.goal[:, 0].tolist())
sim.stop()
