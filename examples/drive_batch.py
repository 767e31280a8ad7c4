"""Drive a batch of robots to a goal each, around the kitchen stand-in's furniture, without leaving the device: lidar scan ->
world-frame occupancy accumulated over the drive -> exact distance field -> inflated costmap -> exact cost-to-goal field -> the best
of a table of candidate arcs -> set_base_velocity.  The chain of examples/navigate_batch.py with its host loop replaced by the
local planner.

    python examples/drive_batch.py [num_envs] [iterations]

pull_base_command() lays every candidate arc (35 here: utils.arc_candidates()) over the costmap from the robot's pose, drops
those that touch a lethal cell, end where there is no path, or lie out of reach of the last commanded velocity, and scores the rest
by the potential at a point ahead of the arc's end plus the largest cost swept.  cmd.v and cmd.w are [B] tensors on the device and go
into set_base_velocity as they are.  cmd.status: 0 driving, 1 arrived, 2 every arc blocked, 3 off the grid.
"""
import sys

import torch

sys.path.insert(0, ".")
from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors  # noqa: E402
from stretch_mujoco_amd.utils import arc_candidates  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
iterations = int(sys.argv[2]) if len(sys.argv) > 2 else 100
sim = StretchBatchSimulator(num_envs=B, device="cuda:0", scene="stretch_kitchen_standin", sensors_to_use=[StretchSensors.base_lidar])
sim.start()
dev = sim.device
grid = dict(frame="world", origin=(-3.2, -3.2), cell=0.05, shape=(128, 128))
angle = torch.tensor([0.9, 1.3, 2.1], device=dev)[torch.arange(B, device=dev) % 3]  # three free directions of the room, in turn
goal = torch.stack((torch.cos(angle), torch.sin(angle)), 1)                          # [B, 2] metres, a metre from the start
steps = 100
# the simulated base reaches about a quarter of a commanded speed: arcs of half a second, a scoring point just ahead, turning in place
# biased by three cells of path (DESIGN.md section 3 has the measurement)
table = arc_candidates(horizon=0.5, lookahead=0.05, turn_bias=1500, device=dev)
period = steps * float(sim.timestep)                                                 # a new command every 0.2 s
sim.step(20)
for it in range(iterations):
    og = sim.pull_occupancy_grid(accumulate=it > 0, **grid)                          # the map grows across steps
    df = sim.pull_distance_field(og, max_distance=0.56)
    cost = df.inflated_cost(0.17, 0.56, 10.0)                                        # the costmap the field is planned on
    nf = sim.pull_navigation_field(goal, df)                                          # inflated the same way, then relaxed
    cmd = sim.pull_base_command(nf, cost, candidates=table, max_accel=(0.5, 2.5), period=period)        # within 0.1 m/s and 0.5 rad/s of the last command
    sim.set_base_velocity(cmd.v, cmd.w)                                               # device tensors: nothing was read back
    if it % 10 == 0 or it == iterations - 1:
        print(f"iteration {it}: status {cmd.status.tolist()} chosen {cmd.chosen.tolist()} cmd " + " ".join(f"({v:.2f}, {w:+.2f})" for v, w in zip(cmd.v.tolist(), cmd.w.tolist())))
    sim.step(steps)
sim.set_base_velocity(0.0, 0.0)
sim.step(10)
torch.cuda.synchronize()
print("cmd", tuple(cmd.cmd.shape), cmd.cmd.dtype, "best", tuple(cmd.best.shape), "frame", cmd.frame, "arrived", cmd.arrived().tolist())
sim.stop()
