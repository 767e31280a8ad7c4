"""Let a batch of robots explore the kitchen stand-in on their own, with every layer on the device: lidar scan -> world-frame
occupancy accumulated over the drive -> exact distance field -> inflated costmap -> frontier regions -> exact cost-to-goal field to
the regions' goal cells -> the base follows heading().  Nobody hands in a goal.

    python examples/explore_batch.py [num_envs] [iterations]

pull_frontiers() gives the free cells that border unseen space, grouped into regions, and one goal cell per region (fr.goal); that
tensor is the goal of pull_navigation_field() as it is.  With cost=... a goal never lies where the robot does not fit.  Here: the
world frame, 128 x 128 cells of 5 cm, returns out to 2 m; every 250 steps (half a second) the chain is rebuilt from the grown map and
the base turns towards heading() at its own cell -- the nearest goal in path cost wins, as the field is relaxed from all of them.  An
env without a region of at least min_size cells left has seen what it can reach and stops.
"""
import sys

import torch

sys.path.insert(0, ".")
from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
iterations = int(sys.argv[2]) if len(sys.argv) > 2 else 40
sim = StretchBatchSimulator(num_envs=B, device="cuda:0", scene="stretch_kitchen_standin", sensors_to_use=[StretchSensors.base_lidar])
sim.start()
grid = dict(frame="world", origin=(-3.2, -3.2), cell=0.05, shape=(128, 128), range_limits=(0.2, 2.0))
sim.step(20)
for it in range(iterations):
    og = sim.pull_occupancy_grid(accumulate=it > 0, **grid)                          # the map grows across steps
    df = sim.pull_distance_field(og, max_distance=0.56)
    cost = df.inflated_cost(0.17, 0.56, 10.0)
    fr = sim.pull_frontiers(og, cost=cost, min_size=6)                                # up to 16 regions per env, the largest first
    nf = sim.pull_navigation_field(fr.goal, cost, cell=og.cell, origin=og.origin, next=True)
    pose = sim.base_pose                                                              # [3, B]: x, y, theta
    here = torch.stack((pose[0], pose[1]), 1)
    cells = nf.path(here, 0)[:, 0]                                                    # the robot's own cell, -1 where it has no path
    want = nf.heading().reshape(B, -1).gather(1, cells.clamp(min=0).unsqueeze(1)).squeeze(1)      # NaN on a goal cell
    turn = torch.atan2(torch.sin(want - pose[2]), torch.cos(want - pose[2]))
    go = (cells >= 0) & torch.isfinite(want) & (fr.count[:, 0] > 0)                   # no region left: stop
    v = torch.where(go & (turn.abs() < 0.5), 0.25, 0.0)
    w = torch.where(go, turn.clamp(-1.0, 1.0), torch.zeros_like(turn))
    for e, (ve, we) in enumerate(zip(v.tolist(), w.tolist())):                         # the host loop is the example's, not the pipeline's
        sim.set_base_velocity(ve, we, env_ids=[e])
    if it % 5 == 0 or it == iterations - 1:
        seen = ((og.hit > 0) | (og.miss > 0)).sum((1, 2)).tolist()
        print(f"iteration {it}: " + "; ".join(f"env {e}: {r} regions left, {s} cells seen" for e, (r, s) in enumerate(zip(fr.count[:, 0].tolist(), seen))))
    sim.step(250)
sim.set_base_velocity(0.0, 0.0)
sim.step(10)
torch.cuda.synchronize()
print("goal", tuple(fr.goal.shape), fr.goal.dtype, "label", tuple(fr.label.shape), "frame", fr.frame, "goal cells of env 0", fr.goal[0].tolist())
sim.stop()
