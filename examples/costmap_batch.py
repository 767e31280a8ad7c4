"""Distance fields and inflated costmaps from the lidar, for a batch of robots in the kitchen stand-in: the layer every navigation
stack puts on its occupancy grid, computed on the device.

    python examples/costmap_batch.py [num_envs]

pull_distance_field() turns the occupancy grid of the last scan (pull_occupancy_grid) into the exact squared distance, in cells, from
every cell to the nearest occupied cell, and with nearest=True into that cell's index -- integers only, one fused pass.  Here: the
base frame, 128 x 128 cells of 5 cm (robot in the middle), searched out to 1 m.  distance() gives metres, so the value at the robot's own
cell is the clearance of the base; inflated_cost() gives the costmap_2d convention: 254 lethal, 253 inscribed, decaying to 0.
"""
import sys

import torch

sys.path.insert(0, ".")
from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
sim = StretchBatchSimulator(num_envs=B, device="cuda:0", scene="stretch_kitchen_standin", sensors_to_use=[StretchSensors.base_lidar])
sim.start()
for e in range(B):                                     # every env its own turn of the base
    sim.set_base_velocity(0.05, 0.3 * (e - (B - 1) / 2), env_ids=[e])
sim.step(300)
sim.set_base_velocity(0.0, 0.0)
sim.step(50)
df = sim.pull_distance_field(nearest=True, max_distance=1.0, origin=(-3.2, -3.2), cell=0.05, shape=(128, 128))
print("dist2", tuple(df.dist2.shape), df.dist2.dtype, "nearest", tuple(df.nearest.shape), "frame", df.frame, "cell", df.cell)
dist, cost, off = df.distance(), df.inflated_cost(inscribed_radius=0.17, inflation_radius=0.55), df.nearest_offset()
iy, ix = int((0.0 - df.origin[1]) / df.cell), int((0.0 - df.origin[0]) / df.cell)          # the cell of the base's origin
chars = " .:-=+*#%@"
for e in range(B):
    d = float(dist[e, iy, ix])
    dy, dx = (int(v) for v in off[e, iy, ix])
    print(f"env {e}: clearance of the base {d:.2f} m" + (f", nearest obstacle {dx * df.cell:+.2f} m in x, {dy * df.cell:+.2f} m in y" if d < float("inf") else " (nothing within 1 m)")
          + f"; lethal cells {int((cost[e] == 254).sum())}, inscribed {int((cost[e] == 253).sum())}, inflated {int(((cost[e] > 0) & (cost[e] < 253)).sum())}")
    coarse = cost[e].view(32, 4, 32, 4).amax((1, 3))                # 32 x 32 blocks of 4 x 4 cells, the dearest cell of each
    for row in reversed(range(32)):                                  # +y up
        print("    " + "".join("R" if (row, col) == (iy // 4, ix // 4) else chars[min(9, int(v) * 10 // 255)] for col, v in enumerate(coarse[row].tolist())))
torch.cuda.synchronize()
sim.stop()
