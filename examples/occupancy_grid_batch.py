"""Ray-traced 2-D occupancy grids from the lidar, for a batch of robots in the default scene: the flow of the reference's
examples/laser_scan.py (ranges -> x/y points around the robot, filtered to 0.2 .. 5 m) carried one step further, on the device.

    python examples/occupancy_grid_batch.py [num_envs]

pull_occupancy_grid() walks every ray of the scan through a grid around the robot in one fused pass: per cell the rays that end in
it on something (hit) and the rays that pass through it (miss).  Here: the base frame, 128 x 128 cells of 5 cm (6.4 m square, robot in
the middle); a ray without a return clears the cells over 5 m.  occupancy() folds the two counts into the ROS convention: 100
occupied, 0 free, -1 unknown.  Then the same in the world frame, accumulated while the robots turn: a map.
"""
import sys

import torch

sys.path.insert(0, ".")
from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
sim = StretchBatchSimulator(num_envs=B, device="cuda:0", scene="stretch_scene", sensors_to_use=[StretchSensors.base_lidar])
sim.start()
for e in range(B):                                     # every env its own turn of the base
    sim.set_base_velocity(0.0, 0.3 * (e - (B - 1) / 2), env_ids=[e])
sim.step(500)
sim.set_base_velocity(0.0, 0.0)
sim.step(100)
scan = sim.pull_sensor_data().lidar                    # [B, 360] ranges, -1 where nothing was hit
keep = (scan > 0.2) & (scan < 5.0)                     # laser_scan.py's filter
print("scan", tuple(scan.shape), "rays kept by the 0.2 .. 5 m filter per env:", [int(v) for v in keep.sum(1)])
og = sim.pull_occupancy_grid(frame="base", origin=(-3.2, -3.2), cell=0.05, shape=(128, 128), range_limits=(0.2, 5.0))
print("hit", tuple(og.hit.shape), og.hit.dtype, "miss", tuple(og.miss.shape), og.miss.dtype, "frame", og.frame)
occ = og.occupancy()
for e in range(B):
    print(f"  env {e}: free {int((occ[e] == 0).sum())}, occupied {int((occ[e] == 100).sum())}, unknown {int((occ[e] == -1).sum())} of {occ[e].numel()} cells")
world = dict(frame="world", origin=(-4.8, -4.8), cell=0.05, shape=(192, 192))
sim.pull_occupancy_grid(**world)                       # the first scan overwrites the map ...
sim.set_base_velocity(0.0, 0.5)
for _ in range(10):                                    # ... the next ten, taken while turning, accumulate into it
    sim.step(50)
    mapped = sim.pull_occupancy_grid(accumulate=True, **world)
sim.set_base_velocity(0.0, 0.0)
occ, lo = mapped.occupancy(min_hits=2), mapped.log_odds()
for e in range(B):
    print(f"  env {e}, world map of 11 scans: free {int((occ[e] == 0).sum())}, occupied {int((occ[e] == 100).sum())}, unknown {int((occ[e] == -1).sum())}; "
          f"log odds in [{float(lo[e].min()):.1f}, {float(lo[e].max()):.1f}]")
torch.cuda.synchronize()
sim.stop()
