"""Map and localise at once, for a batch of robots, without leaving the device: the first scan is mapped at the start pose; then, per
leg of a slow arc, a prior is dead-reckoned from the commanded twist (with a deliberate bias on top of what the wheels really do),
the scan is matched against the map so far, integrated into it at the matched pose, and the distance field is made anew.

    python examples/slam_batch.py [num_envs] [legs]

pull_scan_match() finds the pose, pull_map_update(match.pose, gate=match) ray-traces the scan into the map at that pose -- only for
the envs whose match is ok: the gate reads the matcher's status where it lies -- and pull_distance_field(update.grid) turns the map
into what the next match runs against.  Nothing is read back inside the loop.  Printed per env: the pose error of dead reckoning and
of the loop against the simulator's own pose, and the share of the map's hit cells that lie within one cell of a map made with the
simulator's own pose.
"""
import sys

import torch

sys.path.insert(0, ".")
from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
legs = int(sys.argv[2]) if len(sys.argv) > 2 else 8
sim = StretchBatchSimulator(num_envs=B, device="cuda:0", scene="stretch_kitchen_standin", sensors_to_use=[StretchSensors.base_lidar])
sim.start()
dev = sim.device
grid = dict(origin=(-3.2, -3.2), cell=0.05, shape=(128, 128))
sim.step(20)
start = sim.base_pose.clone()
update = sim.pull_map_update(start, accumulate=False, **grid)                         # the first scan, at the start pose
truth_map = sim.pull_occupancy_grid(frame="world", accumulate=False, **grid)          # the same map with the simulator's own pose, to compare
df = sim.pull_distance_field(update.grid)
est, dead = start.clone(), start.clone()
v, w, steps = 0.08, 0.35, 100
dt = steps * float(sim.timestep)
bias = torch.tensor([[0.02], [-0.015], [0.02]], device=dev)                           # per leg: metres, metres, radians (1.1 degrees)
gated = torch.zeros(B, dtype=torch.int32, device=dev)
sim.set_base_velocity(v, w)
for leg in range(legs):
    sim.step(steps)

    def reckon(pose):
        """the pose a leg later by the commanded twist, plus the bias"""
        th = pose[2] + 0.5 * w * dt
        return pose + torch.stack((v * dt * torch.cos(th), v * dt * torch.sin(th), torch.full_like(th, w * dt))) + bias

    dead = reckon(dead)
    match = sim.pull_scan_match(df, reckon(est), sigma=0.10)
    update = sim.pull_map_update(match.pose, gate=match, **grid)
    est = match.pose.clone()
    gated += update.gated().to(torch.int32)
    df = sim.pull_distance_field(update.grid)
    truth_map = sim.pull_occupancy_grid(frame="world", accumulate=True, **grid)
sim.set_base_velocity(0.0, 0.0)
torch.cuda.synchronize()
truth = sim.base_pose


def err(pose):
    d = pose - truth
    d[2] = torch.atan2(torch.sin(d[2]), torch.cos(d[2]))
    return " ".join(f"({x * 100:.1f} cm, {y * 100:.1f} cm, {t * 57.2958:.2f} deg)" for x, y, t in d.abs().t().tolist())


near = torch.nn.functional.max_pool2d((truth_map.hit > 0).float().unsqueeze(1), 3, 1, 1).squeeze(1) > 0
ours = update.grid.hit > 0
share = (ours & near).sum((1, 2)).float() / ours.sum((1, 2)).clamp(min=1).float()
print("legs", legs, "status of the last match", match.status.tolist(), "returns integrated", update.returns().tolist(), "legs gated", gated.tolist())
print("error of dead reckoning", err(dead))
print("error of the loop      ", err(est))
print("hit cells", ours.sum((1, 2)).tolist(), "share within one cell of the truth-pose map", [round(s, 3) for s in share.tolist()])
print("map", tuple(update.grid.hit.shape), update.grid.frame, "info", tuple(update.info.shape))
sim.stop()
