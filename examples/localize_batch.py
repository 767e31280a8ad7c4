"""Localise a batch of robots in a map they made themselves, without leaving the device: lidar scans -> world-frame occupancy
accumulated over a short turn on the spot -> exact distance field -> likelihood field -> correlative scan matching from priors that
are off by a few cells and degrees -> the error before and after.

    python examples/localize_batch.py [num_envs] [mapping_iterations]

pull_scan_match() lays the returns of the scan over the likelihood field from every pose of a window round the prior (here 21
rotations of half a degree by 21 x 21 shifts of one cell) and keeps the pose under which they collect the largest sum.  match.pose
is a [3, B] tensor on the device and goes into pull_base_command(pose=match.pose) as it is; refined() interpolates between the
lattice poses.  match.status: 0 ok, 1 too few returns, 2 the prior is not finite.
"""
import sys

import torch

sys.path.insert(0, ".")
from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
iterations = int(sys.argv[2]) if len(sys.argv) > 2 else 8
sim = StretchBatchSimulator(num_envs=B, device="cuda:0", scene="stretch_kitchen_standin", sensors_to_use=[StretchSensors.base_lidar])
sim.start()
dev = sim.device
grid = dict(frame="world", origin=(-3.2, -3.2), cell=0.05, shape=(128, 128))
sim.step(20)
sim.set_base_velocity(0.0, 0.6)                                                       # turn on the spot: the rays sweep the walls
for it in range(iterations):
    og = sim.pull_occupancy_grid(accumulate=it > 0, **grid)                           # mapped with the simulator's own pose
    sim.step(50)
sim.set_base_velocity(0.0, 0.0)
sim.step(100)
df = sim.pull_distance_field(og)
truth = sim.base_pose.clone()
# priors off the truth by whole lattice steps: cells of 5 cm in x and y, half degrees in theta
off = torch.tensor([[3.0, -2.0, 4.0], [-7.0, 5.0, -6.0], [0.0, 0.0, 0.0], [6.0, -8.0, 9.0]], device=dev)[torch.arange(B, device=dev) % 4].t()
step = torch.tensor([[0.05], [0.05], [0.008727]], device=dev)
prior = truth + off * step
match = sim.pull_scan_match(df, prior, sigma=0.10, scores=True)
fine = match.refined()
torch.cuda.synchronize()


def err(pose):
    d = (pose - truth).abs()
    return " ".join(f"({x * 100:.1f} cm, {y * 100:.1f} cm, {t * 57.2958:.2f} deg)" for x, y, t in d.t().tolist())


print("status", match.status.tolist(), "returns", match.best[:, 2].tolist(), "fit", [round(v, 3) for v in match.fit().tolist()])
print("offset (dx, dy, rotation row)", match.offset().tolist())
print("error of the prior  ", err(prior))
print("error of the match  ", err(match.pose))
print("error of refined()  ", err(fine))
print("pose", tuple(match.pose.shape), match.pose.dtype, "best", tuple(match.best.shape), "score", tuple(match.score.shape), "frame", match.frame)
sim.stop()
