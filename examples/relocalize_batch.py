"""Find a batch of robots again after they were moved, without leaving the device: map with the loop of slam_batch.py, put every robot
down somewhere else (0.45 m, 0.4 m and 20 degrees from where it believes it is), and localise with a particle filter from a spread
of +-1 m and +-30 degrees round the stale belief; then hand the best particle to the scan matcher for the last cell.

    python examples/relocalize_batch.py [num_envs] [updates]

pull_particle_update() weighs P pose hypotheses per env by the likelihood field under the scan's returns and resamples them
(update.particles goes into the next call as it is; update.predict(odometry) first when the robot has moved in between -- here it
stands still, so only noise is added).  update.pose, the best particle, is a [3, B] tensor on the device and goes into
pull_scan_match(prior=...) as it is.  The scan matcher alone searches +-0.5 m and +-5 degrees round its prior: from the stale belief
it cannot turn far enough.  update.status: 0 ok, 1 too few returns, 2 lost (no particle puts a return on the map).  Printed per env:
the error of the best particle per update, of the matcher started from it, and of the matcher alone.
"""
import sys

import torch

sys.path.insert(0, ".")
from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors, utils  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
updates = int(sys.argv[2]) if len(sys.argv) > 2 else 6
P = 2048
sim = StretchBatchSimulator(num_envs=B, device="cuda:0", scene="stretch_kitchen_standin", sensors_to_use=[StretchSensors.base_lidar])
sim.start()
dev = sim.device
grid = dict(origin=(-3.2, -3.2), cell=0.05, shape=(128, 128))
sim.step(20)

# ---- map: the loop of slam_batch.py, four legs of a slow arc
est = sim.base_pose.clone()
update = sim.pull_map_update(est, accumulate=False, **grid)
df = sim.pull_distance_field(update.grid)
v, w, steps = 0.08, 0.35, 100
dt = steps * float(sim.timestep)
sim.set_base_velocity(v, w)
for leg in range(4):
    sim.step(steps)
    th = est[2] + 0.5 * w * dt
    prior = est + torch.stack((v * dt * torch.cos(th), v * dt * torch.sin(th), torch.full_like(th, w * dt)))
    match = sim.pull_scan_match(df, prior, sigma=0.10)
    update = sim.pull_map_update(match.pose, gate=match, **grid)
    est = match.pose.clone()
    df = sim.pull_distance_field(update.grid)
sim.set_base_velocity(0.0, 0.0)
sim.step(100)

# ---- move every robot: the free joint's position and quaternion, then let it settle.  `est` is now a stale belief
yaw = sim.base_pose[2] + 0.349
sim.qpos[0] += 0.45
sim.qpos[1] -= 0.40
sim.qpos[3], sim.qpos[4], sim.qpos[5], sim.qpos[6] = torch.cos(yaw / 2), torch.zeros_like(yaw), torch.zeros_like(yaw), torch.sin(yaw / 2)
sim.qvel[:6] = 0.0
sim.step(200)
truth = sim.base_pose.clone()

# ---- localise: a spread round the stale belief, a few updates, then the matcher from the best particle
gen = torch.Generator(device=dev)
gen.manual_seed(1)
particles = utils.spread_particles(est, (1.0, 1.0, 0.5236), P, generator=gen)
history = []
for it in range(updates):
    up = sim.pull_particle_update(df, particles, utils.particle_noise(0.02, 0.01, (3, B, P), generator=gen), span=4096)
    particles = up.particles
    history.append((up.pose.clone(), up.ess().clone(), up.status.clone()))
alone = sim.pull_scan_match(df, est, sigma=0.10).pose.clone()                          # the matcher from the stale belief
both = sim.pull_scan_match(df, up.pose, sigma=0.10).pose.clone()                       # the matcher from the best particle
torch.cuda.synchronize()


def err(pose):
    d = pose - truth
    ang = torch.atan2(torch.sin(d[2]), torch.cos(d[2])).abs()
    return " ".join(f"({m * 100:.1f} cm, {t * 57.2958:.2f} deg)" for m, t in zip(torch.hypot(d[0], d[1]).tolist(), ang.tolist()))


print("particles", P, "updates", updates, "the robots were moved by", err(est))
for it, (pose, ess, status) in enumerate(history):
    print(f"update {it}: status {status.tolist()} effective sample size {ess.tolist()} error of the best particle {err(pose)}")
print("error of the matcher alone           ", err(alone))
print("error of the filter, then the matcher", err(both))
print("particles", tuple(up.particles.shape), up.particles.dtype, "weights", tuple(up.weights.shape), "stat", tuple(up.stat.shape), "frame", up.frame)
sim.stop()
