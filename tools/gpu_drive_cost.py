"""Cost of the base command (smj_navigation_to_velocity) at 4096 envs of 128 x 128 cells, by the method of gpu_frontier_cost.py: the
world-frame map of the scene's lidar accumulated over a short drive, the maps of the first three envs tiled over all of them, their
inflated costmap and the navigation field to a goal a metre ahead; on it the default table (utils.arc_candidates(): 35 candidates of
13 points) and the largest one (1024 candidates of 32 points), each with cmd and best alone and with score_dev and cell_dev too; and,
in the same run on the same grids, smj_costmap_to_navigation, potential alone.  The statuses and the candidates scored per env are
printed, so that a map on which everything is blocked cannot pass for a cheap one.  Device events around `reps` back-to-back calls
after a warm-up; the variants alternate round by round; the median of the rounds is printed with its spread.  The head of the file is
what the compiler reports for the kernel, when hipcc is there.
Usage: python tools/gpu_drive_cost.py [--envs 4096] [--rounds 3] [--reps 3] [--scene stretch_scene] [--out profiles/drive_cost.txt]"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors  # noqa: E402
from stretch_mujoco_amd.utils import arc_candidates  # noqa: E402
from cost_common import LINES, alternate, resource_usage, say  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scene", default="stretch_scene")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "drive_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    B, dev = a.envs, "cuda:0"
    resource_usage("smj_drive.hip")
    sim = StretchBatchSimulator(num_envs=B, device=dev, scene=a.scene, solver="newton", sensors_to_use=[StretchSensors.base_lidar])
    sim.start(home=False)
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    nx = ny = 128
    x0, y0, cell = -3.187, -3.229, 0.05
    say(f"base command cost: {B} envs, {a.scene}, grid {nx} x {ny}, cell {cell} m, lethal 253, goal_weight 1, obstacle_weight 20, no window; ms per call from device "
        f"events, {a.reps} calls per window, median [min .. max] of {a.rounds} alternating rounds; beside it smj_costmap_to_navigation (lethal 253, neutral 50, "
        f"potential alone) on the same grid in the same run")
    grid = dict(frame="world", origin=(x0, y0), cell=cell, shape=(ny, nx), range_limits=(0.2, 2.0))
    for k in range(4):      # a short drive: the map grows
        og = sim.pull_occupancy_grid(accumulate=k > 0, **grid)
        sim.set_base_velocity(0.2, 0.5)
        sim.step(100)
    sim.set_base_velocity(0.0, 0.0)
    tile = lambda t: t[:3].repeat((B + 2) // 3, *([1] * (t.dim() - 1)))[:B].contiguous()
    og.hit.copy_(tile(og.hit))
    og.miss.copy_(tile(og.miss))
    pose = tile(sim.base_pose.t().contiguous()).t().contiguous()      # [3, B], the poses of the first three envs
    cost = sim.pull_distance_field(og, max_distance=0.56).inflated_cost(0.17, 0.56, 10.0).contiguous()
    ahead = torch.stack((pose[0] + torch.cos(pose[2]), pose[1] + torch.sin(pose[2])), 1)
    nf = sim.pull_navigation_field(ahead, cost, cell=cell, origin=(x0, y0))
    pot, goal = nf.potential, nf.goal.contiguous()
    scratch = torch.empty_like(pot)
    cmd, best = torch.empty(2, B, device=dev), torch.empty(B, 2, dtype=torch.int32, device=dev)
    rng = np.random.default_rng(5)
    tables = {"default table": arc_candidates(device=dev),
              "largest table": arc_candidates(rng.uniform(0.0, 0.25, 1024), rng.uniform(-1.0, 1.0, 1024), samples=31, device=dev)}

    def nav():
        assert sim._L.smj_costmap_to_navigation(sim._ctx, vp(cost), vp(goal), 1, nx, ny, 253, 50, vp(scratch), None, sim._stream()) == 0

    for name, t in tables.items():
        K, P = t.points.shape[:2]
        score, cells = torch.empty(B, K, dtype=torch.int64, device=dev), torch.empty(B, K, P, dtype=torch.int32, device=dev)

        def drive(full):
            assert sim._L.smj_navigation_to_velocity(sim._ctx, vp(pose), None, vp(cost), vp(pot), nx, ny, x0, y0, cell, vp(t.command), vp(t.points), None, K, P, 253, 0,
                                                     1, 20, 1000, float("inf"), float("inf"), vp(cmd), vp(best), vp(score) if full else None,
                                                     vp(cells) if full else None, sim._stream()) == 0

        drive(True)
        torch.cuda.synchronize()
        scored = (score[:3] != (1 << 63) - 1).sum(1).tolist()
        what = f"status {best[:3, 1].tolist()}, chosen {best[:3, 0].tolist()}, {scored} of {K} candidates scored in envs 0 .. 2"
        res, med = alternate({"cmd and best": lambda: drive(False), "with score and cell": lambda: drive(True), "navigation": nav}, a.rounds, a.reps)
        times = "  ".join(f"{k} {med[k]:9.4f} [{min(res[k]):.4f} .. {max(res[k]):.4f}]" for k in res)
        say(f"  {name}, K = {K}, P = {P} ({what}): {times}   command / navigation = {med['cmd and best'] / med['navigation']:.4f}")
        read = B * K * P * (1 + 8) + B * K * 4      # a cost byte per point and the table entry from L2, a potential per candidate
        say(f"    reads at most {read / 1e6:.1f} MB, writes {B * 16 / 1e6:.2f} MB (+ {(B * K * 8 + B * K * P * 4) / 1e6:.1f} MB with score and cell)")
    sim.stop()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
