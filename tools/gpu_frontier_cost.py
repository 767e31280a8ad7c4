"""Cost of the frontier regions (smj_occupancy_to_frontiers) at 4096 envs of 128 x 128 cells (and 256 x 256, labelled in global
memory), by the method of gpu_navigation_cost.py: the world-frame map of the scene's lidar accumulated over a short drive, the maps of
the first three envs tiled over all of them, with and without the inflated costmap; the serpentine (a free corridor between unknown
walls: one region of 8255 cells at 128 x 128, the worst case for a labelling) in every env; and, in the same run on the same grids,
smj_costmap_to_navigation to the frontier goals (to cell 0 on the serpentine), potential alone.  Regions, frontier cells and goals per
env are printed per map, so that a map without a frontier cannot pass for a cheap one.  Device events around `reps` back-to-back calls
after a warm-up; the variants alternate round by round; the median of the rounds is printed with its spread.  The head of the file is
what the compiler reports for the two kernels, when hipcc is there.
Usage: python tools/gpu_frontier_cost.py [--envs 4096] [--rounds 3] [--reps 3] [--scene stretch_scene] [--out profiles/frontier_cost.txt]"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors  # noqa: E402
from cost_common import LINES, alternate, resource_usage, say  # noqa: E402


def serpentine(ny, nx):
    """(hit, miss) int32: the rows y = 1, 3, 5, .. unknown except one gap at alternating ends, every other cell free."""
    free = np.ones((ny, nx), bool)
    for k, y in enumerate(range(1, ny, 2)):
        free[y, :] = False
        free[y, nx - 1 if k % 2 == 0 else 0] = True
    return np.zeros((ny, nx), np.int32), free.astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scene", default="stretch_scene")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frontier_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    B, dev = a.envs, "cuda:0"
    resource_usage("smj_front.hip")
    sim = StretchBatchSimulator(num_envs=B, device=dev, scene=a.scene, solver="newton", sensors_to_use=[StretchSensors.base_lidar])
    sim.start(home=False)
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    say(f"frontier cost: {B} envs, {a.scene}, cell 0.05 m, min_hits 1, lethal 253, min_size 4, max_regions 16; ms per call from device events, "
        f"{a.reps} calls per window, median [min .. max] of {a.rounds} alternating rounds; beside it smj_costmap_to_navigation (lethal 253, neutral 50, "
        f"potential alone) on the same grid in the same run")
    for nx, ny in ((128, 128), (256, 256)):
        n = nx * ny
        grid = dict(frame="world", origin=(-nx * 0.025, -ny * 0.025), cell=0.05, shape=(ny, nx), range_limits=(0.2, 2.0))
        for k in range(4):      # a short drive: the map grows
            og = sim.pull_occupancy_grid(accumulate=k > 0, **grid)
            sim.set_base_velocity(0.2, 0.5)
            sim.step(100)
        tile = lambda t: t[:3].repeat((B + 2) // 3, 1, 1)[:B].contiguous()
        hit, miss = tile(og.hit), tile(og.miss)
        og.hit.copy_(hit)
        og.miss.copy_(miss)
        cost = sim.pull_distance_field(og, max_distance=0.56).inflated_cost(0.17, 0.56, 10.0).contiguous()
        sh, sm = (torch.tensor(t, device=dev).expand(B, ny, nx).contiguous() for t in serpentine(ny, nx))
        scost = torch.where(sm > 0, 0, 254).to(torch.uint8).contiguous()
        label, pot = (torch.empty(B, ny, nx, dtype=torch.int32, device=dev) for _ in range(2))
        goal, region, count = (torch.empty(B, *s, dtype=torch.int32, device=dev) for s in ((16,), (16, 4), (2,)))
        zero = torch.zeros(B, 16, dtype=torch.int32, device=dev)
        zero[:, 1:] = -1

        def front(h, m, c):
            assert sim._L.smj_occupancy_to_frontiers(sim._ctx, vp(h), vp(m), vp(c), nx, ny, 1, 253, 4, 16, vp(label), vp(goal), vp(region), vp(count), sim._stream()) == 0

        def nav(c, g):
            assert sim._L.smj_costmap_to_navigation(sim._ctx, vp(c), vp(g), 16, nx, ny, 253, 50, vp(pot), None, sim._stream()) == 0

        front(hit, miss, cost)
        torch.cuda.synchronize()
        mapgoals = goal.clone()      # passable goals: the navigation entry uses every one of them
        say(f"  grid {nx} x {ny} ({'labels in LDS' if n <= 16384 else 'labels in label_dev itself'})")
        for name, h, m, c in (("accumulated map", hit, miss, None), ("accumulated map with its costmap", hit, miss, cost), ("serpentine", sh, sm, None)):
            front(h, m, c)
            torch.cuda.synchronize()
            what = f"{count[:3, 0].tolist()} regions, {count[:3, 1].tolist()} frontier cells, {(goal[:3] >= 0).sum(1).tolist()} goals in envs 0 .. 2"
            navcost, navgoal = (scost, zero) if name == "serpentine" else (cost, mapgoals)
            res, med = alternate({"frontiers": lambda: front(h, m, c), "navigation": lambda: nav(navcost, navgoal)}, a.rounds, a.reps)
            times = "  ".join(f"{k} {med[k]:9.4f} [{min(res[k]):.4f} .. {max(res[k]):.4f}]" for k in res)
            say(f"    {name} ({what}): {times}   frontiers / navigation = {med['frontiers'] / med['navigation']:.3f}")
    sim.stop()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
