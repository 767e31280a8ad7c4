"""Cost of the navigation fields (smj_costmap_to_navigation) at 4096 envs, by the method of gpu_distance_field_cost.py: grids of
64 x 64, 128 x 128 and 256 x 256 cells of 0.05 m, each with four maps -- the inflated costmap of the scene's lidar scan (base frame,
inscribed radius 0.17 m, inflation radius 0.56 m, the goal at the zero-cost cell nearest to 1 m ahead of the robot), an empty map (goal
in the centre), the serpentine (rows 1, 3, 5, .. lethal except one gap at alternating ends, goal at cell 0) and a map with 30 % lethal
cells and random costs 0 .. 252 (three goals) -- each with and without the next buffer, lethal 253, neutral 50.  Beside each line the
yardstick: smj_occupancy_to_distance on the lidar grid of the same shape with R = 0, read from profiles/distance_field_cost.txt.  The
share of cells with a finite potential is printed per map, so that a map on which nothing is reachable cannot pass for a cheap one.
Device events around `reps` back-to-back calls after a warm-up of every shape; the variants alternate round by round; the median of
the rounds is printed with its spread.  The head of the file is what the compiler reports for the two kernels, when hipcc is there, and
the sweeps the schedule takes on such maps at 128 x 128 and 129 x 128, as the host harness (tests/nav/nav_check.cpp, the kernel's own
functions in lock step) counts them, when g++ is there: the kernel itself does not report its sweeps.
Usage: python tools/gpu_navigation_cost.py [--envs 4096] [--rounds 3] [--reps 3] [--scene stretch_scene] [--out profiles/navigation_cost.txt]"""
import argparse
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors  # noqa: E402
from cost_common import LINES, alternate, resource_usage, say  # noqa: E402

NONE = 1 << 30


def harness_sweeps():
    """The sweep counts the host harness prints for its 128 x 128 and 129 x 128 maps."""
    gxx = shutil.which("g++")
    if gxx is None:
        say("sweeps: no g++ here, the host harness was not run")
        return
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "nav_check")
        subprocess.check_call([gxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "stretch_mujoco_amd", "csrc"), "-I", os.path.join(ROOT, "tests"),
                               os.path.join(ROOT, "tests", "nav", "nav_check.cpp"), "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True).stdout
    say("sweeps of the schedule, counted by the host harness (tests/nav/nav_check.cpp; the last sweep is the one that changes nothing):")
    for ln in out.splitlines():
        if re.search(r" 12[89] x 128 ", ln):
            say("  " + ln.rstrip())


def yardstick(nx, ny):
    """ms of smj_occupancy_to_distance, lidar scan, R 0, at this shape from profiles/distance_field_cost.txt, or None."""
    try:
        text = open(os.path.join(ROOT, "profiles", "distance_field_cost.txt")).read()
    except OSError:
        return None
    m = re.search(rf"grid {nx} x {ny} .*?lidar scan [^\n]*?: R 0\s+([0-9.]+) ", text, flags=re.S)
    return float(m.group(1)) if m else None


def serpentine(ny, nx):
    c = np.zeros((ny, nx), np.uint8)
    for k, y in enumerate(range(1, ny, 2)):
        c[y, :] = 254
        c[y, nx - 1 if k % 2 == 0 else 0] = 0
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scene", default="stretch_scene")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "navigation_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    B, dev = a.envs, "cuda:0"
    resource_usage("smj_nav.hip")
    harness_sweeps()
    sim = StretchBatchSimulator(num_envs=B, device=dev, scene=a.scene, solver="newton", sensors_to_use=[StretchSensors.base_lidar])
    sim.start(home=False)
    g = torch.Generator(device=dev).manual_seed(7)
    cr = torch.tensor(np.asarray(sim.model["actuator_ctrlrange"], np.float32), device=dev)
    sim.ctrl.copy_(cr[:, 0:1] + (cr[:, 1:2] - cr[:, 0:1]) * torch.rand(sim.nu, B, generator=g, device=dev))   # every env at its own pose
    sim.step(300)
    torch.cuda.synchronize()
    cell = 0.05
    say(f"navigation field cost: {B} envs, {a.scene}, cell 0.05 m, lethal 253, neutral 50; ms per call from device events, {a.reps} calls per window, "
        f"median [min .. max] of {a.rounds} alternating rounds; yardstick: smj_occupancy_to_distance, lidar scan, R 0, same shape (profiles/distance_field_cost.txt)")
    rng = np.random.default_rng(30)
    for nx, ny in ((64, 64), (128, 128), (256, 256)):
        n = nx * ny
        origin = (-nx * cell / 2 + 0.013, -ny * cell / 2 - 0.013)
        df = sim.pull_distance_field(max_distance=0.56, shape=(ny, nx), origin=origin, cell=cell)
        scan = df.inflated_cost(0.17, 0.56, 10.0).contiguous()
        iy, ix = int((0.0 - origin[1]) / cell), int((1.0 - origin[0]) / cell)      # 1 m ahead of the robot
        yy = torch.arange(ny, device=dev).view(1, ny, 1)
        xx = torch.arange(nx, device=dev).view(1, 1, nx)
        away = torch.where(scan == 0, (yy - iy) ** 2 + (xx - min(ix, nx - 1)) ** 2, 1 << 40)
        scan_goal = away.view(B, n).argmin(1).to(torch.int32).view(B, 1).contiguous()
        r30 = np.where(rng.random((ny, nx)) < 0.3, 254, rng.integers(0, 253, (ny, nx))).astype(np.uint8)
        free = np.flatnonzero(r30.ravel() < 253)
        maps = (("lidar scan", scan, scan_goal),
                ("empty", torch.zeros(B, ny, nx, dtype=torch.uint8, device=dev), torch.full((B, 1), (ny // 2) * nx + nx // 2, dtype=torch.int32, device=dev)),
                ("serpentine", torch.tensor(serpentine(ny, nx), device=dev).expand(B, ny, nx).contiguous(), torch.zeros(B, 1, dtype=torch.int32, device=dev)),
                ("30 % lethal", torch.tensor(r30, device=dev).expand(B, ny, nx).contiguous(),
                 torch.tensor(free[[0, len(free) // 2, len(free) - 1]].astype(np.int32), device=dev).expand(B, 3).contiguous()))
        pot = torch.empty(B, ny, nx, dtype=torch.int32, device=dev)
        nxt = torch.empty(B, ny, nx, dtype=torch.int32, device=dev)
        mode = "potential in LDS" if n <= 16384 else "potential relaxed in global memory"
        y = yardstick(nx, ny)
        say(f"  grid {nx} x {ny} ({mode}), {4.0 * B * n / 2**20:.0f} MiB per output; yardstick " + (f"{y:.4f} ms" if y is not None else "not on file"))
        for name, cost, goal in maps:
            def entry(with_next, cost=cost, goal=goal):
                rc = sim._L.smj_costmap_to_navigation(sim._ctx, ctypes.c_void_p(cost.data_ptr()), ctypes.c_void_p(goal.data_ptr()), goal.shape[1], nx, ny, 253, 50,
                                                      ctypes.c_void_p(pot.data_ptr()), ctypes.c_void_p(nxt.data_ptr()) if with_next else None, sim._stream())
                assert rc == 0

            res, med = alternate({"potential": lambda: entry(False), "potential + next": lambda: entry(True)}, a.rounds, a.reps)
            share = float((pot < NONE).sum()) / (B * n)
            times = "  ".join(f"{k} {med[k]:9.4f} [{min(res[k]):.4f} .. {max(res[k]):.4f}]" + (f" = {med[k] / y:.2f} x yardstick" if y else "") for k in res)
            say(f"    {name} ({100 * share:.1f} % of the cells reach a goal): " + times)
    sim.stop()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
