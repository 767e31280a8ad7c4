"""Cost of the lidar occupancy grids (smj_lidar_to_occupancy) at 4096 envs in stretch_scene, by the method of gpu_height_map_cost.py:
base frame, cell 0.05 m, a grid of one band (64 x 64) and one of four (128 x 128), range_limits (0.2, 5) and (0.2, 9.5), rays
without a return clearing.  Per call the time of (a) the entry, both layers; (b) the entry without the miss layer (hits alone);
(c) a torch composition of the HIT layer alone, written below: polar to Cartesian with the laser's pose in the base frame, the
range filter, floor, scatter_add_ -- the free-space layer has no torch counterpart short of a ray walk.  Device events around `reps`
back-to-back calls after a warm-up of every shape; the variants alternate round by round so that drift of the device affects them
alike; the median of the rounds is printed with its spread.  Then what feeds the map: step(1) with the lidar readout and without it
(two simulators of the same scene and state), the difference being one ray cast of 360 rays per env.
The head of the file is what the compiler reports for the kernel (-Rpass-analysis=kernel-resource-usage), when hipcc is there.
Usage: python tools/gpu_occupancy_cost.py [--envs 4096] [--rounds 5] [--reps 5] [--out profiles/occupancy_cost.txt]"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors  # noqa: E402
from cost_common import LINES, alternate, fmt, resource_usage, say  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occupancy_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    B, dev = a.envs, "cuda:0"
    resource_usage("smj_occ.hip")
    sims = {}
    for name, sensors in (("lidar", [StretchSensors.base_lidar]), ("none", [])):
        sim = StretchBatchSimulator(num_envs=B, device=dev, scene="stretch_scene", solver="newton", sensors_to_use=sensors)
        sim.start(home=False)
        g = torch.Generator(device=dev).manual_seed(7)
        cr = torch.tensor(np.asarray(sim.model["actuator_ctrlrange"], np.float32), device=dev)
        sim.ctrl.copy_(cr[:, 0:1] + (cr[:, 1:2] - cr[:, 0:1]) * torch.rand(sim.nu, B, generator=g, device=dev))   # every env at its own pose
        sim.step(300)
        sims[name] = sim
    torch.cuda.synchronize()
    sim = sims["lidar"]
    K = sim.nlidar
    scan = sim.lidar[:K]
    say(f"occupancy cost: {B} envs, stretch_scene, base frame, cell 0.05 m, {K} rays per env, rays without a return clear; ms per call from device "
        f"events, {a.reps} calls per window, median [min .. max] of {a.rounds} alternating rounds")
    say(f"  scan: {100 * float(((scan >= 0.2) & (scan <= 5.0)).float().mean()):.1f} % of the rays return within 0.2 .. 5 m, "
        f"{100 * float(((scan >= 0.2) & (scan <= 9.5)).float().mean()):.1f} % within 0.2 .. 9.5 m, {100 * float((scan < 0).float().mean()):.1f} % hit nothing, "
        f"{100 * float(((scan >= 0) & (scan < 0.2)).float().mean()):.1f} % end on the robot")
    base = int(sim.model["link_fused"][sim.names["body"].index("base_link")])
    sites = np.asarray(sim.model["sensor_lidar_site"]).reshape(-1)
    sb = np.asarray(sim.model["site_bodyid"]).reshape(-1)[sites]
    assert (sb == base).all(), "the torch composition below takes the laser as fixed in the base frame"
    o = torch.tensor(np.asarray(sim.model["site_pos"]).reshape(-1, 3)[sites][:, :2], dtype=torch.float32, device=dev)            # [K, 2]
    d = torch.tensor(np.asarray(sim.model["k_site_mat"]).reshape(-1, 3, 3)[sites][:, :2, 2], dtype=torch.float32, device=dev)    # [K, 2]
    cell = 0.05
    worst = 0.0
    for nx, ny in ((64, 64), (128, 128)):
        x0, y0 = -nx * cell / 2 + 0.013, -ny * cell / 2 - 0.013
        hit = torch.empty(B, ny, nx, dtype=torch.int32, device=dev)
        miss = torch.empty(B, ny, nx, dtype=torch.int32, device=dev)
        t_hit = torch.empty(B, ny * nx, dtype=torch.int32, device=dev)
        x0f, y0f, inv = np.float32(x0).item(), np.float32(y0).item(), (np.float32(1) / np.float32(cell)).item()
        for r_min, r_max in ((0.2, 5.0), (0.2, 9.5)):
            def entry(with_miss=True):
                rc = sim._L.smj_lidar_to_occupancy(sim._ctx, ctypes.c_void_p(scan.data_ptr()), B, base, x0, y0, cell, nx, ny, r_min, r_max, 1, 0,
                                                   ctypes.c_void_p(hit.data_ptr()), ctypes.c_void_p(miss.data_ptr()) if with_miss else None, sim._stream())
                assert rc == 0

            lo, hi = np.float32(r_min).item(), np.float32(r_max).item()

            def composed():
                r = scan.t()                                                   # [B, K]
                ok = (r >= lo) & (r <= hi)
                x, y = o[:, 0] + r * d[:, 0], o[:, 1] + r * d[:, 1]
                fx, fy = torch.floor((x - x0f) * inv), torch.floor((y - y0f) * inv)
                keep = ok & (fx >= 0) & (fx < nx) & (fy >= 0) & (fy < ny)
                idx = torch.where(keep, fy * nx + fx, torch.zeros_like(fx)).long()
                t_hit.zero_()
                t_hit.scatter_add_(1, idx, keep.to(torch.int32))
                return t_hit

            fns = {"entry": entry, "hits only": lambda: entry(False), "torch hits": composed}
            res, med = alternate(fns, a.rounds, a.reps)
            entry()
            th = composed().view(B, ny, nx)
            torch.cuda.synchronize()
            dcells = int((th != hit).sum())
            adds = int(hit.sum()) + int(miss.sum())
            bands = -(-ny // (4096 // nx))
            worst = max(worst, med["entry"])
            say(f"  grid {nx} x {ny} ({bands} band{'s' if bands > 1 else ''}), ranges {r_min:g} .. {r_max:g} m: " + fmt(res, med))
            say(f"    {adds / 1e6:.1f} M cell updates inside the grid ({adds / B:.0f} per env), {8.0 * B * nx * ny / 2**20:.0f} MiB stored: "
                f"{adds / (med['entry'] * 1e-3) / 1e9:.1f} G updates/s, {8.0 * B * nx * ny / (med['entry'] * 1e-3) / 1e12:.2f} TB/s of stores; "
                f"hit cells {int((hit > 0).sum())}, missed cells {int((miss > 0).sum())}; against the torch hit layer: {dcells} cells with another count "
                f"(end points on a cell edge)")
    # what feeds the map: one step with the lidar readout and one without
    fns = {"step(1) with lidar": lambda: sims["lidar"].step(1), "step(1) without": lambda: sims["none"].step(1)}
    res, med = alternate(fns, a.rounds, a.reps)
    cast = med["step(1) with lidar"] - med["step(1) without"]
    say("  " + fmt(res, med))
    say(f"  one lidar readout (the difference): {cast:.4f} ms; the dearest map above costs {worst:.4f} ms = {worst / cast:.2f} x the ray cast that feeds it"
        + ("  -- MORE than the ray cast" if worst > cast else ""))
    for s in sims.values():
        s.stop()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
