"""Cost of the distance fields (smj_occupancy_to_distance) at 4096 envs, by the method of gpu_occupancy_cost.py: grids of 64 x 64,
128 x 128 and 256 x 256 cells of 0.05 m in the base frame, each with three inputs -- the occupancy grid of the scene's lidar scan
(range_limits 0.2 .. 5 m, rays without a return clearing), an empty grid, and a grid with one obstacle in a corner -- each with
R = 0 and R = 20, with and without the nearest buffer.  Beside it (a) smj_lidar_to_occupancy on the same grid, the call that
produced the input, and (b) the torch composition a user would write today: the obstacle cells of every env gathered into a padded
list, squared distances of every cell to every listed obstacle in chunks of envs that keep the [envs, cells, obstacles] tensor under
1 GiB, and min over the list.  The composition is timed on the first `--torch-envs` envs and scaled to all of them (it is linear
in the envs); its dist2 is compared with the entry's.  Device events around `reps` back-to-back calls after a warm-up of every
shape; the variants alternate round by round so that drift of the device affects them alike; the median of the rounds is printed
with its spread.  The head of the file is what the compiler reports for the kernel, when hipcc is there.
Usage: python tools/gpu_distance_field_cost.py [--envs 4096] [--rounds 5] [--reps 5] [--scene stretch_scene] [--out profiles/distance_field_cost.txt]"""
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

NONE = 1 << 30


def torch_field(mask, R):
    """dist2 [n, ny, nx] of bool masks by padded obstacle lists and chunked squared distances with min."""
    n, ny, nx = mask.shape
    C, dev = ny * nx, mask.device
    m = mask.view(n, C)
    count = m.sum(1)
    K = int(count.max())
    out = torch.full((n, C), NONE, dtype=torch.int32, device=dev)
    if K == 0:
        return out.view(n, ny, nx)
    order = torch.argsort(m.to(torch.int8), dim=1, descending=True, stable=True)[:, :K]      # the obstacle cells first, by index
    valid = torch.arange(K, device=dev)[None, :] < count[:, None]
    oy, ox = (order // nx).to(torch.int32), (order % nx).to(torch.int32)
    cy = torch.arange(ny, dtype=torch.int32, device=dev).repeat_interleave(nx)
    cx = torch.arange(nx, dtype=torch.int32, device=dev).repeat(ny)
    step = max(1, (1 << 30) // (4 * C * K))
    for e0 in range(0, n, step):
        e = slice(e0, e0 + step)
        d2 = (cy[None, :, None] - oy[e, None, :]) ** 2 + (cx[None, :, None] - ox[e, None, :]) ** 2
        out[e] = torch.where(valid[e, None, :], d2, NONE).min(-1).values
    if R > 0:
        out = torch.where(out > R * R, NONE, out)
    return out.view(n, ny, nx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-envs", type=int, default=64)
    ap.add_argument("--scene", default="stretch_scene")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_field_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    B, dev = a.envs, "cuda:0"
    resource_usage("smj_edt.hip")
    sim = StretchBatchSimulator(num_envs=B, device=dev, scene=a.scene, solver="newton", sensors_to_use=[StretchSensors.base_lidar])
    sim.start(home=False)
    g = torch.Generator(device=dev).manual_seed(7)
    cr = torch.tensor(np.asarray(sim.model["actuator_ctrlrange"], np.float32), device=dev)
    sim.ctrl.copy_(cr[:, 0:1] + (cr[:, 1:2] - cr[:, 0:1]) * torch.rand(sim.nu, B, generator=g, device=dev))   # every env at its own pose
    sim.step(300)
    torch.cuda.synchronize()
    K = sim.nlidar
    scan = sim.lidar[:K]
    base = int(sim.model["link_fused"][sim.names["body"].index("base_link")])
    cell, lim = 0.05, (0.2, 5.0)
    n_t = min(a.torch_envs, B)
    say(f"distance field cost: {B} envs, {a.scene}, base frame, cell 0.05 m, min_hits 1; ms per call from device events, {a.reps} calls per window, "
        f"median [min .. max] of {a.rounds} alternating rounds; torch: padded obstacle lists, chunked squared distances and min, timed on {n_t} envs and "
        f"scaled to {B}")
    for nx, ny in ((64, 64), (128, 128), (256, 256)):
        x0, y0 = -nx * cell / 2 + 0.013, -ny * cell / 2 - 0.013
        hit = torch.empty(B, ny, nx, dtype=torch.int32, device=dev)
        miss = torch.empty(B, ny, nx, dtype=torch.int32, device=dev)
        dist2 = torch.empty(B, ny, nx, dtype=torch.int32, device=dev)
        near = torch.empty(B, ny, nx, dtype=torch.int32, device=dev)

        def occupancy():
            rc = sim._L.smj_lidar_to_occupancy(sim._ctx, ctypes.c_void_p(scan.data_ptr()), B, base, x0, y0, cell, nx, ny, lim[0], lim[1], 1, 0,
                                               ctypes.c_void_p(hit.data_ptr()), ctypes.c_void_p(miss.data_ptr()), sim._stream())
            assert rc == 0

        occupancy()
        torch.cuda.synchronize()
        empty = torch.zeros_like(hit)
        corner = torch.zeros_like(hit)
        corner[:, ny - 1, nx - 1] = 1
        strips = -(-nx // -(-nx // -(-nx // (16384 // ny))))
        say(f"  grid {nx} x {ny} ({strips} strip{'s' if strips > 1 else ''}), {4.0 * B * nx * ny / 2**20:.0f} MiB per layer")
        res, med = alternate({"smj_lidar_to_occupancy": occupancy}, a.rounds, a.reps)
        t_occ = med["smj_lidar_to_occupancy"]
        say("    " + fmt(res, med))
        for name, src in (("lidar scan", hit), ("empty", empty), ("one corner", corner)):
            def entry(R, with_nearest, src=src):
                rc = sim._L.smj_occupancy_to_distance(sim._ctx, ctypes.c_void_p(src.data_ptr()), None, nx, ny, 1, 0, R, ctypes.c_void_p(dist2.data_ptr()),
                                                      ctypes.c_void_p(near.data_ptr()) if with_nearest else None, sim._stream())
                assert rc == 0

            fns = {f"R {R}{', nearest' if wn else ''}": (lambda R=R, wn=wn: entry(R, wn)) for R in (0, 20) for wn in (False, True)}
            res, med = alternate(fns, a.rounds, a.reps)
            ob = float((src > 0).sum()) / B
            say(f"    {name} ({ob:.1f} obstacle cells per env): " + fmt(res, med))
            line = []
            for R in (0, 20):
                sub = (src[:n_t] > 0)
                rt, mt = alternate({"torch": lambda: torch_field(sub, R)}, 2, 1)
                entry(R, False)
                same = bool(torch.equal(torch_field(sub, R), dist2[:n_t]))
                line.append(f"R {R}: {mt['torch'] * B / n_t:9.3f} ms ({mt['torch']:.3f} ms for {n_t} envs), dist2 {'equal' if same else 'DIFFERENT'}")
            say("      torch composition, " + "; ".join(line))
            if name == "lidar scan":
                worst = max(med.values())
                say(f"      the dearest variant costs {worst:.4f} ms = {worst / t_occ:.2f} x the occupancy call that produced the grid"
                    + ("  -- MORE than the ray walk" if worst > t_occ else ""))
    sim.stop()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
