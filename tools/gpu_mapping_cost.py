"""Cost of the mapping step (smj_scan_to_map) at 4096 envs, by the method of gpu_scanmatch_cost.py: the scene's lidar scan after a
short drive, the scans and poses of the first three envs tiled over all of them, a 128 x 128 grid of 5 cm cells in the world frame.
Timed, in the same run and on the same scans and grid: smj_scan_to_map at the simulator's own pose (SMJ_SLOT_BASE_POSE) with ranges
to 5 m and to 9.5 m; the same without the miss layer, with cell_dev, and with a gate that skips half of the envs (every other one, and a random half); and beside it
smj_lidar_to_occupancy in the world frame, which walks the same rays from the pose it reads out of XPOSE -- the yardstick: the new
entry does the same walk plus one 2-D transform per ray, and less work off the band.  The statuses and the rays kept per env are
printed, so that an empty scan cannot pass for a cheap one, and so is the share of cells on which the two entries agree (they form the
cells by different float paths).  Device events around `reps` back-to-back calls after a warm-up; the variants alternate round by
round; the median of the rounds is printed with its spread.  The head of the file is what the compiler reports for the kernel, when
hipcc is there.
Usage: python tools/gpu_mapping_cost.py [--envs 4096] [--rounds 5] [--reps 20] [--scene stretch_scene] [--out profiles/mapping_cost.txt]"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors  # noqa: E402
from cost_common import LINES, alternate, resource_usage, say  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scene", default="stretch_scene")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mapping_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    B, dev = a.envs, "cuda:0"
    resource_usage("smj_map.hip")
    sim = StretchBatchSimulator(num_envs=B, device=dev, scene=a.scene, solver="newton", sensors_to_use=[StretchSensors.base_lidar])
    sim.start(home=False)
    L, K = sim._L, sim.nlidar
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    n, cell = 128, 0.05
    origin = (-n * cell / 2 + 0.013, -n * cell / 2 - 0.029)
    say(f"mapping cost: {B} envs, {a.scene}, {K} rays per env, {n} x {n} cells of {cell} m, no_return_clears 1, accumulate 0; ms per call from device events, "
        f"{a.reps} calls per window, median [min .. max] of {a.rounds} alternating rounds")
    sim.set_base_velocity(0.2, 0.5)      # a short drive, as the scan matcher's cost run
    sim.step(400)
    sim.set_base_velocity(0.0, 0.0)
    sim.step(20)
    body = sim._base_frame()[0]
    # the first three envs tiled over all of them: scans, planar poses, and the XPOSE array smj_lidar_to_occupancy reads its pose from
    idx = torch.arange(B, device=dev) % 3
    scan = sim.lidar[:K][:, idx].contiguous()                 # [K, B]
    pose = sim.base_pose[:, idx].contiguous()                 # [3, B]
    sim.xpose.copy_(sim.xpose[:, idx].contiguous())
    hit, miss = (torch.empty(B, n, n, dtype=torch.int32, device=dev) for _ in range(2))
    hit_o, miss_o = (torch.empty(B, n, n, dtype=torch.int32, device=dev) for _ in range(2))
    info = torch.empty(B, 4, dtype=torch.int32, device=dev)
    cells = torch.empty(B, K, 4, dtype=torch.int32, device=dev)
    # two gates that skip half of the envs: every other env, and a seeded random half.  With four bands per env the workgroups of
    # every other env are blocks 4 .. 7 of every eight, and blocks are dealt round-robin over the chip's eight XCDs: that gate idles
    # four XCDs and saves nothing; the random half spreads
    half = (torch.arange(B, device=dev) % 2).to(torch.int32).contiguous()
    scattered = torch.zeros(B, dtype=torch.int32)
    scattered[torch.randperm(B, generator=torch.Generator().manual_seed(7))[:B // 2]] = 1
    scattered = scattered.to(dev)

    def mapping(r_max, with_miss=True, with_cells=False, gate=None):
        def call():
            assert L.smj_scan_to_map(sim._ctx, vp(scan), B, body, 0.2, r_max, vp(pose), vp(gate), 1, origin[0], origin[1], cell, n, n, 1, 0, vp(hit),
                                     vp(miss) if with_miss else None, vp(info), vp(cells) if with_cells else None, sim._stream()) == 0
        return call

    def occupancy(r_max, with_miss=True):
        def call():
            assert L.smj_lidar_to_occupancy(sim._ctx, vp(scan), B, -2, origin[0], origin[1], cell, n, n, 0.2, r_max, 1, 0, vp(hit_o), vp(miss_o) if with_miss else None,
                                            sim._stream()) == 0
        return call

    variants = {}
    for r_max in (5.0, 9.5):
        variants[f"map, to {r_max} m"] = mapping(r_max)
        variants[f"map, to {r_max} m, no miss layer"] = mapping(r_max, with_miss=False)
        variants[f"map, to {r_max} m, with cell_dev"] = mapping(r_max, with_cells=True)
        variants[f"map, to {r_max} m, every other env gated"] = mapping(r_max, gate=half)
        variants[f"map, to {r_max} m, a random half gated"] = mapping(r_max, gate=scattered)
        variants[f"occupancy(world), to {r_max} m"] = occupancy(r_max)
        variants[f"occupancy(world), to {r_max} m, no miss layer"] = occupancy(r_max, with_miss=False)
    # what is being timed: the rays kept and the agreement of the two entries, per range limit
    for r_max in (5.0, 9.5):
        mapping(r_max, with_cells=True)()
        occupancy(r_max)()
        torch.cuda.synchronize()
        same = [round(float(((hit[:3] == hit_o[:3]) & (miss[:3] == miss_o[:3])).float().mean((1, 2))[e]), 4) for e in range(3)]
        say(f"  to {r_max} m: info (status, returns, clearing rays, dropped by a guard) of the first three envs {info[:3].tolist()}; hit cells {(hit[:3] > 0).sum((1, 2)).tolist()}, "
            f"cells visited {((hit[:3] + miss[:3]) > 0).sum((1, 2)).tolist()}, adds {(hit[:3] + miss[:3]).sum((1, 2)).tolist()} "
            f"(occupancy(world): {(hit_o[:3] + miss_o[:3]).sum((1, 2)).tolist()}); share of cells equal to occupancy(world) {same}")
    for name, gate in (("every other env", half), ("a random half", scattered)):
        mapping(5.0, gate=gate)()
        torch.cuda.synchronize()
        say(f"  {name} gated: statuses of the first eight envs {info[:8, 0].tolist()}, integrated {int((info[:, 0] == 0).sum())} of {B}")
    res, med = alternate(variants, a.rounds, a.reps)
    for k in res:
        say(f"    {k:46s} {med[k]:9.4f} [{min(res[k]):.4f} .. {max(res[k]):.4f}]")
    for r_max in (5.0, 9.5):
        m, o = med[f"map, to {r_max} m"], med[f"occupancy(world), to {r_max} m"]
        say(f"    to {r_max} m: map / occupancy(world) = {m / o:.3f} ({m - o:+.4f} ms); without the miss layer {med[f'map, to {r_max} m, no miss layer'] / med[f'occupancy(world), to {r_max} m, no miss layer']:.3f}")
    say(f"    the longer range costs the map x {med['map, to 9.5 m'] / med['map, to 5.0 m']:.2f}, the occupancy entry x {med['occupancy(world), to 9.5 m'] / med['occupancy(world), to 5.0 m']:.2f}")
    sim.stop()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
