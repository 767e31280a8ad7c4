"""Cost of the egocentric height maps (smj_depth_to_heightmap) at 4096 envs in stretch_scene: base frame, each depth camera at its own
size, both fused into one map (the first call overwrites, the second accumulates), for a grid of one band (64 x 64) and one of four
(128 x 128), cell 0.05 m.  Per fused map the time of (a) the entry, (b) the torch composition of the same map: pull_point_cloud(render=False)
per camera, then mask, floor, scatter_reduce_(amax) and scatter_add_ -- written below.  Device events around `reps` back-to-back maps
after a warm-up of every shape; the two alternate round by round so that drift of the device affects them alike; the median of the
rounds is printed with its spread.  Beside the times: the bytes a map has to move, derived from the shapes, not measured --
bands * 4 B per kept pixel, 8 B per cell, 8 B per cell more for the accumulating call -- and the rate that makes of the measured time.
The head of the file is what the compiler reports for the kernel (-Rpass-analysis=kernel-resource-usage), when hipcc is there.
Usage: python tools/gpu_height_map_cost.py [--envs 4096] [--rounds 5] [--reps 5] [--out profiles/height_map_cost.txt]"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stretch_mujoco_amd import StretchBatchSimulator  # noqa: E402
from stretch_mujoco_amd.enums import StretchCameras  # noqa: E402
from cost_common import LINES, resource_usage, say, timed  # noqa: E402

BAND_CELLS = 4096      # SMJ_HMAP_BAND_CELLS of csrc/smj_hmap.h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "height_map_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    B = a.envs
    resource_usage("smj_hmap.hip")
    cams = StretchCameras.depth()
    sim = StretchBatchSimulator(num_envs=B, device="cuda:0", scene="stretch_scene", solver="newton", cameras_to_use=cams)
    sim.start(home=False)
    g = torch.Generator(device="cuda:0").manual_seed(7)
    cr = torch.tensor(np.asarray(sim.model["actuator_ctrlrange"], np.float32), device="cuda:0")
    sim.ctrl.copy_(cr[:, 0:1] + (cr[:, 1:2] - cr[:, 0:1]) * torch.rand(sim.nu, B, generator=g, device="cuda:0"))   # every env at its own pose
    sim.step(300)
    sim.pull_camera_data()      # the depth images every variant reads
    torch.cuda.synchronize()
    say(f"height map cost: {B} envs, stretch_scene, base frame, cell 0.05 m, z band [-0.05, 2]; ms per FUSED map (both depth cameras) from device "
        f"events, {a.reps} maps per window, median [min .. max] of {a.rounds} alternating rounds")
    kept = 0
    for cam in cams:
        st = cam.initial_camera_settings
        d = sim._depth[cam]
        kept += B * st.width * st.height
        say(f"  {cam.name}: {st.width} x {st.height}, depth limit {cam.depth_limit:g} m, pixels with a depth {100 * float((d > 0).float().mean()):.1f} %")
    base = int(sim.model["link_fused"][sim.names["body"].index("base_link")])
    names = sim.names["camera"]
    lo, hi, cell = -0.05, 2.0, 0.05
    for nx, ny in ((64, 64), (128, 128)):
        x0, y0 = -nx * cell / 2 + 0.013, -ny * cell / 2 - 0.013
        height = torch.empty(B, ny, nx, dtype=torch.float32, device="cuda:0")
        count = torch.empty(B, ny, nx, dtype=torch.int32, device="cuda:0")

        def fused():
            for k, cam in enumerate(cams):
                st = cam.initial_camera_settings
                rc = sim._L.smj_depth_to_heightmap(sim._ctx, names.index(cam.camera_name_in_mjcf), st.width, st.height,
                                                   float(st.field_of_view_vertical_in_degrees), ctypes.c_void_p(sim._depth[cam].data_ptr()), 1, base,
                                                   x0, y0, cell, nx, ny, lo, hi, int(k > 0), ctypes.c_void_p(height.data_ptr()),
                                                   ctypes.c_void_p(count.data_ptr()), sim._stream())
                assert rc == 0

        x0f, y0f, inv = np.float32(x0).item(), np.float32(y0).item(), (np.float32(1) / np.float32(cell)).item()
        t_h = torch.empty(B, ny * nx, dtype=torch.float32, device="cuda:0")
        t_n = torch.empty(B, ny * nx, dtype=torch.int32, device="cuda:0")

        def composed():
            t_h.fill_(float("-inf"))
            t_n.zero_()
            for cam in cams:
                pts = sim.pull_point_cloud(cam, "base", stride=1, render=False)
                x, y, z = pts.unbind(-1)
                fx, fy = torch.floor((x - x0f) * inv), torch.floor((y - y0f) * inv)
                keep = (fx >= 0) & (fx < nx) & (fy >= 0) & (fy < ny) & (z >= lo) & (z <= hi)
                idx = torch.where(keep, fy * nx + fx, torch.zeros_like(fx)).long().view(B, -1)      # dropped points: cell 0 with -inf / 0
                t_h.scatter_reduce_(1, idx, torch.where(keep, z, torch.full_like(z, float("-inf"))).view(B, -1), "amax")
                t_n.scatter_add_(1, idx, keep.view(B, -1).to(torch.int32))
            return torch.where(t_n > 0, t_h, torch.full_like(t_h, float("nan")))

        fns = {"fused": fused, "torch": composed}
        for f in fns.values():      # warm-up of every shape
            f(); f()
        fused()
        th = composed().view(B, ny, nx)
        torch.cuda.synchronize()
        dcells = int((t_n.view(B, ny, nx) != count).sum())
        dh = float(torch.nan_to_num(th - height, nan=0.0).abs().max())
        res = {k: [] for k in fns}
        order = list(fns)
        for r in range(a.rounds):
            for k in order[r % 2:] + order[:r % 2]:
                res[k].append(timed(fns[k], a.reps))
        med = {k: float(np.median(v)) for k, v in res.items()}
        bands = -(-ny // (BAND_CELLS // nx))
        need = bands * 4.0 * kept + (8.0 + 16.0) * B * nx * ny
        say(f"  grid {nx} x {ny} ({bands} band{'s' if bands > 1 else ''}): " + "  ".join(f"{k} {med[k]:8.3f} [{min(res[k]):.3f} .. {max(res[k]):.3f}]" for k in order))
        say(f"    {kept / 1e6:.1f} M pixels x {bands} x 4 B + 24 B x {B * nx * ny / 1e6:.1f} M cells = {need / 2**30:.2f} GiB to move: the entry reaches "
            f"{need / (med['fused'] * 1e-3) / 1e12:.2f} TB/s of that traffic; torch / fused = {med['torch'] / med['fused']:.1f} x")
        say(f"    occupied cells {int((count > 0).sum())}; against the torch composition: {dcells} cells with another count (points on a cell "
            f"edge), max |height| difference {dh:.2e} m")
    sim.stop()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
