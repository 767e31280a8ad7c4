"""Cost of the scan matcher (smj_scan_to_pose) at 4096 envs, by the method of gpu_drive_cost.py: the world-frame map of the scene's
lidar accumulated over a short drive, the maps of the first three envs tiled over all of them, its distance field and likelihood
field (sigma 0.10) on 128 x 128 cells; the scan of the last step matched from priors three cells, two cells and four half-degrees
off the simulator's pose.  Timed: the default search (21 rotations x 21 x 21 shifts) with pose and best alone and with score_dev and
cell_dev too, and on a scan whose every ray returns; the largest search (64 x 65 x 65); the default search on 256 x 256 cells; and, in the same run, smj_lidar_to_occupancy
and smj_costmap_to_navigation on the 128 x 128 grid, and a plain torch gather of the default volume -- what a user would write
without the entry -- at a batch that fits memory, scaled to the envs.  The statuses, the winners and the returns per env are printed,
so that a scan without returns cannot pass for a cheap one.  Device events around `reps` back-to-back calls after a warm-up; the
variants alternate round by round; the median of the rounds is printed with its spread.  The head of the file is what the compiler
reports for the kernel, when hipcc is there.
Usage: python tools/gpu_scanmatch_cost.py [--envs 4096] [--rounds 3] [--reps 3] [--scene stretch_scene] [--torch-envs 16] [--out profiles/scanmatch_cost.txt]"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors  # noqa: E402
from stretch_mujoco_amd.utils import ScanAngles, scan_angles  # noqa: E402
from cost_common import LINES, alternate, resource_usage, say  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scene", default="stretch_scene")
    ap.add_argument("--torch-envs", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scanmatch_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    B, dev = a.envs, "cuda:0"
    resource_usage("smj_match.hip")
    sim = StretchBatchSimulator(num_envs=B, device=dev, scene=a.scene, solver="newton", sensors_to_use=[StretchSensors.base_lidar])
    sim.start(home=False)
    L, K = sim._L, sim.nlidar
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    cell, limits = 0.05, (0.2, 5.0)
    say(f"scan matching cost: {B} envs, {a.scene}, {K} rays per env, cell {cell} m, ranges {limits[0]} .. {limits[1]} m, likelihood field of sigma 0.10 m, min_points 30; ms per "
        f"call from device events, {a.reps} calls per window, median [min .. max] of {a.rounds} alternating rounds")
    tile = lambda t: t[:3].repeat((B + 2) // 3, *([1] * (t.dim() - 1)))[:B].contiguous()
    fields = {}
    for n in (128, 256):
        origin = (-n * cell / 2 + 0.013, -n * cell / 2 - 0.029)
        grid = dict(frame="world", origin=origin, cell=cell, shape=(n, n), range_limits=limits)
        if n == 128:
            for k in range(4):      # a short drive: the map grows
                og = sim.pull_occupancy_grid(accumulate=k > 0, **grid)
                sim.set_base_velocity(0.2, 0.5)
                sim.step(100)
            sim.set_base_velocity(0.0, 0.0)
            sim.step(20)
        og = sim.pull_occupancy_grid(accumulate=n == 128, **grid)
        og.hit.copy_(tile(og.hit))
        og.miss.copy_(tile(og.miss))
        df = sim.pull_distance_field(og)
        fields[n] = (origin, df.likelihood(0.10).contiguous(), og, df)
    scan = tile(sim.lidar[:K].t().contiguous()).t().contiguous()      # [K, B], the scans of the first three envs
    truth = tile(sim.base_pose.t().contiguous()).t().contiguous()     # [3, B]
    prior = (truth + torch.tensor([[3 * cell], [-2 * cell], [4 * 0.008727]], device=dev)).contiguous()
    body = sim._base_frame()[0]
    returns = ((scan >= limits[0]) & (scan <= limits[1])).sum(0)[:3].tolist()
    pose, best = torch.empty(3, B, device=dev), torch.empty(B, 4, dtype=torch.int32, device=dev)

    def matcher(n, ang, wx, wy, full, scan=scan):
        origin, field, _, _ = fields[n]
        T = ang.angles.shape[0]
        score = torch.empty(B, T, 2 * wy + 1, 2 * wx + 1, dtype=torch.int32, device=dev) if full else None
        cells = torch.empty(B, T, K, 2, dtype=torch.int32, device=dev) if full else None

        def call():
            assert L.smj_scan_to_pose(sim._ctx, vp(scan), B, body, limits[0], limits[1], vp(field), n, n, origin[0], origin[1], cell, vp(prior), vp(ang.angles), vp(ang.bias),
                                      T, wx, wy, 0, 30, vp(pose), vp(best), vp(score), vp(cells), sim._stream()) == 0
        call.outputs = (score, cells)
        return call

    default = scan_angles(device=dev)
    largest = ScanAngles(((torch.arange(64, device=dev) - 32) * 0.004).to(torch.float32), torch.zeros(64, dtype=torch.int32, device=dev))
    assert default.angles.shape[0] == 21
    og128, df128 = fields[128][2], fields[128][3]
    cost = df128.inflated_cost(0.17, 0.56, 10.0).contiguous()
    ahead = torch.stack((truth[0] + torch.cos(truth[2]), truth[1] + torch.sin(truth[2])), 1)
    nf = sim.pull_navigation_field(ahead, cost, cell=cell, origin=fields[128][0])
    goal, scratch = nf.goal.contiguous(), torch.empty_like(nf.potential)
    hit, miss = torch.empty_like(og128.hit), torch.empty_like(og128.miss)

    def occupancy():
        o = fields[128][0]
        assert L.smj_lidar_to_occupancy(sim._ctx, vp(scan), B, -2, o[0], o[1], cell, 128, 128, limits[0], limits[1], 1, 0, vp(hit), vp(miss), sim._stream()) == 0

    def navigation():
        assert L.smj_costmap_to_navigation(sim._ctx, vp(cost), vp(goal), 1, 128, 128, 253, 50, vp(scratch), None, sim._stream()) == 0

    # the torch composition: the device's own cells of the default search, gathered over every shift at once
    b = min(a.torch_envs, B)
    full = matcher(128, default, 10, 10, True)
    full()
    torch.cuda.synchronize()
    winners = f"status {best[:3, 3].tolist()}, winner {best[:3, 0].tolist()}, J {best[:3, 1].tolist()}, counted returns {best[:3, 2].tolist()} (in range {returns})"
    cells_b, field_b = full.outputs[1][:b].to(torch.int64), fields[128][1][:b].reshape(b, -1)
    d = torch.arange(-10, 11, device=dev)

    def torch_gather():
        sx = cells_b[..., 0][:, :, None, None, :] + d[None, None, None, :, None]      # [b, T, 1, WX, K]
        sy = cells_b[..., 1][:, :, None, None, :] + d[None, None, :, None, None]      # [b, T, WY, 1, K]
        on = (sx >= 0) & (sx < 128) & (sy >= 0) & (sy < 128)
        lin = (sy * 128 + sx) * on
        v = torch.gather(field_b, 1, lin.reshape(b, -1)).reshape(lin.shape)
        J = (v * on).sum(-1, dtype=torch.int32)
        return J.reshape(b, -1).argmax(1), J

    first, J = torch_gather()
    torch.cuda.synchronize()
    same = bool(torch.equal(J, full.outputs[0][:b])) and bool(torch.equal(first.to(torch.int32), best[:b, 0]))
    dense = torch.full_like(scan, 1.5)      # every ray returns: four times the points of the scene's scan
    variants = {"pose and best": matcher(128, default, 10, 10, False), "with score and cell": full, f"all {K} rays return": matcher(128, default, 10, 10, False, dense), "64 x 65 x 65": matcher(128, largest, 32, 32, False),
                "256 x 256": matcher(256, default, 10, 10, False), "occupancy": occupancy, "navigation": navigation, f"torch gather, {b} envs": torch_gather}
    res, med = alternate(variants, a.rounds, a.reps)
    say(f"  128 x 128, default search 21 x 21 x 21 ({winners}):")
    for k in res:
        say(f"    {k:24s} {med[k]:9.4f} [{min(res[k]):.4f} .. {max(res[k]):.4f}]")
    n = sum(best[:3, 2].tolist()) / 3      # `best` holds the last call of the alternation: the scene's scan
    say(f"    field look-ups (candidates x counted returns): {B * 21 * 441 * n / 1e9:.2f} G per default call, {B * 21 * 441 * n / med['pose and best'] / 1e6:.0f} G look-ups/s; "
        f"with all {K} rays {B * 21 * 441 * K / 1e9:.2f} G, {B * 21 * 441 * K / med[f'all {K} rays return'] / 1e6:.0f} G look-ups/s; the largest search "
        f"{B * 64 * 4225 * n / 1e9:.1f} G, {B * 64 * 4225 * n / med['64 x 65 x 65'] / 1e6:.0f} G look-ups/s")
    tg = med[f"torch gather, {b} envs"]
    say(f"    torch gather of the same volume: {tg:.3f} ms for {b} envs, {tg * B / b:.1f} ms scaled to {B} envs ({tg * B / b / med['with score and cell']:.0f} x the entry with "
        f"score and cell); scores and winners equal the entry's: {same}")
    say(f"    the match / the occupancy pass = {med['pose and best'] / med['occupancy']:.2f}, / the navigation pass = {med['pose and best'] / med['navigation']:.3f}")
    sim.stop()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
