"""Cost of the particle-filter update (smj_scan_to_particles) at 4096 envs, by the method of gpu_scanmatch_cost.py: the world-frame map
of the scene's first three envs tiled over all of them, 128 x 128 cells of 5 cm, its likelihood field of sigma 0.10 m, and per env P
particles spread over +-1 m and +-30 degrees round the simulator's own pose.
Timed, in the same run: the entry with P = 256, 1024 and 4096 on the scene's scan and when every ray returns, with the env's field
staged in LDS (the default) and gathered from global memory through L2 (option "mcl_stage_field" = 0: the weights are asserted equal);
the entry without resampling; smj_scan_to_pose's default search (21 x 21 x 21) beside it; and the same volume of look-ups -- P
particles x the counted returns -- as torch gathers on a few envs, scaled.  Statuses, counted returns and effective sample sizes are
printed, so that an empty scan or a lost filter cannot pass for a cheap one.  Device events around `reps` back-to-back calls after a
warm-up; the variants alternate round by round; the median of the rounds is printed with its spread.  The head of the file is what
the compiler reports for the kernel, when hipcc is there.
Usage: python tools/gpu_localize_cost.py [--envs 4096] [--rounds 3] [--reps 3] [--scene stretch_scene] [--out profiles/localize_cost.txt]"""
import argparse
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors  # noqa: E402
from stretch_mujoco_amd.utils import particle_noise, scan_angles, spread_particles  # noqa: E402
from cost_common import LINES, alternate, resource_usage, say  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scene", default="stretch_scene")
    ap.add_argument("--torch-envs", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "localize_cost.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    B, dev = a.envs, "cuda:0"
    resource_usage("smj_mcl.hip")
    sim = StretchBatchSimulator(num_envs=B, device=dev, scene=a.scene, solver="newton", sensors_to_use=[StretchSensors.base_lidar])
    sim.start(home=False)
    L, K = sim._L, sim.nlidar
    vp = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    n, cell, limits = 128, 0.05, (0.2, 5.0)
    origin = (-n * cell / 2 + 0.013, -n * cell / 2 - 0.029)
    say(f"localisation cost: {B} envs, {a.scene}, {K} rays per env, {n} x {n} cells of {cell} m, ranges {limits[0]} .. {limits[1]} m, likelihood field of sigma 0.10 m, span 4096, "
        f"min_points 30, with noise; ms per call from device events, {a.reps} calls per window, median [min .. max] of {a.rounds} alternating rounds")
    tile = lambda t: t[:3].repeat((B + 2) // 3, *([1] * (t.dim() - 1)))[:B].contiguous()
    grid = dict(frame="world", origin=origin, cell=cell, shape=(n, n), range_limits=limits)
    for k in range(4):      # a short drive: the map grows
        og = sim.pull_occupancy_grid(accumulate=k > 0, **grid)
        sim.set_base_velocity(0.2, 0.5)
        sim.step(100)
    sim.set_base_velocity(0.0, 0.0)
    sim.step(20)
    og = sim.pull_occupancy_grid(accumulate=True, **grid)
    og.hit.copy_(tile(og.hit))
    og.miss.copy_(tile(og.miss))
    field = sim.pull_distance_field(og).likelihood(0.10).contiguous()
    scan = tile(sim.lidar[:K].t().contiguous()).t().contiguous()      # [K, B], the scans of the first three envs
    truth = tile(sim.base_pose.t().contiguous()).t().contiguous()     # [3, B]
    sim.xpose.copy_(sim.xpose[:, torch.arange(B, device=dev) % 3].contiguous())
    dense = torch.full_like(scan, 1.5)                                # every ray returns
    body = sim._base_frame()[0]
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    draw = torch.randint(-(1 << 31), 1 << 31, (B,), device=dev, generator=gen).to(torch.int32)
    sets = {}
    for P in (256, 1024, 4096):
        sets[P] = dict(part=spread_particles(truth, (1.0, 1.0, 0.5236), P, generator=gen), noise=particle_noise(0.02, 0.01, (3, B, P), generator=gen),
                       out=torch.empty(3, B, P, device=dev), weight=torch.empty(B, P, dtype=torch.int32, device=dev))
    stat, pose = torch.empty(B, 8, dtype=torch.int32, device=dev), torch.empty(3, B, device=dev)

    def mcl(P, scan=scan, staged=1, resample=1):
        s = sets[P]

        def call():
            assert L.smj_set_option(sim._ctx, b"mcl_stage_field", float(staged)) == 0
            assert L.smj_scan_to_particles(sim._ctx, vp(scan), B, body, limits[0], limits[1], vp(field), n, n, origin[0], origin[1], cell, vp(s["part"]), P, vp(s["noise"]),
                                           vp(draw), 4096, 30, resample, vp(s["out"]), vp(s["weight"]), None, vp(stat), vp(pose), sim._stream()) == 0
        return call

    ang = scan_angles(device=dev)
    mpose, mbest = torch.empty(3, B, device=dev), torch.empty(B, 4, dtype=torch.int32, device=dev)
    mcells = torch.empty(B, 1, K, 2, dtype=torch.int32, device=dev)
    zero = torch.zeros(1, device=dev)

    def matcher(scan=scan):
        def call():
            assert L.smj_scan_to_pose(sim._ctx, vp(scan), B, body, limits[0], limits[1], vp(field), n, n, origin[0], origin[1], cell, vp(truth), vp(ang.angles), vp(ang.bias),
                                      21, 10, 10, 0, 30, vp(mpose), vp(mbest), None, None, sim._stream()) == 0
        return call

    # what is being timed, and that the two builds weigh alike
    for P in sets:
        mcl(P, staged=0)()
        torch.cuda.synchronize()
        global_w = sets[P]["weight"].clone()
        mcl(P)()
        torch.cuda.synchronize()
        say(f"  P {P}: status {stat[:3, 3].tolist()}, counted returns {stat[:3, 2].tolist()}, S_max {stat[:3, 1].tolist()}, effective sample size {stat[:3, 5].tolist()}, distinct "
            f"ancestors {stat[:3, 7].tolist()}; weights with the field in LDS and in global memory equal: {bool(torch.equal(global_w, sets[P]['weight']))}")
    returns = sum(stat[:3, 2].tolist()) / 3
    # the torch composition of P = 1024: the cells of the scan at the true pose, moved per particle by whole cells, gathered at once
    b, Pt = min(a.torch_envs, B), 1024
    assert L.smj_scan_to_pose(sim._ctx, vp(scan), B, body, limits[0], limits[1], vp(field), n, n, origin[0], origin[1], cell, vp(truth), vp(zero), None, 1, 0, 0, 0, 30,
                              vp(mpose), vp(mbest), None, vp(mcells), sim._stream()) == 0
    torch.cuda.synchronize()
    keep = mcells[0, 0, :, 0] != -32768                                                 # the counted returns of env 0: the volume of the scene's scan
    cells_b = mcells[:b, 0][:, keep].to(torch.int64)                                    # [b, returns, 2]
    shift = torch.randint(-20, 21, (b, Pt, 1, 2), device=dev, generator=gen)
    field_b = field[:b].reshape(b, -1)

    def torch_gather():
        c = cells_b[:, None] + shift                                                    # [b, Pt, returns, 2]
        on = (c[..., 0] >= 0) & (c[..., 0] < n) & (c[..., 1] >= 0) & (c[..., 1] < n)
        lin = (c[..., 1] * n + c[..., 0]) * on
        v = torch.gather(field_b, 1, lin.reshape(b, -1)).reshape(lin.shape)
        S = (v * on).sum(-1, dtype=torch.int32)
        return S.argmax(1), S

    variants = {}
    for P in sets:
        variants[f"P {P}"] = mcl(P)
        variants[f"P {P}, field in global memory"] = mcl(P, staged=0)
        variants[f"P {P}, all {K} rays return"] = mcl(P, dense)
        variants[f"P {P}, all {K} rays return, field in global memory"] = mcl(P, dense, staged=0)
    variants["P 1024, no resampling"] = mcl(1024, resample=0)
    variants["scan_to_pose, 21 x 21 x 21"] = matcher()
    variants[f"scan_to_pose, 21 x 21 x 21, all {K} rays return"] = matcher(dense)
    variants[f"torch gather, P {Pt}, {b} envs"] = torch_gather
    res, med = alternate(variants, a.rounds, a.reps)
    assert L.smj_set_option(sim._ctx, b"mcl_stage_field", 1.0) == 0
    for k in res:
        say(f"    {k:58s} {med[k]:9.4f} [{min(res[k]):.4f} .. {max(res[k]):.4f}]")
    for P in sets:
        say(f"    P {P}: field look-ups (particles x counted returns) {B * P * returns / 1e9:.2f} G per call, {B * P * returns / med[f'P {P}'] / 1e6:.0f} G look-ups/s; with all {K} rays "
            f"{B * P * K / 1e9:.2f} G, {B * P * K / med[f'P {P}, all {K} rays return'] / 1e6:.0f} G look-ups/s; LDS / global memory = "
            f"{med[f'P {P}'] / med[f'P {P}, field in global memory']:.2f} and {med[f'P {P}, all {K} rays return'] / med[f'P {P}, all {K} rays return, field in global memory']:.2f}")
    tg = med[f"torch gather, P {Pt}, {b} envs"]
    say(f"    torch gather of the volume of P {Pt} ({int(keep.sum())} returns): {tg:.3f} ms for {b} envs, {tg * B / b:.1f} ms scaled to {B} envs ({tg * B / b / med[f'P {Pt}']:.0f} x the entry)")
    say(f"    P 1024 / scan_to_pose's default search = {med['P 1024'] / med['scan_to_pose, 21 x 21 x 21']:.2f} (its candidates: 9261 poses on a lattice; here 1024 poses anywhere); "
        f"resampling costs {med['P 1024'] - med['P 1024, no resampling']:+.4f} ms of {med['P 1024']:.4f}")
    sim.stop()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
