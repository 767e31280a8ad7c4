"""Cost of the contact readout (SMJ_READ_CONTACTS): ms per step(50) and per step(1) at 4096 envs, with and without contacts=True, in
stretch_empty and stretch_kitchen_robocasa (Newton, random actions held per call).  The two settings alternate call by call so that
drift of the device affects both alike; the median of each is printed with its spread (min .. max of the per-round medians).
Usage: python tools/contact_readout_cost.py [--envs 4096] [--rounds 5]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stretch_mujoco_amd import StretchBatchSimulator  # noqa: E402


def _timed(sim, n, reps, g, lo, hi):
    out = []
    for _ in range(reps):
        sim.ctrl.copy_(lo + (hi - lo) * torch.rand(sim.nu, sim.num_envs, generator=g, device=sim.device))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sim.step(n)
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    print(f"contact readout cost: {a.envs} envs, Newton, {a.rounds} alternating rounds; ms per call, median [min .. max of the rounds]")
    for scene in ("stretch_empty", "stretch_kitchen_robocasa"):
        sims = {}
        for on in (False, True):
            s = StretchBatchSimulator(num_envs=a.envs, device="cuda:0", scene=scene, solver="newton", contacts=on)
            s.start(home=False)
            s.step(200)
            sims[on] = s
        cr = torch.tensor(np.asarray(sims[False].model["actuator_ctrlrange"], np.float32), device="cuda:0")
        lo, hi = cr[:, 0:1], cr[:, 1:2]
        res = {(on, n): [] for on in (False, True) for n in (50, 1)}
        for r in range(a.rounds):
            for n, reps in ((50, 4), (1, 40)):
                for on in ((False, True) if r % 2 == 0 else (True, False)):
                    g = torch.Generator(device="cuda:0").manual_seed(100 * r + n)
                    res[(on, n)].append(_timed(sims[on], n, reps, g, lo, hi))
        for n in (50, 1):
            off, on = np.array(res[(False, n)]), np.array(res[(True, n)])
            print(f"  {scene:26s} step({n:2d}): off {np.median(off):8.3f} [{off.min():.3f} .. {off.max():.3f}]  "
                  f"on {np.median(on):8.3f} [{on.min():.3f} .. {on.max():.3f}]  overhead {100 * (np.median(on) / np.median(off) - 1):+.1f} %")
        cap = sims[True].contact_cap
        print(f"  {scene:26s} records: {cap} x 96 B per env = {a.envs * cap * 96 / 2**20:.1f} MiB per call at {a.envs} envs; "
              f"mean contacts per env at the last call {sims[True].info[1].float().mean().item():.1f}")
        for s in sims.values():
            s.stop()


if __name__ == "__main__":
    main()
