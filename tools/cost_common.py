"""What the cost tools of the perception entries share (gpu_point_cloud_cost.py, gpu_height_map_cost.py, gpu_occupancy_cost.py,
gpu_distance_field_cost.py, gpu_navigation_cost.py): the printed lines kept for the --out file, the compiler's resource report of a kernel source, device-event
timing of back-to-back calls, and variants alternated round by round so that drift of the device affects them alike."""
import os
import re
import shutil
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def resource_usage(source):
    """What the compiler reports for the kernels of csrc/`source`, with the Makefile's flags."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "stretch_mujoco_amd", "csrc")
    if not os.path.exists(hipcc):
        say("kernel resource usage: no hipcc here")
        return
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS \?= (.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    p = subprocess.run([hipcc, *flags, "-Rpass-analysis=kernel-resource-usage", "-c", source, "-o", os.devnull], cwd=csrc,
                       capture_output=True, text=True)
    say("kernel resource usage (hipcc -Rpass-analysis=kernel-resource-usage, the Makefile's flags):")
    for ln in p.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name: .*|VGPRs: .*|AGPRs: .*|TotalSGPRs: .*|ScratchSize.*|Occupancy.*|LDS Size.*|VGPRs Spill.*) \[-Rpass", ln)
        if m:
            t = m.group(1)
            say(("  " if t.startswith("Function") else "    ") + t)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, rounds, reps):
    for f in fns.values():      # warm-up of every shape
        f(); f()
    torch.cuda.synchronize()
    res = {k: [] for k in fns}
    order = list(fns)
    for r in range(rounds):
        k0 = r % len(order)
        for k in order[k0:] + order[:k0]:
            res[k].append(timed(fns[k], reps))
    return res, {k: float(np.median(v)) for k, v in res.items()}


def fmt(res, med):
    return "  ".join(f"{k} {med[k]:8.4f} [{min(res[k]):.4f} .. {max(res[k]):.4f}]" for k in res)
