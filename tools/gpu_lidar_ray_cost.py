"""Kernel times of the lidar scan and of both depth cameras, for comparing two builds of the library (the ray-primitive forms of
csrc/smj_ray.h against an earlier build): 4096 envs at random-action poses, stretch_empty and stretch_kitchen_robocasa.
   rocprofv3 --kernel-trace --output-format csv -d DIR -o smj -- python tools/gpu_lidar_ray_cost.py run      (SMJ_LIB_PATH picks the build)
   python tools/gpu_lidar_ray_cost.py stats DIR TAG          one line per scene and kernel: calls, median and spread of the kernel time
The scenes run one after the other in one process; `run` launches a marker fill between them so that `stats` can tell them apart."""
import collections
import csv
import glob
import os
import sys

SCENES = ("stretch_empty", "stretch_kitchen_robocasa")
KERNELS = ("smj_lidar_kernel", "smj_depth_prepass", "smj_depth_kernel", "smj_meshlet_kernel")
B, SCANS, RENDERS = 4096, 30, 8


def run():
    import numpy as np
    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from stretch_mujoco_amd import StretchBatchSimulator, StretchSensors
    from stretch_mujoco_amd.enums import StretchCameras

    for scene in SCENES:
        sim = StretchBatchSimulator(num_envs=B, device="cuda:0", scene=scene, sensors_to_use=StretchSensors.all(), cameras_to_use=StretchCameras.depth())
        sim.start(home=False)
        g = torch.Generator(device=sim.device).manual_seed(1234)
        lo = torch.tensor(np.asarray(sim.model["actuator_ctrlrange"], np.float32)[:, 0], device=sim.device)
        hi = torch.tensor(np.asarray(sim.model["actuator_ctrlrange"], np.float32)[:, 1], device=sim.device)
        for _ in range(4):
            sim.ctrl[:] = lo[:, None] + (hi - lo)[:, None] * torch.rand(sim.nu, B, generator=g, device=sim.device)
            sim.step(50)
        for _ in range(SCANS):      # one lidar scan per call
            sim.step(1)
        for _ in range(RENDERS):
            cd = sim.pull_camera_data()
        torch.cuda.synchronize()
        lidar = sim.pull_sensor_data().lidar
        print(scene, "lidar checksum %.6e" % float(lidar.double().sum()), "depth checksums", ["%.6e" % float(getattr(cd, c.name).double().sum()) for c in StretchCameras.depth()], flush=True)
        sim.stop()


def stats(directory, tag):
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    # every step call scans once, the same number of times in each scene: the scenes split at the middle of the lidar kernel's calls
    lid = [r for r in rows if "smj_lidar_kernel" in r["Kernel_Name"]]
    split = int(lid[len(lid) // 2]["Start_Timestamp"])
    for si, scene in enumerate(SCENES):
        d = collections.defaultdict(list)
        for r in rows:
            if (int(r["Start_Timestamp"]) >= split) != bool(si):
                continue
            for k in KERNELS:
                if k in r["Kernel_Name"]:
                    d[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        for k in KERNELS:
            v = sorted(d[k][-(SCANS if k == "smj_lidar_kernel" else 2 * RENDERS):])      # the timed calls are the last of each scene
            if v:
                print(f"{tag:8s} {scene:26s} {k:20s} calls {len(v):3d}  median {v[len(v) // 2]:9.1f} us  min {v[0]:9.1f}  max {v[-1]:9.1f}", flush=True)


if __name__ == "__main__":
    run() if sys.argv[1] == "run" else stats(sys.argv[2], sys.argv[3])
