"""World-frame point clouds from both depth cameras for a batch of robots in the default scene (floor, table, two objects).

    python examples/point_cloud_batch.py [num_envs]

pull_point_cloud() deprojects the depth image on the device in one pass: [B, H', W', 3] metres, NaN rows where the pixel has no
depth (beyond the camera's limit).  Here: stride 4, world frame; per env the number of valid points and the height range of the
points on the table top.
"""
import sys

import torch

sys.path.insert(0, ".")
from stretch_mujoco_amd import StretchBatchSimulator, StretchCameras  # noqa: E402
from stretch_mujoco_amd.utils import render_K  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 4
sim = StretchBatchSimulator(num_envs=B, device="cuda:0", scene="stretch_scene", cameras_to_use=StretchCameras.depth())
sim.start()                                            # home pose: the wrist camera looks over the table
sim.move_to("head_pan", -1.57)                         # the head camera along the arm, down at the table
sim.move_to("head_tilt", -0.8)
sim.step(500)
for cam in StretchCameras.depth():
    pts = sim.pull_point_cloud(cam, frame="world", stride=4)          # renders the depth, then one fused pass
    valid = ~torch.isnan(pts).any(-1)                                  # [B, H', W']
    z = pts[..., 2]
    top = valid & (z > 0.45) & (z < 0.52) & (pts[..., 1] < -0.3)       # the table stands on the arm's side (-y); its top is 0.48 m up
    print(cam.name, "cloud", tuple(pts.shape))
    for e in range(B):
        t = z[e][top[e]]
        rng = f"{float(t.min()):.3f} .. {float(t.max()):.3f} m" if t.numel() else "not in view"
        print(f"  env {e}: valid points {int(valid[e].sum())} of {valid[e].numel()}, table-top heights {rng}")
st = StretchCameras.cam_d405_depth.initial_camera_settings
print("K that fits the d405 image (not cam_d405_K, which follows the sensor resolution):")
print(render_K(st.field_of_view_vertical_in_degrees, st.width, st.height))
sim.stop()
