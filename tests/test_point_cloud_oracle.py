"""Organised point clouds, CPU side: the fp64 restatement (tests/point_cloud_ref.py) applied to the oracle's depth images.  The floor
seen by a camera must come out at world z = 0, the frames must chain, utils.render_K must project every point back to the centre
of the pixel it came from, and the NaN rows are the zeros of the limited render.  37 x 23 images of both depth cameras in the empty
scene and in scene.xml."""
import os

import numpy as np
import pytest

from conftest import MODELS, home_qpos
from oracle.oracle import Oracle
from point_cloud_ref import deproject
from stretch_mujoco_amd import model_blob
from stretch_mujoco_amd.utils import render_K

D405, D435 = 1, 3
W, H = 37, 23
FOVY = {D405: 58.0, D435: 42.0}


@pytest.fixture(scope="module", params=["stretch_empty", "stretch_scene"])
def posed(request):
    with open(os.path.join(MODELS, request.param + ".smjb"), "rb") as f:
        blob = f.read()
    m = model_blob.loads(blob)
    o = Oracle(blob)
    o.arr("qpos")[:] = home_qpos(m["qpos0"])
    o.forward()
    views = {}
    for cam in (D405, D435):    # rendered once, shared by the tests below and left unchanged
        views[cam] = dict(raw=o.render_depth(cam, W, H, FOVY[cam], 0.0), gid=o.render_geomid(cam, W, H, FOVY[cam])[0],
                          xpos=o.arr("cam_xpos").reshape(-1, 3)[cam].copy(), xmat=o.arr("cam_xmat").reshape(-1, 3, 3)[cam].copy())
    views[D435]["lim"] = o.render_depth(D435, W, H, FOVY[D435], 10.0)
    import json
    names = json.loads(model_blob.get_str(m, "names_json"))["body"]
    fb = int(m["link_fused"][names.index("base_link")])
    base = (o.arr("xpos").reshape(-1, 3)[fb].copy(), o.arr("xmat").reshape(-1, 3, 3)[fb].copy())
    return m, views, base


@pytest.mark.parametrize("cam", [D405, D435])
def test_floor_pixels_lie_in_the_world_plane(posed, cam):
    """Every pixel whose first geom is the plane deprojects to |z| <= 1e-6 + 1e-6 d in the world frame (the bound of
    test_depth_oracle.test_plane_closed_form), at depths up to the far plane's 40 m; at least 200 such pixels per image."""
    m, views, _ = posed
    v = views[cam]
    pts = deproject(v["raw"], W, H, FOVY[cam], 1, v["xpos"], v["xmat"], "world")
    planes = np.where(np.asarray(m["geom_type"]) == 0)[0]
    floor = np.isin(v["gid"], planes)
    print("floor pixels", int(floor.sum()), "worst |z|", float(np.abs(pts[floor][:, 2]).max()), "deepest", float(v["raw"][floor].max()))
    assert floor.sum() >= 200
    assert np.all(np.abs(pts[floor][:, 2]) <= 1e-6 + 1e-6 * v["raw"][floor])


@pytest.mark.parametrize("cam", [D405, D435])
@pytest.mark.parametrize("stride", [1, 3])
def test_frames_chain_and_render_K_projects_back(posed, cam, stride):
    _, views, (bp, bm) = posed
    v = views[cam]
    c = deproject(v["raw"], W, H, FOVY[cam], stride, None, None, "camera")
    w = deproject(v["raw"], W, H, FOVY[cam], stride, v["xpos"], v["xmat"], "world")
    b = deproject(v["raw"], W, H, FOVY[cam], stride, v["xpos"], v["xmat"], "body", bp, bm)
    hp, wp = -(-H // stride), -(-W // stride)
    assert c.shape == w.shape == b.shape == (hp, wp, 3) and np.isfinite(c).all()
    # camera -> world -> base, by hand: the optical frame is the MuJoCo camera frame with y and z flipped
    w2 = (c * [1, -1, -1]) @ v["xmat"].T + v["xpos"]
    b2 = (w2 - bp) @ bm
    scale = 1 + np.abs(w).max()
    assert np.abs(w2 - w).max() <= 1e-12 * scale and np.abs(b2 - b).max() <= 1e-12 * scale
    back = ((b @ bm.T + bp) - v["xpos"]) @ v["xmat"] * [1, -1, -1]
    assert np.abs(back - c).max() <= 1e-12 * scale
    # projection with the matrix that fits the image: the centre of the pixel each cell was taken from ...
    i, j = np.meshgrid(np.arange(hp), np.arange(wp), indexing="ij")
    uvw = c @ render_K(FOVY[cam], W, H).T
    assert np.abs(uvw[..., 0] / uvw[..., 2] - (stride * j + 0.5)).max() < 1e-9
    assert np.abs(uvw[..., 1] / uvw[..., 2] - (stride * i + 0.5)).max() < 1e-9
    # ... and with the grid's own matrix the centre of the cell
    uvw = c @ render_K(FOVY[cam], W, H, stride).T
    assert np.abs(uvw[..., 0] / uvw[..., 2] - (j + 0.5)).max() < 1e-9 and np.abs(uvw[..., 1] / uvw[..., 2] - (i + 0.5)).max() < 1e-9
    assert np.array_equal(c[..., 2], v["raw"][::stride, ::stride].astype(np.float64))    # z of the optical frame is the depth


def test_nan_rows_are_the_zeros_of_the_limited_render(posed):
    _, views, _ = posed
    v = views[D435]
    lim = v["lim"]
    assert (lim == 0).any() and (lim > 0).any()
    for frame in ("camera", "world"):
        pts = deproject(lim, W, H, FOVY[D435], 1, v["xpos"], v["xmat"], frame)
        nan = np.isnan(pts)
        assert np.array_equal(nan.all(-1), lim == 0) and np.array_equal(nan.any(-1), lim == 0)
    for bad in (np.inf, -1.0, np.nan):
        d = lim.copy(); d[3, 5] = bad
        assert np.isnan(deproject(d, W, H, FOVY[D435], 1, v["xpos"], v["xmat"], "world")[3, 5]).all()
