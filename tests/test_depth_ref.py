"""tests/depth_ref.py on cases a hand can compute, then the fp64 oracle (oracle/smj_oracle.c smjo_render_depth / smjo_render_geomid)
against it on every scene of tests/depth_rig.py, then the builders' own conditions.  The oracle stores fp32 images, so the bound is
2 ulp of the fp32 value; hit or miss and the geom id are exact off the grazing pixels (depth_rig.compare).  CPU only."""
import math

import numpy as np
import pytest

import depth_ref
import depth_rig
import ray_ref
from ray_rig import body, geom, pose

TH = math.tan(math.radians(45.0))      # fovy 90 degrees: tan(fovy / 2) = 1


def _view(world, eye=(0, 0, 0), width=3, height=3, znear=0.02, zfar=12.0, meshes=None, quat=(1, 0, 0, 0)):
    """A 90-degree camera at `eye`, identity frame unless `quat`: it looks down -z, x right, y up.  3 x 3 pixels: the centre pixel's
    ray is (0, 0, -1), the corner pixels' rays are (+-2/3, +-2/3, -1)."""
    scene = dict(world=list(world), bodies=[body("cam")], cameras=[depth_rig.camera(0, fovy=90.0, quat=quat)], meshes=meshes or {})
    return depth_ref.view(scene, [pose(eye, [1, 0, 0, 0])], 0, width, height, 90.0, znear, zfar)


def test_hand_computable_cases():
    close = lambda a, b: abs(a - b) < 1e-11
    # the pixel rays themselves: W = 4, H = 2 at fovy 90 gives x = (+-3/4, +-1/4) * 2, y = +-1/2; a plane z = -2 reads depth 2 everywhere
    rays = depth_ref.pixel_rays(4, 2, 1.0)
    assert np.allclose(rays[:, 0].reshape(2, 4)[0], [-1.5, -0.5, 0.5, 1.5]) and np.allclose(rays[:, 1].reshape(2, 4)[:, 0], [0.5, -0.5]) and (rays[:, 2] == -1).all()
    d, g, _ = _view([geom("plane", (0, 0), pos=[0, 0, -2])])
    assert np.allclose(d, 2.0, atol=1e-11) and (g == 0).all()          # depth is metres along the axis, not along the ray
    # a sphere of radius 0.5, centre 4 ahead and 0.3 beside the axis: a 3-4-5 triangle, the entry 0.4 before the centre's plane
    d, g, _ = _view([geom("sphere", [0.5], pos=[0.3, 0, -4])])
    assert close(d[0, 1, 1], 3.6) and g[0, 1, 1] == 0 and d[0, 0, 0] == 12.0 and g[0, 0, 0] == -1
    # a box face-on; through a corner pixel the depth is still the face's
    d, g, _ = _view([geom("box", [2, 2, 0.5], pos=[0, 0, -3])])
    assert close(d[0, 1, 1], 2.5) and close(d[0, 0, 2], 2.5)
    # a plane at 60 degrees to the view: its normal (sin 60, 0, cos 60) in the camera frame through (0, 0, -2): depth 2 on the axis,
    # and on the ray (2/3, 0, -1): 2 cos 60 / (cos 60 - 2/3 sin 60)  < 0: that ray runs away from it, the ray (-2/3, 0, -1) meets it at 0.928..
    q = [math.cos(math.radians(30)), 0, math.sin(math.radians(30)), 0]
    d, _, _ = _view([geom("plane", (0, 0), pos=[0, 0, -2], quat=q)])
    assert close(d[0, 1, 1], 2.0) and close(d[0, 1, 0], 1.0 / (0.5 + 2 / 3 * math.sin(math.radians(60)))) and d[0, 1, 2] == 12.0
    # a finite plane: inside its half sizes only; a single positive half size bounds one axis only; from behind: nothing
    assert _view([geom("plane", (0.5, 0.5), pos=[0, 0, -2])])[0][0, 0, 0] == 12.0 and close(_view([geom("plane", (0, 0.5), pos=[0, 0, -2])])[0][0, 1, 0], 2.0)
    assert _view([geom("plane", (0, 0), pos=[0, 0, -2], quat=[0, 1, 0, 0])])[0][0, 1, 1] == 12.0
    # capsule and cylinder end on, an ellipsoid along its third axis
    assert close(_view([geom("capsule", [0.2, 0.5], pos=[0, 0, -2])])[0][0, 1, 1], 1.3)
    assert close(_view([geom("cylinder", [0.2, 0.5], pos=[0.1, 0, -2])])[0][0, 1, 1], 1.5)
    assert close(_view([geom("ellipsoid", [0.5, 0.3, 0.2], pos=[0, 0, -2])])[0][0, 1, 1], 1.8)
    # a tetrahedron's slanted face x + y + z = 1, seen from (0.2, 0.2, 3): depth 3 - 0.6
    unit = dict(vertex=[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], face=[[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], convex=True)
    assert close(_view([geom("mesh", mesh="t")], eye=[0.2, 0.2, 3], meshes=dict(t=unit))[0][0, 1, 1], 2.4)


def test_near_plane_limit_one_sided_quad_and_eye_inside():
    close = lambda a, b: abs(a - b) < 1e-11
    flat = dict(vertex=[[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], face=[[0, 1, 2], [0, 2, 3]], convex=False)      # counter-clockwise seen from +z
    back = geom("plane", (0, 0), pos=[0, 0, -5])
    # the open quad from its front, and from its back: what lies behind shows
    assert close(_view([geom("mesh", mesh="q", pos=[-0.5, -0.5, -1]), back], meshes=dict(q=flat))[0][0, 1, 1], 1.0)
    d, g, _ = _view([geom("mesh", mesh="q", pos=[-0.5, -0.5, -1], quat=[0, 1, 0, 0]), back], meshes=dict(q=flat))      # half a turn about x: its back faces the eye
    assert close(d[0, 1, 1], 5.0) and g[0, 1, 1] == 1
    # the eye inside a sphere, a box and a tetrahedron: they are not drawn
    unit = dict(vertex=[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], face=[[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], convex=True)
    for shape, m in ((geom("sphere", [0.5], pos=[0.1, 0, 0.1]), None), (geom("box", [0.5, 1, 1], pos=[0.2, 0, 0]), None), (geom("mesh", mesh="t", pos=[-0.2, -0.2, -0.2]), dict(t=unit))):
        d, g, _ = _view([shape, back], meshes=m)
        assert np.allclose(d, 5.0, atol=1e-11) and (g == 1).all()
    # the near plane: a sphere whose entry depth is 0.3 is drawn with znear 0.25 and not drawn with znear 0.35 (the back shows: not its far side)
    s = geom("sphere", [0.5], pos=[0, 0, -0.8])
    assert close(_view([s, back], znear=0.25)[0][0, 1, 1], 0.3) and close(_view([s, back], znear=0.35)[0][0, 1, 1], 5.0)
    # the far plane and the limit: a hit beyond zfar reads zfar raw and geom -1; with a limit every value above it reads 0, nothing reads 0
    raw, g, gz = _view([geom("sphere", [0.5], pos=[0, 0, -3])], zfar=4.0)
    assert close(raw[0, 1, 1], 2.5) and raw[0, 0, 0] == 4.0
    lim, gl, _ = depth_ref.limited(raw, g, gz, 2.0, 4.0)
    assert lim[0, 1, 1] == 0 and lim[0, 0, 0] == 0 and gl[0, 1, 1] == -1
    lim, gl, _ = depth_ref.limited(raw, g, gz, 3.0, 4.0)
    assert close(lim[0, 1, 1], 2.5) and lim[0, 0, 0] == 0 and gl[0, 1, 1] == 0
    raw, g, _ = _view([geom("sphere", [0.5], pos=[0, 0, -5])], zfar=4.0)
    assert raw[0, 1, 1] == 4.0 and g[0, 1, 1] == -1
    # invisible: alpha 0 and group 3; a geom of the camera's own body is drawn
    scene = dict(world=[dict(geom("sphere", [0.5], pos=[0, 0, -2]), alpha=0.0), dict(geom("sphere", [0.5], pos=[0, 0, -3]), group=3), geom("sphere", [0.5], pos=[0, 0, -6])],
                 bodies=[body("cam", [geom("sphere", [0.5], pos=[0, 0, -5])])], cameras=[depth_rig.camera(0, fovy=90.0)], meshes={})
    d, g, _ = depth_ref.view(scene, [pose([0, 0, 0], [1, 0, 0, 0])], 0, 3, 3, 90.0, 0.02, 12.0)
    assert close(d[0, 1, 1], 4.5) and g[0, 1, 1] == 3


def test_graze_names_a_silhouette_pixel():
    """A pixel ray 5e-5 m inside a sphere's silhouette grazes, one 1 mm inside does not; so for the near plane and the limit."""
    for inset, grazing in ((5e-5, True), (1e-3, False)):
        d, g, gz = _view([geom("sphere", [0.5], pos=[0.5 - inset, 0, -3])])
        assert g[0, 1, 1] == 0 and (gz[0, 1, 1] < ray_ref.GRAZE) == grazing
        d, g, gz = _view([geom("sphere", [0.5], pos=[0, 0, -0.8])], znear=0.3 - inset)          # the entry depth 0.3 against the near plane
        assert (gz[0, 1, 1] < ray_ref.GRAZE) == grazing
    raw, g, gz = _view([geom("sphere", [0.5], pos=[0, 0, -3])])
    for limit, grazing in ((2.5 + 2e-4, True), (2.5 + 5e-3, False)):                           # within the comparison bound of the limit
        assert (depth_ref.limited(raw, g, gz, limit, 12.0)[2][0, 1, 1] < ray_ref.GRAZE) == grazing


@pytest.mark.parametrize("builder", list(depth_rig.BUILDERS))
def test_oracle_against_the_reference(builder):
    """Every rig scene: the oracle's raw image, limited image and geom-id image against the reference."""
    cases, _, _ = depth_rig.reference(builder)
    depth_rig.compare(builder, [depth_rig.oracle_views(c) for c in cases], bound="oracle")


def test_builders_meet_their_own_conditions():
    """What each builder is for, on the reference side."""
    # large: a box face, the open triangle and the sliver each have a candidate box over RASTER_MAX_BOX pixels, and all three are seen
    c = depth_rig.large()[0]
    boxes = depth_rig.screen_boxes(c)
    assert len(boxes) == 3 and all(max(v) > depth_rig.RASTER_MAX_BOX for v in boxes.values()), boxes
    _, who, _ = depth_rig.reference("large")[1][0][0]
    share = [float((who == k).mean()) for k in range(3)]
    assert share[0] > 0.2 and share[1] > 0.2 and 0.002 < share[2] < 0.05, share          # the sliver: a large box, a small area
    # list_full: more than HLCAP triangles are cut by the near plane with their visible part on screen, in every env
    c = depth_rig.list_full()[0]
    cut = [depth_rig.cut_triangles(c, e) for e in range(len(c["q32"]))]
    assert len(c["scene"]["meshes"]["tunnel"]["face"]) >= 320 and min(cut) > depth_rig.HLCAP, cut
    c = depth_rig.list_full()[1]
    boxes = depth_rig.screen_boxes(c)
    _, who, _ = depth_rig.reference("list_full")[1][1][0]
    assert depth_rig.cut_triangles(c, 0) > depth_rig.HLCAP and sum(max(v, default=0) > depth_rig.RASTER_MAX_BOX for v in boxes.values()) >= 4, boxes
    assert all((who == k).mean() > 0.01 for k in range(6)), [float((who == k).mean()) for k in range(6)]          # the tunnel, its end and each large triangle are seen
    # far_thin: every aimed pixel sees its own geom, in range; the marks: inside the limit, outside it, beyond the far plane
    c = depth_rig.far_thin()[0]
    raw, who, graze = depth_rig.reference("far_thin")[1][0][0]
    for k, (u, v) in enumerate(c["aimed"]):
        assert (who[:, v, u] == k).all() and (raw[:, v, u] < depth_rig.LIMIT).all(), (k, u, v)
    (u0, v0, _), (u1, v1, _), (u2, v2, _) = c["marks"]
    assert np.allclose(raw[:, v0, u0], depth_rig.LIMIT - 0.01, atol=1e-9) and np.allclose(raw[:, v1, u1], depth_rig.LIMIT + 0.01, atol=1e-9) and (raw[:, v2, u2] == depth_rig.ZFAR).all()
    assert (who[:, v2, u2] == -1).all() and (graze >= ray_ref.GRAZE).all()
    # capacity: exactly 128 drawn geoms, each seen by the pixel aimed at it
    c = depth_rig.capacity()[0]
    _, who, _ = depth_rig.reference("capacity")[1][0][0]
    assert len(depth_ref.geoms_of(c["scene"])) == 128 and len(depth_ref.geoms_of(depth_rig.capacity_overflow())) == 129
    for k, (u, v) in enumerate(c["aimed"]):
        assert (who[:, v, u] == k).all(), (k, u, v)
    # near: the straddled shape is seen in some pixels and cut away in others; from inside it is not seen at all
    cases, refs, _ = depth_rig.reference("near")
    for e in range(len(depth_rig.CLOSED)):
        assert (refs[0][0][1][e] == 1 + e).any() and (refs[0][0][0][e][refs[0][0][1][e] == 1 + e].min() < 2 * depth_rig.ZNEAR), e
        assert not (refs[1][0][1][e] == 1 + e).any() and (refs[1][0][1][e] >= 0).mean() > 0.3, e
    assert all((refs[2][0][1] == k).any() for k in (2, 3))          # both sheets are seen
