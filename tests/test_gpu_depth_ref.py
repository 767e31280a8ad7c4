"""The depth path (smj_depth_prepass -> smj_meshlet_kernel -> smj_depth_kernel, entered through smj_render_depth / smj_render_rgb)
against tests/depth_ref.py, an fp64 reference that shares no code and no formula with the kernels, the oracle or the model compiler:
one test per scene builder of tests/depth_rig.py.  Each renders with depth_raster 1 and 0, raw and with the 10 m limit, plus the
geom-id image, after one step that moves nothing.  The rule is depth_rig.compare's: grazing pixels (named by the reference alone) are
left out, at most 1 % of a test's pixels and 2 % of an image, none where the pixels are aimed; on every other pixel hit or miss and the
geom id agree exactly and the depth is within 16 x the input-rounding floor of the test -- on the pixels that depth_raster = 1
rasterises (meshes and boxes: 1 / depth interpolated with 1-ulp reciprocals) within the project's ceiling 1e-4 + 1e-4 z, which no
path may exceed.  DESIGN.md ("Depth cameras against an independent reference") keeps the measured floors, errors and ratios."""
import numpy as np
import pytest

import depth_rig

pytestmark = pytest.mark.gpu


def _compare(builder):
    cases, _, _ = depth_rig.reference(builder)
    images = [depth_rig.device_views(c) for c in cases]
    for c, per_q in zip(cases, images):
        for q, imgs in zip([c["q32"]] + ([c["then"]] if c["then"] is not None else []), per_q):
            assert np.abs(imgs["qpos"] - np.asarray(q, np.float32)).max() < 1e-6, c["name"]       # the step moved nothing
    return cases, images, depth_rig.compare(builder, images)


def test_every_geom_type_at_general_poses():
    """Infinite, finite and half-bounded plane, sphere, capsule, ellipsoid, cylinder, box, a 20-face convex mesh, a tetrahedron, the
    open quad from its front and from its back: in the world and on free bodies, every frame non-identity, the camera pitched and rolled."""
    _compare("types")


def test_near_plane_and_eye_inside():
    """Every closed type straddling the near plane (drawn where its entry is beyond the plane, cut away where it is nearer); the eye
    inside every closed type: what lies behind shows; a large folded sheet across the near plane, on the camera's body and off it."""
    _compare("near")


def test_triangles_too_large_for_a_wave():
    """160 x 120: a box face and an open triangle with more than 16384 candidate pixels, and a sliver along the diagonal whose box is
    as large but which covers one pixel in a hundred (the per-tile polygon cull of the handed-over triangles)."""
    _compare("large")


def test_hand_over_list_full():
    """384 long triangles round the optical axis, each cut by the near plane with its visible part on screen: more than HLCAP = 256
    per env (tests/test_depth_ref.py pins that on the reference), so the rasteriser keeps the rest."""
    _compare("list_full")


def test_far_and_thin():
    """r = 1, 2, 5 cm spheres, capsules, cylinders and boxes at 3, 6 and 9.9 m on the rays of chosen pixels, their centres up to 0.9 r
    beside the ray; a sphere at 9.99 m reads its depth, one at 10.01 m reads 0 with the limit and its depth without, one beyond the
    far plane reads the far plane.  The pixels are aimed: none grazes."""
    cases, images, stat = _compare("far_thin")
    c, imgs = cases[0], images[0][0]
    assert stat["grazing"] == 0
    (u0, v0, _), (u1, v1, _), (u2, v2, _) = c["marks"]
    for path in ("raster", "ray"):
        raw, lim = imgs[path + "_raw"], imgs[path + "_lim"]
        assert (np.abs(lim[:, v0, u0] - 9.99) < 1e-4).all() and (lim[:, v1, u1] == 0).all() and (np.abs(raw[:, v1, u1] - 10.01) < 1e-4).all()
        assert (raw[:, v2, u2] == depth_rig.ZFAR).all() and (lim[:, v2, u2] == 0).all()
        for u, v in c["aimed"]:
            assert (lim[:, v, u] > 0).all(), (path, u, v)


def test_renderer_capacity():
    """128 camera-visible geoms, each seen by the pixel aimed at it (thread 127 of the staging pass stages the camera and a geom);
    a model with 129 does not load."""
    from stretch_mujoco_amd import StretchBatchSimulator

    cases, images, stat = _compare("capacity")
    assert stat["grazing"] == 0
    gid = images[0][0]["gid"]
    for k, (u, v) in enumerate(cases[0]["aimed"]):
        assert (gid[:, v, u] == k).all(), (k, u, v)
    with pytest.raises(Exception, match="renderer capacity"):
        StretchBatchSimulator(num_envs=1, device="cuda:0", model_blob_bytes=depth_rig.blob(depth_rig.capacity_overflow())).start(home=False)


def test_staging_pass_culls_nothing_that_is_seen():
    """A long capsule with one end behind the eye plane (a box corner behind the eye: the sphere's rectangle is kept), a wide flat box
    under the camera (the eye inside its bounding sphere: no rectangle), spheres whose silhouettes cross a tile's corner by a third of
    a pixel or stay that short of it, a sphere whose centre is beyond the limit and whose surface is within it."""
    _compare("cull")


def test_camera_static_layer():
    """Every primitive type and two meshes on the camera's own body and on a jointless child of it, rendered, the body moved, rendered
    again in the same context (the layer is cached per camera, size and field of view); a camera welded to the world over world geoms
    of every type and a free body; alpha 0 and group 3 are invisible."""
    _compare("layer")


def test_exact_alignments():
    """An identity body with a quarter-turn camera at dyadic positions: box faces, a cylinder end and a capsule end head-on, the floor's
    horizon on the centre row, the centre pixel's ray exactly (0, 0, -1).  No pixel grazes."""
    _, _, stat = _compare("aligned")
    assert stat["grazing"] == 0
