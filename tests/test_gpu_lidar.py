"""smj_lidar_kernel against tests/ray_ref.py, an fp64 reference that shares no code and no formula with the kernel, the oracle or the
model compiler: one test per scene builder of tests/ray_rig.py.  The device scan is read through pull_sensor_data().lidar after one
step that moves nothing; the reference gets the device's qpos.  The rule is ray_rig.compare's: grazing rays (named by the reference
alone: within 1e-4 m of changing between hit and miss, or of a mesh edge / box or cylinder rim) are left out, at most 1 % of a test's
rays and 2 per env; on every other ray hit or miss agrees exactly and the range is within 16 x the input-rounding floor of the test
(the largest change of the reference's own answer when qpos and the model's constants are rounded to fp32), never above 1e-3 m.
DESIGN.md ("Lidar rays against an independent reference") keeps the measured floors, errors and ratios."""
import numpy as np
import pytest

import ray_ref
import ray_rig

pytestmark = pytest.mark.gpu


def _run(builder, options=()):
    cases = ray_rig.BUILDERS[builder]()
    scans = [ray_rig.device_scan(c["scene"], c["q32"], options) for c in cases]
    return cases, scans


def _compare(builder):
    cases, scans = _run(builder)
    for c, (_, q) in zip(cases, scans):
        assert np.abs(q - c["q32"]).max() < 1e-6, c["name"]       # the step moved nothing (a unit quaternion may be renormalised in its last bit)
    out = ray_rig.compare(cases, scans)
    return cases, scans, out


def test_every_geom_type_at_general_poses():
    """(a) plane (infinite, finite), sphere, capsule, ellipsoid, cylinder, box, a 20-face convex mesh, a tetrahedron, an open quad:
    in the world and on free bodies, every frame non-identity, the laser pitched and rolled."""
    _compare("types")


def test_origin_inside_every_closed_type():
    """(b) the exit distance from inside sphere, capsule (side and cap), ellipsoid, cylinder, box and both closed meshes."""
    cases, scans, _ = _compare("inside")
    assert (scans[0][0] > 0).all()          # every ray leaves the shape it starts in


def test_exact_alignments():
    """(c) an identity laser among geoms at quarter turns: zero ray components, rays in a box face's plane, along a cylinder's axis,
    axis-parallel through the mesh tree.  The rays are aimed: none grazes."""
    _, _, (_, _, ngraze, _) = _compare("aligned")
    assert ngraze == 0


def test_far_and_thin():
    """(d) r = 1, 2, 5 cm at 3, 6 and 9.9 m, aimed within 0.9 r; a sphere at 9.99 m reads its range, one at 10.01 m exactly the cutoff,
    an empty direction -1.  The rays are aimed: none grazes."""
    cases, scans, (_, _, ngraze, _) = _compare("far_thin")
    got = scans[0][0]
    assert ngraze == 0
    assert (np.abs(got[:, -3] - 9.99) < 1e-4).all() and (got[:, -2] == ray_rig.CUTOFF).all() and (got[:, -1] == -1).all()
    assert (got[:, :-3] > 0).all() and (got[:, :-3] < ray_rig.CUTOFF).all()


def test_more_geoms_than_one_chunk():
    """(e) 132 spheres: the nearest hit in the first chunk of 128 for some rays, in the last geom of the second chunk for others
    (tests/test_ray_ref.py pins that on the reference)."""
    _compare("chunks")


def test_scan_plane_cull():
    """(f) a coplanar fan on a laser tilted up to 0.5 rad has the cull on: bitwise the same scan with lidar_cull = 0, and equal to the
    reference, with a long capsule crossing the plane far from its centre and spheres that reach into the plane by 2 mm and stay 2 mm
    clear of it.  Two cones at +-20 degrees and a ring of origins are not a fan from one point in one plane: equal to the reference,
    which pins that the loader switched the cull off where it could drop a geom that a ray meets."""
    cases, scans = _run("cull", options=[[("lidar_cull", 1)], [("lidar_cull", 0)]])
    for c, per_option in zip(cases, scans):
        assert np.array_equal(per_option[0][0], per_option[1][0]), c["name"]
    ray_rig.compare(cases, [s[0] for s in scans])
    flat, q = scans[0][0]
    ref, _ = ray_ref.scan(cases[0]["scene"], q)
    reach, clear = ref[:, 0], ref[:, 90]                # the rays of the fan at 0 and 90 degrees: the sphere 2 mm into the plane, the one 2 mm clear
    assert (np.abs(reach - 1.5) < 0.03).all() and (np.abs(clear - 1.5) > 0.2).all()


def test_weld_group_own_body_alpha_and_group():
    """(g) every primitive type and two meshes on a jointless child of the laser (the compiler's static table); a geom of the site's own
    body is never seen; a laser welded to the world over a floor and world geoms of every type; alpha 0 invisible, group 3 visible."""
    cases, scans, _ = _compare("welded")
    for c, (got, _) in zip(cases, scans):
        assert (got > 0).mean() > 0.5, c["name"]          # (on the parent commit the welded laser read -1 on every ray)
