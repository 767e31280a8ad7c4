"""tests/ray_ref.py on cases a hand can compute, then the fp64 oracle (oracle/smj_oracle.c, starting from the model compiler's static
table of the geoms welded to the laser) against it on every scene of tests/ray_rig.py.  Both sides are fp64 on identical inputs and
the reference bisects to 1e-12, so the bound is 1e-9 m and no ray is exempt but the grazing ones (ray_rig.compare).  CPU only."""
import math

import numpy as np
import pytest

import ray_ref
import ray_rig
from ray_rig import geom


def _one(g, origin, direction, meshes=None):
    """Range of one ray from `origin` along `direction` against one world geom."""
    scene = dict(world=[g], bodies=[ray_rig.body("laser")], laser=0, sites=[ray_rig.aim(direction)], cutoff=0.0, meshes=meshes or {})
    out, _ = ray_ref.scan(scene, [ray_rig.pose(origin, [1, 0, 0, 0])])
    return float(out[0, 0])


def test_hand_computable_cases():
    close = lambda a, b: abs(a - b) < 1e-11
    # a sphere on the axis: centre 3 m ahead, radius 0.5; from inside, the far side
    assert close(_one(geom("sphere", [0.5], pos=[3, 0, 0]), [0, 0, 0], [1, 0, 0]), 2.5)
    assert close(_one(geom("sphere", [0.5], pos=[3, 0, 0]), [3.1, 0, 0], [1, 0, 0]), 0.4)
    assert _one(geom("sphere", [0.5], pos=[3, 0, 0]), [0, 0, 0], [-1, 0, 0]) == -1
    # ... and off the axis by 0.3: a 3-4-5 triangle, 0.4 before the centre's plane
    assert close(_one(geom("sphere", [0.5], pos=[3, 0.3, 0]), [0, 0, 0], [1, 0, 0]), 2.6)
    # a box face-on, and through it from inside
    assert close(_one(geom("box", [0.5, 1, 1], pos=[2, 0, 0]), [0, 0.3, -0.2], [1, 0, 0]), 1.5)
    assert close(_one(geom("box", [0.5, 1, 1], pos=[2, 0, 0]), [2.1, 0.3, -0.2], [1, 0, 0]), 0.4)
    # a plane at 30 degrees of incidence from 1 m above it: 1 / cos(60 deg) = 2; from behind, and outside its half sizes: nothing
    d = [math.sin(math.radians(60)), 0, -math.cos(math.radians(60))]
    assert close(_one(geom("plane", (0, 0)), [0, 0, 1], d), 2.0)
    assert _one(geom("plane", (0, 0)), [0, 0, -1], [0, 0, 1]) == -1
    assert close(_one(geom("plane", (2, 1)), [0, 0, 1], d), 2.0) and _one(geom("plane", (1.7, 1)), [0, 0, 1], d) == -1
    # a capsule end on: radius 0.2, half length 0.5, along z, from 2 m above its centre; from the side it is a cylinder
    assert close(_one(geom("capsule", [0.2, 0.5]), [0, 0, 2], [0, 0, -1]), 1.3)
    assert close(_one(geom("capsule", [0.2, 0.5]), [2, 0, 0.3], [-1, 0, 0]), 1.8)
    # a cylinder's cap, an ellipsoid along its second axis, a tetrahedron's face, the open quad from both sides
    assert close(_one(geom("cylinder", [0.2, 0.5]), [0.1, 0, 2], [0, 0, -1]), 1.5)
    assert close(_one(geom("ellipsoid", [0.5, 0.3, 0.2]), [0, 2, 0], [0, -1, 0]), 1.7)
    unit = dict(vertex=[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], face=[[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], convex=True)
    assert close(_one(geom("mesh", mesh="t"), [0.2, 0.2, 3], [0, 0, -1], dict(t=unit)), 3 - 0.6)
    assert close(_one(geom("mesh", mesh="t"), [0.2, 0.2, 0.1], [0, 0, -1], dict(t=unit)), 0.1)
    flat = dict(vertex=[[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], face=[[0, 1, 2], [0, 2, 3]], convex=False)
    assert close(_one(geom("mesh", mesh="q"), [0.7, 0.2, 1], [0, 0, -1], dict(q=flat)), 1.0) and close(_one(geom("mesh", mesh="q"), [0.2, 0.7, -2], [0, 0, 1], dict(q=flat)), 2.0)
    assert _one(geom("mesh", mesh="q"), [1.2, 0.2, 1], [0, 0, -1], dict(q=flat)) == -1


def test_the_rule_nearest_visible_geom_own_body_excluded_cutoff():
    far, near = geom("sphere", [0.5], pos=[5, 0, 0]), geom("sphere", [0.5], pos=[3, 0, 0])
    scene = dict(world=[far, dict(near, alpha=0.0), dict(geom("sphere", [0.2], pos=[4, 0, 0]), group=3)], bodies=[ray_rig.body("laser", [geom("sphere", [0.1], pos=[1, 0, 0])])],
                 laser=0, sites=[ray_rig.aim([1, 0, 0]), ray_rig.aim([0, 1, 0])], cutoff=3.5, meshes={})
    out, graze = ray_ref.scan(scene, [ray_rig.pose([0, 0, 0], [1, 0, 0, 0])])
    assert abs(out[0, 0] - 3.5) < 1e-15 and out[0, 1] == -1          # alpha 0 and the own body are passed through, group 3 is met at 3.8: the cutoff
    out, _ = ray_ref.scan(dict(scene, cutoff=0.0), [ray_rig.pose([0, 0, 0], [1, 0, 0, 0])])
    assert abs(out[0, 0] - 3.8) < 1e-11
    # graze names the ray that passes 5e-5 m inside a sphere's silhouette, and not the one 1 mm inside
    for inset, grazing in ((5e-5, True), (1e-3, False)):
        s = dict(scene, world=[geom("sphere", [0.5], pos=[3, 0.5 - inset, 0])], bodies=[ray_rig.body("laser")], sites=[ray_rig.aim([1, 0, 0])])
        out, graze = ray_ref.scan(s, [ray_rig.pose([0, 0, 0], [1, 0, 0, 0])])
        assert out[0, 0] > 0 and (graze[0, 0] < ray_ref.GRAZE) == grazing


@pytest.mark.parametrize("builder", list(ray_rig.BUILDERS))
def test_oracle_and_static_table_against_the_reference(builder):
    """Every rig scene: the oracle's scan of the compiled, fused model within 1e-9 m of the reference, hit or miss the same on every ray
    that does not graze; the grazing rays stay under the cap (none in the builders whose rays are aimed)."""
    cases = ray_rig.BUILDERS[builder]()
    scans = [(ray_rig.oracle_scan(c["scene"], c["q32"]), c["q32"].astype(np.float64)) for c in cases]
    _, _, ngraze, _ = ray_rig.compare(cases, scans, bound=1e-9)
    assert ngraze == 0 or builder not in ray_rig.AIMED


def test_chunks_scene_puts_the_nearest_hit_in_either_chunk():
    """(e): for some rays the nearest hit is the last geom of the last chunk of 128, for others a geom of the first chunk."""
    c = ray_rig.chunks()[0]
    assert len(c["scene"]["world"]) >= 130
    ref, _ = ray_ref.scan(c["scene"], c["q32"].astype(np.float64))
    last, _ = ray_ref.scan(dict(c["scene"], world=c["scene"]["world"][-1:]), c["q32"].astype(np.float64))
    first, _ = ray_ref.scan(dict(c["scene"], world=c["scene"]["world"][:128]), c["q32"].astype(np.float64))
    assert int(((ref > 0) & (ref == last)).sum()) >= 3 and int(((ref > 0) & (ref == first)).sum()) >= 100
    assert int(((ref > 0) & (ref != first)).sum()) >= 10          # rays whose answer lies past the first 128 geoms
