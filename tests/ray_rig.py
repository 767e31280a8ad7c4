"""Robot-less scenes with a lidar, as plain data: tests/ray_ref.py reads the data, the MJCF compiled for the oracle and the device is
written from the same data.  TEST INFRASTRUCTURE.  Gravity is off and no geom collides, so one step moves nothing; the laser is a body
whose sites are named ray000 .. with one <rangefinder site="ray" cutoff="10"/>; at most three further free bodies, which stays
within the standard build's 32 columns.  Per-env poses are drawn in fp64 (`q64`); the device, the oracle and the reference all get
them rounded to fp32 (`q32`), the reference's input-rounding floor compares q64 with exact constants against q32 with rounded ones.

The builders, one per property of the ray caster (each returns a list of cases, a case = dict(name, scene, q64)):
  types()      (a) every geom type once in the world and once on a free body, both with non-identity frames; laser with pitch and roll
  inside()     (b) the laser inside every closed type (the capsule: cylindrical part and cap), one type per env
  aligned()    (c) identity laser, geoms at quarter turns: ray components that are exactly 0, rays in the plane of a box face, along a
               cylinder's axis, axis-parallel through a mesh tree
  far_thin()   (d) r = 1, 2, 5 cm at 3, 6, 9.9 m with rays aimed inside 0.9 r; 9.99 m and 10.01 m; an empty direction
  chunks()     (e) 132 spheres on two rings, more than one chunk of the kernel's geom list
  cull()       (f) a coplanar tilted fan (cull on) with geoms that just reach and just miss the scan plane; two cones (cull off)
  welded()     (g) geoms on a jointless child of the laser and on the laser's own body; a laser welded to the world; alpha 0; group 3"""
import math

import numpy as np

import ray_ref

CUTOFF = 10.0
S = math.sqrt(0.5)


def geom(type, size=(0, 0, 0), pos=(0, 0, 0), quat=(1, 0, 0, 0), alpha=1.0, group=0, mesh=None):
    size = list(size) + [0.0] * (3 - len(size))
    return dict(type=type, size=[float(x) for x in size], pos=[float(x) for x in pos], quat=[float(x) for x in quat], alpha=alpha, group=group, mesh=mesh)


def body(name, geoms=(), pos=(0, 0, 0), quat=(1, 0, 0, 0), free=True, parent=-1):
    return dict(name=name, parent=parent, pos=[float(x) for x in pos], quat=[float(x) for x in quat], free=free, geoms=list(geoms))


def qmul(a, b):
    return ray_ref._qmul(np.asarray(a, np.float64), np.asarray(b, np.float64))


def axis_quat(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return np.concatenate([[math.cos(angle / 2)], math.sin(angle / 2) * a])


def ypr(yaw, pitch, roll):
    return qmul(qmul(axis_quat([0, 0, 1], yaw), axis_quat([0, 1, 0], pitch)), axis_quat([1, 0, 0], roll))


def random_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


# site orientations whose +Z is exactly +x, +y, -x, -y, -z in fp32 and fp64 alike (every product of their components is exact)
EXACT = {0: (0.5, 0.5, 0.5, 0.5), 90: (0.5, -0.5, 0.5, 0.5), 180: (0.5, 0.5, -0.5, -0.5), 270: (0.5, 0.5, 0.5, -0.5)}


def ray_site(azimuth, elevation=0.0, pos=(0, 0, 0)):
    """A site at `pos` of the laser whose +Z points along the azimuth (about the laser's z) at the elevation."""
    return ([float(x) for x in pos], [float(x) for x in qmul(axis_quat([0, 0, 1], azimuth), axis_quat([0, 1, 0], math.pi / 2 - elevation))])


def fan(n, elevation=0.0):
    return [ray_site(2 * math.pi * i / n, elevation) for i in range(n)]


def aim(target, origin=(0, 0, 0)):
    """A site at `origin` whose +Z points at `target` (laser frame)."""
    d = np.asarray(target, np.float64) - np.asarray(origin, np.float64)
    return ray_site(math.atan2(d[1], d[0]), math.atan2(d[2], math.hypot(d[0], d[1])), origin)


def _icosahedron():
    from scipy.spatial import ConvexHull

    p = (1 + math.sqrt(5)) / 2
    v = np.array([[0, a, b * p] for a in (-1, 1) for b in (-1, 1)] + [[a, b * p, 0] for a in (-1, 1) for b in (-1, 1)] + [[b * p, 0, a] for a in (-1, 1) for b in (-1, 1)], float)
    v = 0.3 * v / np.linalg.norm(v[0])
    v = ray_ref._rotate(np.tile(ypr(0.37, -0.52, 0.81), (len(v), 1)), v) + np.array([0.02, -0.03, 0.01])   # no vertex, edge or face normal along an axis
    f = ConvexHull(v).simplices.copy()
    for k in range(len(f)):
        a, b, c = v[f[k]]
        if np.dot(np.cross(b - a, c - a), a - v.mean(0)) < 0:
            f[k] = f[k][::-1]
    return dict(vertex=v.tolist(), face=f.tolist(), convex=True)


MESHES = {
    "ico": _icosahedron(),      # 20 faces: 10 leaves of the kernel's tree, padded to 16
    "tet": dict(vertex=[[0.3, 0.02, -0.1], [-0.2, 0.25, -0.12], [-0.15, -0.28, -0.08], [0.03, -0.01, 0.33]], face=[[0, 2, 1], [0, 1, 3], [1, 2, 3], [2, 0, 3]], convex=True),
    "quad": dict(vertex=[[-0.3, -0.2, 0.0], [0.3, -0.25, 0.02], [0.32, 0.2, 0.0], [-0.28, 0.22, -0.02]], face=[[0, 1, 2], [0, 2, 3]], convex=False),   # open: one leaf
}
for _m in MESHES.values():      # the model stores the triangles of a ray-cast mesh in fp32: vertices that fp32 holds exactly, so every side gets the same mesh
    _m["vertex"] = np.asarray(_m["vertex"], np.float32).astype(np.float64).tolist()


def make_scene(world, bodies, laser, sites):
    used = {g["mesh"] for g in world if g["mesh"]} | {g["mesh"] for b in bodies for g in b["geoms"] if g["mesh"]}
    return dict(world=list(world), bodies=list(bodies), laser=laser, sites=list(sites), cutoff=CUTOFF, meshes={k: MESHES[k] for k in sorted(used)})


def case(name, scene, q64):
    q64 = np.asarray(q64, np.float64)
    assert q64.shape[1] == 7 * sum(b["free"] for b in scene["bodies"])
    return dict(name=name, scene=scene, q64=q64, q32=q64.astype(np.float32))


def pose(p, q):
    return np.concatenate([np.asarray(p, np.float64), np.asarray(q, np.float64)])


# ------------------------------------------------------------------------------------------------ MJCF
def _f(v):
    return " ".join(repr(float(x)) for x in v)


def _geom_xml(g):
    size = f'size="{_f(g["size"][:2])} 1"' if g["type"] == "plane" else (f'mesh="{g["mesh"]}"' if g["type"] == "mesh" else f'size="{_f(g["size"])}"')
    name = f'name="{g["name"]}" ' if g.get("name") else ""
    return (f'<geom {name}type="{g["type"]}" {size} pos="{_f(g["pos"])}" quat="{_f(g["quat"])}" rgba="0.5 0.5 0.5 {g["alpha"]}" group="{g["group"]}" '
            'contype="0" conaffinity="0" density="0"/>')


def mjcf(scene):
    def body_xml(i):
        b = scene["bodies"][i]
        inner = '<freejoint/><inertial pos="0 0 0" mass="1" diaginertia="0.01 0.01 0.01"/>' if b["free"] else ""
        inner += "".join(_geom_xml(g) for g in b["geoms"])
        if i == scene["laser"]:
            inner += "".join(f'<site name="ray{r:03d}" pos="{_f(p)}" quat="{_f(q)}"/>' for r, (p, q) in enumerate(scene["sites"]))
        inner += "".join(f'<camera name="cam{k}" pos="{_f(c["pos"])}" quat="{_f(c["quat"])}" fovy="{float(c["fovy"])!r}"/>'
                         for k, c in enumerate(scene.get("cameras", ())) if c["body"] == i)
        inner += "".join(body_xml(j) for j, c in enumerate(scene["bodies"]) if c["parent"] == i)
        return f'<body name="{b["name"]}" pos="{_f(b["pos"])}" quat="{_f(b["quat"])}">{inner}</body>'

    meshes = "".join(f'<mesh name="{k}" vertex="{_f(np.ravel(m["vertex"]))}" face="{" ".join(str(int(i)) for i in np.ravel(m["face"]))}"/>' for k, m in scene["meshes"].items())
    return ('<mujoco><compiler angle="radian"/><option gravity="0 0 0"/>' + scene.get("header", "") + '<asset>' + meshes + '</asset><worldbody>' + "".join(_geom_xml(g) for g in scene["world"]) +
            "".join(body_xml(i) for i, b in enumerate(scene["bodies"]) if b["parent"] < 0) +
            f'</worldbody><sensor><rangefinder site="ray" cutoff="{scene["cutoff"]}"/></sensor></mujoco>')


def blob(scene):
    from stretch_mujoco_amd import mjcf_compiler, model_blob, model_fuse

    return model_blob.dumps(model_fuse.prepare_for_kernels(mjcf_compiler.compile_string(mjcf(scene))))


def oracle_scan(scene, q32):
    """The fp64 oracle's scan [E, R] (the compiler's static table included: the oracle starts from it)."""
    from oracle.oracle import Oracle

    o = Oracle(blob(scene))
    out = []
    for q in np.asarray(q32, np.float64):
        o.arr("qpos")[:] = q
        o.forward(); o.sensors(True)
        out.append(o.arr("lidar").copy())
    o.close()
    return np.array(out)


def device_scan(scene, q32, options=()):
    """(scan [E, R] of the device after one step, qpos [E, nq] after that step) -- per entry of `options` when some are given."""
    import torch

    from stretch_mujoco_amd import StretchBatchSimulator
    from stretch_mujoco_amd.enums import StretchSensors

    sim = StretchBatchSimulator(num_envs=len(q32), device="cuda:0", model_blob_bytes=blob(scene), sensors_to_use=[StretchSensors.base_lidar])
    sim.start(home=False)
    out = []
    for opt in (options or [()]):
        for name, v in opt:
            sim.set_option(name, v)
        sim.qpos[:] = torch.tensor(np.ascontiguousarray(np.asarray(q32, np.float32).T), device=sim.device)
        sim.qvel.zero_()
        sim.step(1)
        out.append((sim.pull_sensor_data().lidar.cpu().numpy().astype(np.float64), sim.qpos.t().cpu().numpy().astype(np.float64)))
    sim.stop()
    return out if options else out[0]


# ------------------------------------------------------------------------------------------------ comparison
def compare(cases, scans, bound=None):
    """The rule of every test: grazing rays (reference alone) are left out and capped at 1 % of the test's rays and 2 per env; on
    the others hit-or-miss agrees exactly and the range is within `bound`, by default 16 x the input-rounding floor and at most
    1e-3 m.  Returns (floor, largest error, grazing rays, rays) after asserting; prints them first."""
    floor = max(ray_ref.floor(c["scene"], c["q64"]) for c in cases)
    worst, ngraze, nray, flips = 0.0, 0, 0, []
    for c, (got, q) in zip(cases, scans):
        ref, graze = ray_ref.scan(c["scene"], q)
        g = graze < ray_ref.GRAZE
        assert g.sum(1).max() <= 2, (c["name"], "grazing rays per env", g.sum(1))
        ngraze += int(g.sum()); nray += g.size
        bad = ~g & ((got < 0) != (ref < 0))
        flips += [(c["name"], int(e), int(r), float(got[e, r]), float(ref[e, r])) for e, r in zip(*np.nonzero(bad))]
        ok = ~g & ~bad
        worst = max(worst, float(np.max(np.abs(got - ref)[ok], initial=0.0)))
    if bound is None:
        bound = min(16 * floor, 1e-3)
    print(f"rays {nray} grazing {ngraze} floor {floor:.3e} bound {bound:.3e} worst {worst:.3e} ratio {worst / floor if floor else float('nan'):.2f} hit/miss flips {len(flips)}")
    assert ngraze <= 0.01 * nray, ("grazing rays", ngraze, nray)
    assert not flips, flips[:10]
    assert worst <= bound, (worst, bound, floor)
    return floor, worst, ngraze, nray


# ------------------------------------------------------------------------------------------------ (a)
def _laser(sites_world_geoms=()):
    return body("laser", sites_world_geoms)


def types(E=6, seed=1):
    rng = np.random.default_rng(seed)
    kinds = {"sphere": geom("sphere", [0.35]), "capsule": geom("capsule", [0.2, 0.4]), "ellipsoid": geom("ellipsoid", [0.5, 0.3, 0.2]),
             "cylinder": geom("cylinder", [0.3, 0.35]), "box": geom("box", [0.4, 0.3, 0.25]), "ico": geom("mesh", mesh="ico"), "tet": geom("mesh", mesh="tet"),
             "quad": geom("mesh", mesh="quad")}
    order = list(kinds)
    cases = []
    for k, (plane, free) in enumerate([((0, 0), ["cylinder", "box", "ico"]), ((4.0, 3.0), ["sphere", "capsule", "ellipsoid"]), ((0, 0), ["tet", "quad", "ico"])]):
        world = [geom("plane", plane, pos=[0.1, -0.2, -0.45], quat=ypr(0.3, 0.04, -0.03))]
        static = [n for n in order if n not in free] if k < 2 else ["sphere", "box", "capsule"]
        for i, n in enumerate(static):     # a ring of world geoms, each with its own frame
            a = 2 * math.pi * (i + 0.3 * k) / len(static)
            world.append(dict(kinds[n], pos=[2.4 * math.cos(a), 2.4 * math.sin(a), 0.05 * i - 0.1], quat=random_quat(rng).tolist()))
        bodies = [_laser()] + [body("b" + n, [dict(kinds[n], pos=[0.1, -0.05, 0.08], quat=random_quat(rng).tolist())]) for n in free]
        q = []
        for e in range(E):
            row = [pose(rng.uniform(-0.2, 0.2, 3), ypr(rng.uniform(-3, 3), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)))]
            for i in range(len(free)):
                a = 2 * math.pi * (i + 0.5) / len(free) + rng.uniform(-0.3, 0.3)
                row.append(pose([1.3 * math.cos(a), 1.3 * math.sin(a), rng.uniform(-0.1, 0.1)], random_quat(rng)))
            q.append(np.concatenate(row))
        cases.append(case(f"types{k}", make_scene(world, bodies, 0, fan(72)), q))
    return cases


# ------------------------------------------------------------------------------------------------ (b)
def inside(seed=2):
    rng = np.random.default_rng(seed)
    shapes = [("sphere", geom("sphere", [0.35]), [0.1, -0.05, 0.1]), ("capsule side", geom("capsule", [0.2, 0.4]), [0.05, 0.04, 0.1]),
              ("capsule cap", geom("capsule", [0.2, 0.4]), [0.03, -0.02, 0.47]), ("ellipsoid", geom("ellipsoid", [0.5, 0.3, 0.2]), [0.2, 0.05, -0.04]),
              ("cylinder", geom("cylinder", [0.3, 0.35]), [0.1, 0.1, -0.2]), ("box", geom("box", [0.4, 0.3, 0.25]), [-0.2, 0.1, 0.15]),
              ("ico", geom("mesh", mesh="ico"), [0.05, 0.02, -0.03]), ("tet", geom("mesh", mesh="tet"), [0.01, 0.0, 0.02])]
    world, q = [], []
    for i, (_, g, at) in enumerate(shapes):
        a = 2 * math.pi * i / len(shapes)
        gq = random_quat(rng)
        gp = np.array([4 * math.cos(a), 4 * math.sin(a), 0.3 * math.sin(3 * a)])
        world.append(dict(g, pos=gp.tolist(), quat=gq.tolist()))
        q.append(pose(gp + ray_ref._rotate(gq, np.asarray(at, float)), random_quat(rng)))     # env i: the laser at `at` of shape i's frame
    sites = fan(36) + fan(12, 0.9) + fan(12, -0.9)
    return [case("inside", make_scene(world, [_laser()], 0, sites), q)]


# ------------------------------------------------------------------------------------------------ (c)
def aligned():
    sites = [(list(map(float, (0, 0, 0))), list(map(float, EXACT[a]))) if a in EXACT else ray_site(math.radians(a)) for a in range(0, 360, 10)]
    sites += [([0.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]), ([0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0])]      # straight up and straight down
    quarter = [S, 0, 0, S]
    world = [
        geom("plane", (0, 0), pos=[0, 0, -1.0]),                                    # below: the down ray meets it head on
        geom("box", [0.25, 0.25, 0.25], pos=[2.0, 0, 0.0]),                         # ahead on +x, face on
        geom("box", [0.25, 0.25, 0.25], pos=[1.25, 0.25, 0.75], quat=quarter),      # its face y = 0 holds the +x ray, which passes 0.5 below it
        geom("box", [0.5, 0.25, 0.25], pos=[0.0, 0.0, 1.5], quat=[0, 0, 0, 1]),     # overhead: the up ray meets it head on
        geom("cylinder", [0.2, 0.3], pos=[0.0, 2.5, 0.0], quat=[0.5, -0.5, 0.5, 0.5]),   # axis along y: the +y ray runs along it
        geom("cylinder", [0.2, 0.5], pos=[-2.0, 0.0, 0.0]),                         # upright: the -x ray meets its side head on
        geom("capsule", [0.15, 0.3], pos=[0.0, -3.0, 0.0], quat=[0.5, -0.5, 0.5, 0.5]),  # end on
        geom("mesh", mesh="ico", pos=[1.5, 1.5, 0.0]), geom("mesh", mesh="ico", pos=[-1.5, -1.5, 0.0], quat=quarter),
        geom("sphere", [0.3], pos=[-1.5, 1.5, 0.0]), geom("ellipsoid", [0.3, 0.2, 0.4], pos=[1.5, -1.5, 0.0], quat=quarter),
    ]
    # every coordinate of the laser is a dyadic fraction: exact in fp32
    q = [pose(p, [1, 0, 0, 0]) for p in ([0, 0, 0], [0.125, 0, 0], [0, -0.125, 0.0625], [-0.25, 0.125, 0])]
    q[1][0:3] = [0.0, 0.0, 0.0]; q[1][3:7] = [0, 0, 0, 1]      # half a turn about z: the rays swap sides, every component still exact
    # the axis-parallel rays through the mesh tree: from a second scene whose meshes sit on the axes
    world2 = [geom("mesh", mesh="ico", pos=[2.0, 0, 0]), geom("mesh", mesh="ico", pos=[0, 2.0, 0], quat=quarter), geom("mesh", mesh="ico", pos=[-2.0, 0, 0], quat=[0, 0, 0, 1]),
              geom("mesh", mesh="tet", pos=[0, -2.0, 0]), geom("mesh", mesh="tet", pos=[0, 0, 2.0]), geom("mesh", mesh="quad", pos=[0, 0, -2.0]), geom("box", [0.5, 0.5, 0.5], pos=[3.5, 3.5, 0])]
    return [case("aligned primitives", make_scene(world, [_laser()], 0, sites), q), case("aligned meshes", make_scene(world2, [_laser()], 0, sites), [q[0], q[3]])]


# ------------------------------------------------------------------------------------------------ (d)
def far_thin(E=4, seed=4):
    rng = np.random.default_rng(seed)
    targets, sites = [], []
    k = 0
    for kind in ("sphere", "capsule", "cylinder"):
        for r in (0.01, 0.02, 0.05):
            for dist in (3.0, 6.0, 9.9):
                az, el = 2 * math.pi * k / 29, 0.5 * math.sin(1.7 * k)
                k += 1
                u = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
                side = np.cross(u, [0, 0, 1.0]); side /= np.linalg.norm(side)
                up = np.cross(side, u)                                            # the geom's axis: across the ray
                c = (dist + r) * u
                zq = ray_site(math.atan2(up[1], up[0]), math.atan2(up[2], math.hypot(up[0], up[1])))[1]
                targets.append(geom(kind, [r, 0.2] if kind != "sphere" else [r], pos=c, quat=zq))
                for off in (-0.9, -0.45, 0.0, 0.6, 0.9):
                    sites.append(aim(c + off * r * side + (0.1 * off if kind != "sphere" else 0.0) * up))
    for dist in (9.99, 10.01):                    # either side of the cutoff: the first reads its range, the second exactly the cutoff
        az = 2 * math.pi * k / 29
        k += 1
        targets.append(geom("sphere", [0.05], pos=[(dist + 0.05) * math.cos(az), (dist + 0.05) * math.sin(az), 0]))
        sites.append(aim(targets[-1]["pos"]))
    sites.append(ray_site(0.05, 1.4))             # nothing there
    bodies = [_laser(), body("targets", targets)]
    q = [np.concatenate([pose([0, 0, 0], [1, 0, 0, 0])] * 2)]
    for e in range(1, E):                         # the same rigid motion for both bodies: the aim holds, the frames do not
        p, qt = rng.uniform(-1, 1, 3), random_quat(rng)
        q.append(np.concatenate([pose(p, qt)] * 2))
    return [case("far and thin", make_scene([], bodies, 0, sites), q)]


# ------------------------------------------------------------------------------------------------ (e)
def chunks(E=4, seed=5):
    rng = np.random.default_rng(seed)
    world = []
    for ring, (radius, phase) in enumerate(((3.0, 0.5), (2.0, 0.0))):      # the inner ring last: its last spheres are the second chunk, and nearest
        for i in range(66):
            a = 2 * math.pi * (i + phase) / 66
            world.append(geom("sphere", [0.05], pos=[radius * math.cos(a), radius * math.sin(a), 0.0], group=3))      # (group 3: the depth cameras' table takes 128 geoms)
    q = [pose(np.append(rng.uniform(-0.3, 0.3, 2), rng.uniform(-0.01, 0.01)), ypr(rng.uniform(-3, 3), rng.uniform(-0.01, 0.01), rng.uniform(-0.01, 0.01))) for _ in range(E)]
    return [case("chunks", make_scene(world, [_laser()], 0, fan(180)), q)]


# ------------------------------------------------------------------------------------------------ (f)
def cull(E=6, seed=6):
    rng = np.random.default_rng(seed)
    r = 0.1
    # a probe body that shares the laser's pose: its spheres sit at fixed heights above and below the scan plane, on rays of the fan
    probe = [geom("sphere", [r], pos=[1.5, 0, r - 0.002]), geom("sphere", [r], pos=[0, 1.5, r + 0.002]),
             geom("sphere", [r], pos=[-1.5, 0, -(r - 0.002)]), geom("sphere", [r], pos=[0, -1.5, -(r + 0.002)]),
             geom("box", [0.1, 0.1, 0.1], pos=[1.2, 1.2, 0.3]), geom("mesh", mesh="tet", pos=[-1.2, 1.2, 0.36])]
    world = [geom("plane", (0, 0), pos=[0, 0, -1.2]), geom("capsule", [0.1, 3.0], pos=[2.5, 0.5, 1.0], quat=ypr(0.2, 0.9, 0.1)),
             geom("box", [0.3, 0.4, 0.5], pos=[-2.5, 1.0, 0.2], quat=ypr(0.5, 0.2, 0.1)), geom("mesh", mesh="ico", pos=[0.5, -2.5, -0.1]),
             geom("cylinder", [0.2, 1.5], pos=[-1.5, -2.0, 0.5], quat=ypr(0.1, 0.7, 0.0)), geom("ellipsoid", [0.5, 0.3, 0.8], pos=[2.0, 2.5, 0.3])]
    q = []
    for e in range(E):
        lp = pose(rng.uniform(-0.2, 0.2, 3), ypr(rng.uniform(-3, 3), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5)))
        q.append(np.concatenate([lp, lp]))
    flat = case("cull on", make_scene(world, [_laser(), body("probe", probe)], 0, fan(360)), q)
    cones = fan(36, math.radians(20)) + fan(36, -math.radians(20))
    q2 = [pose(rng.uniform(-0.2, 0.2, 3), ypr(rng.uniform(-3, 3), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3))) for _ in range(E)]
    ring = [([0.1 * math.cos(a), 0.1 * math.sin(a), 0.0], ray_site(a)[1]) for a in np.linspace(0, 2 * math.pi, 36, endpoint=False)]   # origins on a ring: one plane, not one point
    return [flat, case("cull off: cones", make_scene(world, [_laser()], 0, cones), q2), case("ring of origins", make_scene(world, [_laser()], 0, ring), q2)]


# ------------------------------------------------------------------------------------------------ (g)
def welded(E=4, seed=7):
    rng = np.random.default_rng(seed)
    shapes = [geom("sphere", [0.15]), geom("capsule", [0.08, 0.2]), geom("ellipsoid", [0.2, 0.1, 0.15]), geom("cylinder", [0.1, 0.2]), geom("box", [0.1, 0.15, 0.12]),
              geom("mesh", mesh="tet"), geom("mesh", mesh="ico")]
    carried = []
    for i, g in enumerate(shapes):      # 1 m ahead of the laser, every 40 degrees, each with its own frame in the child body
        a = math.radians(40 * i)
        carried.append(dict(g, pos=[math.cos(a) - 0.05, math.sin(a) + 0.1, 0.02 * i - 0.32], quat=random_quat(rng).tolist()))
    own = [geom("box", [0.05, 0.3, 0.3], pos=[0.5, 0, 0])]       # on the site's own body, in the way of the rays ahead: never seen
    world = [geom("plane", (0, 0), pos=[0, 0, -0.8]), geom("box", [0.3, 0.3, 0.3], pos=[-2.0, 0.5, 0.0], alpha=0.0),      # invisible, in front of ...
             geom("box", [0.3, 0.6, 0.4], pos=[-3.0, 0.5, 0.0], group=3), geom("sphere", [0.4], pos=[0.5, -3.0, 0.1], group=3)]
    bodies = [_laser(own), body("mount", carried, pos=[0.05, -0.1, 0.3], quat=ypr(0.1, 0.05, -0.02).tolist(), free=False, parent=0), body("bfree", [geom("cylinder", [0.2, 0.4])])]
    q = [np.concatenate([pose(rng.uniform(-0.2, 0.2, 3), ypr(rng.uniform(-3, 3), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2))), pose([2.0 + 0.1 * e, 2.0, 0.0], random_quat(rng))]) for e in range(E)]
    carried_case = case("geoms carried by the laser", make_scene(world, bodies, 0, fan(72)), q)
    # the laser welded to the world: a jointless body over a floor and world geoms of every type
    ring = []
    every = [geom("sphere", [0.3]), geom("capsule", [0.15, 0.4]), geom("ellipsoid", [0.4, 0.25, 0.3]), geom("cylinder", [0.25, 0.3]), geom("box", [0.3, 0.25, 0.2]),
             geom("mesh", mesh="ico"), geom("mesh", mesh="tet"), geom("mesh", mesh="quad"), geom("plane", (0.5, 0.4))]
    for i, g in enumerate(every):
        a = 2 * math.pi * i / len(every)
        quat = random_quat(rng) if g["type"] != "plane" else qmul(axis_quat([0, 0, 1], a + math.pi), axis_quat([0, 1, 0], -1.2))      # the finite plane faces the laser
        ring.append(dict(g, pos=[2.2 * math.cos(a) + 0.3, 2.2 * math.sin(a) - 0.2, 0.35 + 0.03 * i], quat=np.asarray(quat).tolist()))
    fixed = [body("laser", [], pos=[0.3, -0.2, 0.4], quat=ypr(0.4, 0.1, -0.15).tolist(), free=False), body("bfree", [geom("box", [0.2, 0.2, 0.2])])]
    q2 = [pose([1.0 + 0.1 * e, -0.3, 0.4], random_quat(rng)) for e in range(E)]
    return [carried_case, case("laser welded to the world", make_scene([geom("plane", (0, 0), pos=[0, 0, 0])] + ring, fixed, 0, fan(72)), q2)]


BUILDERS = dict(types=types, inside=inside, aligned=aligned, far_thin=far_thin, chunks=chunks, cull=cull, welded=welded)
AIMED = ("aligned", "far_thin")     # their rays are aimed: no grazing ray at all
