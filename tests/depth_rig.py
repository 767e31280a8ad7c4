"""Robot-less scenes with a depth camera, as plain data: tests/depth_ref.py reads the data, the MJCF compiled for the oracle and the
device is written from the same data by ray_rig's writer (which names the geoms g000 .. in the order of depth_ref.geoms_of and adds
the <camera>).  TEST INFRASTRUCTURE.  Gravity is off and no geom collides, so one step moves nothing.  <statistic extent="2"/> and
<visual><map znear="0.01" zfar="6"/> pin the clip planes where the compiler reads them: ZNEAR = 0.02 m, ZFAR = 12 m; the d435i's
limit LIMIT = 10 m.  The camera's body also carries one lidar site, so that the models load like ray_rig's.

The builders, one per property of the depth path (each returns a list of cases; a case = ray_rig.case plus width, height, fovy):
  types()      every geom type once in the world and once on a free body, non-identity frames; camera on a free body, pitched and rolled
  near()       each closed type straddling the near plane; the eye inside each closed type; a large open sheet crossing the near plane
  large()      160 x 120: a box face, an open triangle and a long thin triangle whose candidate boxes exceed 16384 pixels
  list_full()  384 long front-facing triangles round the optical axis, each cut by the near plane and on screen: more than HLCAP;
               and at 160 x 120 with four triangles over 16384 pixels that compete for the full list
  far_thin()   r = 1, 2, 5 cm at 3, 6, 9.9 m on the rays of chosen pixels, every sphere also 0.9 r beside its ray in four directions;
               either side of the limit; beyond the far plane
  capacity()   128 camera-visible geoms, each aimed at by a pixel (capacity_overflow(): 129, which must not load)
  cull()       a long capsule with one end behind the eye plane, a flat box under the eye, geoms at a tile corner, a far big sphere
  layer()      every type on the camera's own body and a jointless child, the body moved between two renders of one context;
               a camera welded to the world; alpha 0 and group 3
  aligned()    an identity camera body, quarter-turn camera frame, dyadic positions: faces head-on, the floor at the horizon"""
import functools
import math

import numpy as np

import depth_ref
import ray_ref
import ray_rig
from ray_rig import MESHES, axis_quat, body, geom, pose, qmul, random_quat, ypr

ZNEAR, ZFAR, LIMIT = 0.02, 12.0, 10.0
HEADER = '<statistic extent="2"/><visual><map znear="0.01" zfar="6"/></visual>'
W, H, FOVY = 81, 51, 58.0
HLCAP, RASTER_MAX_BOX = 256, 16384        # csrc/smj_render.hip: the builders' own conditions are stated against them
RASTERISED = ("mesh", "box")             # what depth_raster = 1 puts into the z-buffer

OWN_MESHES = {}


def _mesh(name, vertex, face, convex=False, eye=None):
    """`eye`: a point every triangle is turned to face (counter-clockwise seen from it)."""
    vertex, face = np.asarray(vertex, np.float32).astype(np.float64), [list(map(int, f)) for f in face]
    for t in face:
        a, b, c = vertex[t]
        if eye is not None and np.dot(np.cross(b - a, c - a), np.asarray(eye, np.float64) - a) < 0:
            t[1], t[2] = t[2], t[1]
    OWN_MESHES[name] = dict(vertex=np.asarray(vertex, np.float32).astype(np.float64).tolist(), face=[list(map(int, f)) for f in face], convex=convex)
    return geom("mesh", mesh=name)


def mat_quat(m):
    """Unit quaternion of a rotation matrix (columns = the frame's axes)."""
    m = np.asarray(m, np.float64)
    q = np.array([1 + m[0, 0] + m[1, 1] + m[2, 2], m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]])
    if q[0] < 1e-3:      # near a half turn: from the largest diagonal entry
        k = int(np.argmax(np.diag(m)))
        i, j = (k + 1) % 3, (k + 2) % 3
        q = np.zeros(4)
        q[1 + k] = 1 + m[k, k] - m[i, i] - m[j, j]
        q[1 + i], q[1 + j], q[0] = m[i, k] + m[k, i], m[j, k] + m[k, j], m[j, i] - m[i, j]
    return q / np.linalg.norm(q)


def look(direction, up=(0, 0, 1)):
    """Quaternion of a camera frame (x right, y up, looking down -z) that looks along `direction`."""
    f = np.asarray(direction, np.float64) / np.linalg.norm(direction)
    x = np.cross(f, up); x /= np.linalg.norm(x)
    return mat_quat(np.stack([x, np.cross(x, f), -f], 1))


def camera(body_index=0, pos=(0, 0, 0), quat=(1, 0, 0, 0), fovy=FOVY):
    return dict(body=body_index, pos=[float(x) for x in pos], quat=[float(x) for x in quat], fovy=float(fovy))


def make_scene(world, bodies, cam):
    world, bodies = [dict(g) for g in world], [dict(b, geoms=[dict(g) for g in b["geoms"]]) for b in bodies]
    for k, (_, g) in enumerate(depth_ref.geoms_of(dict(world=world, bodies=bodies))):
        g["name"] = f"g{k:03d}"
    used = {g["mesh"] for _, g in depth_ref.geoms_of(dict(world=world, bodies=bodies)) if g["mesh"]}
    return dict(world=world, bodies=bodies, laser=cam["body"], sites=[ray_rig.ray_site(0.0)], cutoff=ray_rig.CUTOFF, cameras=[cam], header=HEADER,
                meshes={k: (MESHES.get(k) or OWN_MESHES[k]) for k in sorted(used)})


def case(name, scene, q64, width=W, height=H, then=None):
    """`then`: a second qpos [E, nq] rendered after the first in the same context."""
    c = ray_rig.case(name, scene, q64)
    c.update(width=width, height=height, fovy=scene["cameras"][0]["fovy"], then=None if then is None else np.asarray(then, np.float64))
    return c


def args(c):
    return (0, c["width"], c["height"], c["fovy"], ZNEAR, ZFAR)


def camera_pose(scene, q):
    """(eye [3], rotation matrix [3, 3]) of the camera for one qpos row."""
    cam = scene["cameras"][0]
    p, qt = ray_ref._compose(*ray_ref.body_poses(scene, np.asarray(q, np.float64)[None])[cam["body"]], cam["pos"], cam["quat"])
    return p[0], np.stack([ray_ref._rotate(qt[0], e) for e in np.eye(3)], 1)


def pixel_ray(cam, u, v, width=W, height=H):
    """Camera-frame direction of pixel (u, v), rotated by the camera's own quaternion (body frame of the camera's body)."""
    th = math.tan(math.radians(cam["fovy"]) / 2)
    dc = np.array([((u + 0.5) / width * 2 - 1) * th * width / height, (1 - (v + 0.5) / height * 2) * th, -1.0])
    return ray_ref._rotate(ray_ref._unit(cam["quat"]), dc)


# ------------------------------------------------------------------------------------------------ the three sides
def blob(scene):
    return ray_rig.blob(scene)


def geom_ids(model_names, scene):
    """compiled geom id -> index into depth_ref.geoms_of(scene), through the names; -1 stays -1."""
    names = list(model_names["geom"])
    table = np.full(len(names) + 1, -2)
    for k, (_, g) in enumerate(depth_ref.geoms_of(scene)):
        table[names.index(g["name"])] = k
    table[-1] = -1
    return table


def oracle_views(c):
    """[dict(raw, lim, gid)] of images [E, H, W] from the fp64 oracle (its images are fp32)."""
    import json

    from oracle.oracle import Oracle
    from stretch_mujoco_amd import model_blob

    b = blob(c["scene"])
    table = geom_ids(json.loads(model_blob.get_str(model_blob.loads(b), "names_json")), c["scene"])
    o = Oracle(b)
    out = dict(raw=[], lim=[], gid=[])
    for q in np.asarray(c["q32"], np.float64):
        o.arr("qpos")[:] = q
        o.forward()
        out["raw"].append(o.render_depth(0, c["width"], c["height"], c["fovy"], 0.0).astype(np.float64))
        out["lim"].append(o.render_depth(0, c["width"], c["height"], c["fovy"], LIMIT).astype(np.float64))
        out["gid"].append(table[o.render_geomid(0, c["width"], c["height"], c["fovy"])[0]])
    o.close()
    return [{k: np.array(v) for k, v in out.items()}]


def device_views(c):
    """[dict(raster_raw, raster_lim, ray_raw, ray_lim, gid, qpos)] per qpos of the case (the second, `then`, in the same
    contexts as the first).  One context per depth_raster setting: the camera-static layer is cached per context, and is built by
    whichever path renders first."""
    import ctypes

    import torch

    from stretch_mujoco_amd import StretchBatchSimulator, lib

    L = lib.load()
    b = blob(c["scene"])
    qs = [c["q32"]] + ([c["then"].astype(np.float32)] if c["then"] is not None else [])
    E, Wd, Ht = len(c["q32"]), c["width"], c["height"]
    out = [dict() for _ in qs]
    for raster in (1, 0):
        sim = StretchBatchSimulator(num_envs=E, device="cuda:0", model_blob_bytes=b)
        sim.start(home=False)
        sim.set_option("depth_raster", raster)
        table = geom_ids(sim.names, c["scene"])
        for k, q in enumerate(qs):
            sim.qpos[:] = torch.tensor(np.ascontiguousarray(np.asarray(q, np.float32).T), device=sim.device)
            sim.qvel.zero_()
            sim.step(1)
            out[k]["qpos"] = sim.qpos.t().cpu().numpy().astype(np.float64)
            for tag, limit in (("raw", 0.0), ("lim", LIMIT)):
                img = torch.full((E, Ht, Wd), -7.0, dtype=torch.float32, device=sim.device)
                assert L.smj_render_depth(sim._ctx, 0, Wd, Ht, float(c["fovy"]), float(limit), ctypes.c_void_p(img.data_ptr()), sim._stream()) == 0, L.smj_last_error(sim._ctx)
                torch.cuda.synchronize()
                out[k][("raster_" if raster else "ray_") + tag] = img.cpu().numpy().astype(np.float64)
            if not raster:
                gid = torch.full((E, Ht, Wd), -7, dtype=torch.int32, device=sim.device)
                rgb = torch.zeros(E, Ht, Wd, 3, dtype=torch.uint8, device=sim.device)
                assert L.smj_render_rgb(sim._ctx, 0, Wd, Ht, float(c["fovy"]), ctypes.c_void_p(rgb.data_ptr()), ctypes.c_void_p(gid.data_ptr()), sim._stream()) == 0
                torch.cuda.synchronize()
                out[k]["gid"] = table[gid.cpu().numpy()]
        sim.stop()
    return out


@functools.lru_cache(maxsize=None)
def reference(builder):
    """(cases, [per case: list per qpos of (raw, geom, graze)], floor) -- computed once per process and builder, never changed."""
    cases = BUILDERS[builder]()
    refs = [[depth_ref.view(c["scene"], q, *args(c)) for q in [c["q32"].astype(np.float64)] + ([c["then"].astype(np.float32).astype(np.float64)] if c["then"] is not None else [])]
            for c in cases]
    floor = max(depth_ref.floor(c["scene"], c["q64"], *args(c)) for c in cases)
    return cases, refs, floor


def compare(builder, images, bound="device"):
    """The rule of every test.  `images`: per case, per qpos, a dict of images [E, H, W] keyed raster_raw / raster_lim / ray_raw /
    ray_lim / gid (device) or raw / lim / gid (oracle).  Grazing pixels (the reference alone names them) are left out and capped at
    1 % of the test's pixels and 2 % of any one image -- at zero for the aimed builders.  On every other pixel hit or miss agrees
    exactly, the geom id agrees exactly and the depth is within the bound:
      device   min(16 x the input-rounding floor, ceiling) -- on the pixels that depth_raster = 1 rasterises (meshes, boxes) the
               ceiling itself, the project's 1e-4 + 1e-4 z;
      oracle   2 ulp of the fp32 value it stores.
    Returns dict(floor, worst per path, ratio, grazing, pixels) after asserting; prints it first."""
    cases, refs, floor = reference(builder)
    stat = dict(floor=floor, pixels=0, grazing=0, worst={}, flips=[], over=[])
    for c, per_q, ref_q in zip(cases, images, refs):
        kind = np.array([g["type"] for _, g in depth_ref.geoms_of(c["scene"])] + ["none"])
        for imgs, (raw, who, graze) in zip(per_q, ref_q):
            lim, who_lim, graze_lim = depth_ref.limited(raw, who, graze, LIMIT, ZFAR)
            g_raw, g_lim = graze < ray_ref.GRAZE, graze_lim < ray_ref.GRAZE
            per_image = g_lim.reshape(len(raw), -1).mean(1)
            assert per_image.max() <= (0.0 if builder in AIMED else 0.02), (c["name"], "grazing pixels per image", per_image)
            stat["pixels"] += raw.size; stat["grazing"] += int(g_lim.sum())
            rasterised = np.isin(kind[who], RASTERISED)
            for key, got in imgs.items():
                if key == "qpos":
                    continue
                if key == "gid":
                    bad = ~g_raw & (got != who)
                    stat["flips"] += [(c["name"], key, int(e), int(v), int(u), int(got[e, v, u]), int(who[e, v, u])) for e, v, u in zip(*np.nonzero(bad))]
                    continue
                limited_image = key.endswith("lim")
                ref, idx, gz = (lim, who_lim, g_lim) if limited_image else (raw, who, g_raw)
                miss = 0.0 if limited_image else ZFAR
                bad = ~gz & ((got == miss) != (idx < 0))
                stat["flips"] += [(c["name"], key, int(e), int(v), int(u), float(got[e, v, u]), float(ref[e, v, u])) for e, v, u in zip(*np.nonzero(bad))]
                ceiling = 1e-4 + 1e-4 * np.abs(ref)
                if bound == "oracle":
                    allowed = 2 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
                else:
                    allowed = np.where(rasterised & key.startswith("raster"), ceiling, np.minimum(16 * floor, ceiling))
                err = np.where(gz | bad, 0.0, np.abs(got - ref))
                path = key if bound == "oracle" else ("rasterised" if key.startswith("raster") else "ray")
                for name, sel in ((path, rasterised if path == "rasterised" else np.ones_like(rasterised)), ("ray", ~rasterised if path == "rasterised" else np.zeros_like(rasterised))):
                    if sel.any():
                        stat["worst"][name] = max(stat["worst"].get(name, 0.0), float(err[sel].max()))
                stat["over"] += [(c["name"], key, int(e), int(v), int(u), float(got[e, v, u]), float(ref[e, v, u]), float(allowed[e, v, u]), str(kind[who[e, v, u]])) for e, v, u in zip(*np.nonzero(err > allowed))]
    ratio = {k: (w / floor if floor else float("nan")) for k, w in stat["worst"].items()}
    print(f"{builder}: pixels {stat['pixels']} grazing {stat['grazing']} floor {floor:.3e} worst " + " ".join(f"{k} {w:.3e} ({ratio[k]:.1f} x)" for k, w in stat["worst"].items()) +
          f" hit/miss or id flips {len(stat['flips'])} over the bound {len(stat['over'])}")
    if stat["over"]:
        print("  over the bound, per image kind:", {k: sum((o[1], o[8]) == k for o in stat["over"]) for k in sorted({(o[1], o[8]) for o in stat["over"]})},
              "largest excess", max(stat["over"], key=lambda o: abs(o[5] - o[6]) / o[7]))
    assert stat["grazing"] <= (0 if builder in AIMED else 0.01 * stat["pixels"]), ("grazing pixels", stat["grazing"], stat["pixels"])
    assert not stat["flips"], (len(stat["flips"]), stat["flips"][:10])
    assert not stat["over"], (len(stat["over"]), stat["over"][:10])
    stat["ratio"] = ratio
    return stat


# ------------------------------------------------------------------------------------------------ shapes
KINDS = {"sphere": geom("sphere", [0.35]), "capsule": geom("capsule", [0.2, 0.4]), "ellipsoid": geom("ellipsoid", [0.5, 0.3, 0.2]),
         "cylinder": geom("cylinder", [0.3, 0.35]), "box": geom("box", [0.4, 0.3, 0.25]), "ico": geom("mesh", mesh="ico"), "tet": geom("mesh", mesh="tet"),
         "quad": geom("mesh", mesh="quad")}
CLOSED = ("sphere", "capsule", "ellipsoid", "cylinder", "box", "ico", "tet")


def _cam_body(geoms=(), **kw):
    return body("cam", geoms, **kw)


def _facing(direction, tilt, spin):
    """A frame whose +z points along `direction`, tilted and spun."""
    return qmul(qmul(look(-np.asarray(direction, np.float64)), axis_quat([1, 0, 0], tilt)), axis_quat([0, 0, 1], spin))


_STAGE_T, _STAGE_R = np.array([0.11, -0.07, 0.05]), ypr(0.3, -0.2, 0.1)


def _stage(geoms, name="stage"):
    """A free body for geoms given in the frame of the camera's body: its own frame is offset from that body's, so that the two poses
    round to fp32 independently (`_stage_pose` of the camera body's pose puts it where the geoms are meant)."""
    inv = _STAGE_R * depth_ref._CONJ
    return body(name, [dict(g, pos=ray_ref._rotate(inv, np.asarray(g["pos"]) - _STAGE_T).tolist(), quat=qmul(inv, ray_ref._unit(g["quat"])).tolist()) for g in geoms])


def _stage_pose(p):
    return pose(p[:3] + ray_ref._rotate(ray_ref._unit(p[3:]), _STAGE_T), qmul(ray_ref._unit(p[3:]), _STAGE_R))


# ------------------------------------------------------------------------------------------------ types
def types(E=6, seed=11):
    """The camera near the origin looks along +x; nine world geoms on a 3 x 3 grid 3.5 m ahead, three free bodies 1.9 m ahead.  Planes
    are in the world only: a plane belongs to the world body (MuJoCo's compiler refuses one on a moving body); layer() has a finite plane
    under a camera welded to the world, where the camera-static layer composes its frame."""
    rng = np.random.default_rng(seed)
    order = list(KINDS) + ["quad back"]
    cases = []
    for k, (plane, free) in enumerate([((0, 0), ["cylinder", "box", "ico"]), ((4.0, 3.0), ["sphere", "capsule", "ellipsoid"]), ((0, 2.5), ["tet", "quad", "quad back"])]):
        world = [geom("plane", plane, pos=[3.0, 0.1, -1.3], quat=ypr(0.3, 0.04, -0.03))]
        for i, n in enumerate(order):
            at = [3.5 + 0.15 * (i % 2), 1.25 * (i % 3 - 1), 0.95 * (i // 3 - 1) + 0.1]
            if n.startswith("quad"):      # the open quad shows its front (+z of its frame) to the camera, or its back
                quat = _facing([-1, 0, 0] if n == "quad" else [1, 0, 0], 0.3, 0.4 * i)
            else:
                quat = random_quat(rng)
            world.append(dict(KINDS[n.split()[0]], pos=at, quat=np.asarray(quat).tolist()))
        cam = camera(0, pos=[0.03, -0.02, 0.05], quat=qmul(look([1, 0, 0]), ypr(0.05, -0.04, 0.03)))
        bodies = [_cam_body()] + [body("b" + n.replace(" ", ""), [dict(KINDS[n.split()[0]], pos=[0.05, -0.03, 0.04], quat=random_quat(rng).tolist())]) for n in free]
        q = []
        for e in range(E):
            row = [pose(rng.uniform(-0.15, 0.15, 3), ypr(rng.uniform(-0.12, 0.12), rng.uniform(-0.12, 0.12), rng.uniform(-0.3, 0.3)))]
            for i, n in enumerate(free):
                at = [1.9 + rng.uniform(-0.1, 0.1), 0.62 * (i - 1) + rng.uniform(-0.05, 0.05), rng.uniform(-0.3, -0.2) + 0.45 * (i % 2)]
                quat = random_quat(rng) if not n.startswith("quad") else _facing([-1, 0, 0] if n == "quad" else [1, 0, 0], rng.uniform(-0.4, 0.4), rng.uniform(-3, 3))
                row.append(pose(at, quat))
            q.append(np.concatenate(row))
        cases.append(case(f"types{k}", make_scene(world, bodies, cam), q))
    return cases


# ------------------------------------------------------------------------------------------------ near
def _surface_point(g, meshes, u):
    """The point where the ray from 2 u towards the geom's centre enters it (geom frame)."""
    u = np.asarray(u, np.float64) / np.linalg.norm(u)
    x, _, _ = depth_ref.enter_geom(g, meshes, 2.0 * u[None], -u[None], np.zeros(1))
    assert x[0] > 0
    return (2.0 - x[0]) * u


_SHEET = _mesh("sheet", [[-0.3, -0.25, 0.05], [0.4, -0.2, -0.6], [-0.1, 0.5, -0.9], [0.5, 0.45, -0.2]], [[0, 1, 2], [1, 3, 2]], eye=[0, 0, 0])      # two large triangles, folded; vertex 0 is behind the eye plane


def near(seed=12):
    rng = np.random.default_rng(seed)
    inside_at = dict(sphere=[0.1, -0.05, 0.1], capsule=[0.03, -0.02, 0.47], ellipsoid=[0.2, 0.05, -0.04], cylinder=[0.1, 0.1, -0.2], box=[-0.2, 0.1, 0.15], ico=[0.05, 0.02, -0.03], tet=[0.01, 0.0, 0.02])
    world, frames = [geom("plane", (0, 0), pos=[0, 0, -0.9])], []
    for i, n in enumerate(CLOSED):
        a = 2 * math.pi * i / len(CLOSED)
        gq, gp = random_quat(rng), np.array([4 * math.cos(a), 4 * math.sin(a), 0.3 * math.sin(3 * a)])
        world.append(dict(KINDS[n], pos=gp.tolist(), quat=gq.tolist()))
        frames.append((gp, gq))
    world += [geom("box", [0.5, 0.4, 0.6], pos=[0.2, -0.1, 0.0], quat=ypr(0.4, 0.1, 0.2)), geom("sphere", [0.4], pos=[-0.3, 0.5, 0.8])]      # what lies behind, at the ring's centre
    meshes = dict(MESHES)
    q_in, q_out = [], []
    for (gp, gq), n in zip(frames, CLOSED):
        eye = gp + ray_ref._rotate(gq, np.asarray(inside_at[n], float))
        q_in.append(pose(eye, qmul(look(-eye + rng.uniform(-0.3, 0.3, 3)), axis_quat([0, 0, 1], rng.uniform(-0.3, 0.3)))))
        # outside, 15 mm from the surface on the side of the ring's centre, looking back through the shape at a slant: the entry depth
        # runs from below to above the near plane across the image
        u = ray_ref._rotate(gq * depth_ref._CONJ, -gp / np.linalg.norm(gp)) + rng.uniform(-0.2, 0.2, 3)
        u /= np.linalg.norm(u)
        ps = _surface_point(KINDS[n], meshes, u)
        a, b = np.cross(u, [0.3, 0.5, 0.8]), np.cross(u, np.cross(u, [0.3, 0.5, 0.8]))
        nrm = np.cross(_surface_point(KINDS[n], meshes, u + 1e-4 * a) - ps, _surface_point(KINDS[n], meshes, u + 1e-4 * b) - ps)      # the surface normal there
        nrm *= np.sign(nrm @ u) / np.linalg.norm(nrm)
        w = np.cross(nrm, [0.3, 0.5, 0.8]); w /= np.linalg.norm(w)
        eye = gp + ray_ref._rotate(gq, ps + 0.015 * nrm)
        u = nrm
        q_out.append(pose(eye, look(ray_ref._rotate(gq, -u + 0.7 * w))))
    cam = camera(0)
    scene = make_scene(world, [_cam_body()], cam)
    # the sheet on the camera's own body (the static layer) and on a free body that shares its pose (the per-env pass), over the floor
    slant = make_scene([geom("plane", (0, 0), pos=[0, 0, -1.5]), geom("box", [0.6, 0.5, 0.4], pos=[3.0, 0.3, 0.0], quat=ypr(0.3, 0.2, 0.1))],
                       [_cam_body([dict(_SHEET, pos=[0.0, 0.0, 0.0])]), body("carrier", [dict(_SHEET, pos=[0.25, -0.3, 0.1], quat=axis_quat([0, 0, 1], 2.4).tolist())])],
                       camera(0))
    q_s = []
    for e in range(4):
        p = pose(rng.uniform(-0.2, 0.2, 3), qmul(look([1, 0.1 * e, -0.1]), axis_quat([0, 0, 1], rng.uniform(-0.4, 0.4))))
        q_s.append(np.concatenate([p, p]))
    return [case("straddling the near plane", scene, q_out), case("eye inside", scene, q_in), case("sheet across the near plane", slant, q_s)]


# ------------------------------------------------------------------------------------------------ large
_BIGTRI = _mesh("bigtri", [[-1.9, -1.3, -2.0], [2.0, -1.25, -2.2], [-1.8, 1.35, -1.9], [-2.5, -1.8, -2.5]], [[0, 1, 2], [0, 2, 3]], eye=[0, 0, 0])      # camera frame: the lower-left half of the screen
_SLIVER = _mesh("sliver", [[-1.0, -0.68, -1.3], [-0.97, -0.72, -1.3], [1.15, 0.8, -1.5], [1.2, 0.9, -1.45]], [[0, 1, 2], [1, 3, 2]], eye=[0, 0, 0])    # long and thin along the diagonal


def large():
    cam = camera(0, fovy=FOVY)
    # everything on a free body placed in the camera body's frame; the camera frame is the body frame
    back = geom("box", [4.0, 3.0, 0.2], pos=[0.2, -0.1, -3.4], quat=ypr(0.05, 0.1, -0.08))      # its near face fills the screen
    scene = make_scene([], [_cam_body(), _stage([back, _BIGTRI, _SLIVER])], cam)
    p = pose([0.3, -0.2, 0.9], ypr(0.4, -0.3, 0.2))
    return [case("large", scene, [np.concatenate([p, _stage_pose(p)])], width=160, height=120)]


def screen_boxes(c):
    """Candidate pixels (pixel centres in the screen box, clipped to the image) of every front-facing triangle of the case's open
    meshes and of the box faces nearest the eye, env 0: {geom name: [counts]}.  Triangles with a vertex nearer than the near plane
    are left out (`cut_triangles` counts those)."""
    scene, out = c["scene"], {}
    eye, R = camera_pose(scene, c["q32"][0].astype(np.float64))
    poses = ray_ref.body_poses(scene, c["q32"][:1].astype(np.float64))
    th = math.tan(math.radians(c["fovy"]) / 2)
    for bi, g in depth_ref.geoms_of(scene):
        bp, bq = poses[bi] if bi >= 0 else (np.zeros((1, 3)), np.array([[1.0, 0, 0, 0]]))
        gp, gq = ray_ref._compose(bp, bq, g["pos"], g["quat"])
        if g["type"] == "mesh":
            m = scene["meshes"][g["mesh"]]
            verts, faces = np.asarray(m["vertex"]), m["face"]
        elif g["type"] == "box":
            s = np.asarray(g["size"])
            verts = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * s
            faces = [[4, 6, 7], [4, 7, 5], [0, 1, 3], [0, 3, 2], [2, 3, 7], [2, 7, 6], [0, 4, 5], [0, 5, 1], [1, 5, 7], [1, 7, 3], [0, 2, 6], [0, 6, 4]]      # outward
        else:
            continue
        pc = (ray_ref._rotate(np.repeat(gq, len(verts), 0), verts) + gp - eye) @ R      # camera frame
        counts = []
        for f in faces:
            a, b, cc = pc[f[0]], pc[f[1]], pc[f[2]]
            if np.dot(np.cross(b - a, cc - a), -a) <= 0 or min(-a[2], -b[2], -cc[2]) < ZNEAR:
                continue
            px = np.array([[(p[0] / -p[2] / (th * c["width"] / c["height"]) + 1) / 2 * c["width"], (1 - p[1] / -p[2] / th) / 2 * c["height"]] for p in (a, b, cc)])
            lo, hi = np.ceil(np.maximum(px.min(0) - 0.5, 0)), np.floor(np.minimum(px.max(0) - 0.5, [c["width"] - 1, c["height"] - 1]))
            counts.append(int(max(hi[0] - lo[0] + 1, 0) * max(hi[1] - lo[1] + 1, 0)))
        out[g["name"]] = counts
    return out


# ------------------------------------------------------------------------------------------------ list_full
def _tunnel(n=384, radius=4.0, back=-0.5, length=11.0):
    """n long triangles round the optical axis (camera frame, looking down -z), the inside facing the axis: each runs from behind the
    eye plane to `length` metres ahead, where it tapers to a point."""
    v, f = [], []
    for k in range(n):
        a, d = 2 * math.pi * k / n, 0.8 * math.pi / n
        v += [[radius * math.cos(a - d), radius * math.sin(a - d), -back], [radius * math.cos(a + d), radius * math.sin(a + d), -back], [radius * math.cos(a), radius * math.sin(a), -length]]
        f.append([3 * k, 3 * k + 1, 3 * k + 2])
    v = np.asarray(v, np.float32).astype(np.float64)
    for t in f:      # counter-clockwise seen from the axis
        a, b, c = v[t]
        if np.dot(np.cross(b - a, c - a), -a * [1, 1, 0]) < 0:
            t[1], t[2] = t[2], t[1]
    return v, f


_TUNNEL = _mesh("tunnel", *_tunnel())


def list_full():
    end = geom("box", [5.0, 5.0, 0.1], pos=[0.0, 0.0, -11.6], quat=ypr(0.02, 0.03, 0.0))      # closes the tunnel, inside the far plane
    scene = make_scene([], [_cam_body(), _stage([dict(_TUNNEL, pos=[0.013, -0.021, 0.0]), end])], camera(0))
    p0, p1 = pose([0.1, 0.2, 0.3], ypr(-0.2, 0.1, 0.05)), pose([0.4, -0.3, 1.1], ypr(0.7, -0.4, 0.3))
    # 160 x 120: four staggered copies of large()'s triangle in front of the tunnel.  Their boxes exceed RASTER_MAX_BOX, and they
    # compete with the 384 cut triangles for the list's 256 slots (in the order the waves arrive): those that find it full are
    # shaded by the rasteriser's wave itself
    big = []
    for k in range(4):
        v = (np.asarray(OWN_MESHES["bigtri"]["vertex"]) + [0.15 * k, 0.12 * k, 0.0]) * (1 + 0.25 * k)
        big.append(_mesh(f"bigtri{k}", v, OWN_MESHES["bigtri"]["face"], eye=[0, 0, 0]))
    crowded = make_scene([], [_cam_body(), _stage([dict(_TUNNEL, pos=[0.013, -0.021, 0.0]), end] + big)], camera(0))
    p2 = pose([-0.2, 0.3, 0.6], ypr(-0.5, 0.2, -0.1))
    return [case("list full", scene, [np.concatenate([p0, _stage_pose(p0)]), np.concatenate([p1, _stage_pose(p1)])]),
            case("list full, large boxes", crowded, [np.concatenate([p2, _stage_pose(p2)])], width=160, height=120)]


def cut_triangles(c, env=0):
    """How many front-facing triangles of the case's open meshes have a vertex nearer than the near plane and a visible part whose
    screen box holds a pixel centre: what the rasteriser hands over as cut."""
    scene = c["scene"]
    eye, R = camera_pose(scene, c["q32"][env].astype(np.float64))
    poses = ray_ref.body_poses(scene, c["q32"][env:env + 1].astype(np.float64))
    th = math.tan(math.radians(c["fovy"]) / 2)
    n = 0
    for bi, g in depth_ref.geoms_of(scene):
        if g["type"] != "mesh" or scene["meshes"][g["mesh"]]["convex"]:
            continue
        m = scene["meshes"][g["mesh"]]
        bp, bq = poses[bi] if bi >= 0 else (np.zeros((1, 3)), np.array([[1.0, 0, 0, 0]]))
        gp, gq = ray_ref._compose(bp, bq, g["pos"], g["quat"])
        pc = (ray_ref._rotate(np.repeat(gq, len(m["vertex"]), 0), np.asarray(m["vertex"])) + gp - eye) @ R
        for f in m["face"]:
            tri = pc[f]
            depth = -tri[:, 2]
            if np.dot(np.cross(tri[1] - tri[0], tri[2] - tri[0]), -tri[0]) <= 0 or depth.min() >= ZNEAR or depth.max() <= ZNEAR:
                continue
            poly = []      # the part at depth >= ZNEAR
            for i in range(3):
                p, q = tri[i], tri[(i + 1) % 3]
                if -p[2] >= ZNEAR:
                    poly.append(p)
                if (-p[2] >= ZNEAR) != (-q[2] >= ZNEAR):
                    s = (ZNEAR + p[2]) / (p[2] - q[2])
                    poly.append(p + s * (q - p))
            poly = np.array(poly)
            px = np.stack([(poly[:, 0] / -poly[:, 2] / (th * c["width"] / c["height"]) + 1) / 2 * c["width"], (1 - poly[:, 1] / -poly[:, 2] / th) / 2 * c["height"]], 1)
            lo, hi = np.ceil(np.maximum(px.min(0) - 0.5, 0)), np.floor(np.minimum(px.max(0) - 0.5, [c["width"] - 1, c["height"] - 1]))
            n += bool(hi[0] >= lo[0] and hi[1] >= lo[1])
    return n


# ------------------------------------------------------------------------------------------------ far_thin
def _aimed(cam, u, v, depth, g, r, off=(0.0, 0.0)):
    """`g` with its surface at `depth` (metres along the optical axis) on the ray of pixel (u, v), its centre `off` x r beside the ray."""
    d = pixel_ray(cam, u, v)
    scale, d = np.linalg.norm(d), d / np.linalg.norm(d)
    side = np.cross(d, [0.2, 0.3, 1.0]); side /= np.linalg.norm(side)
    up = np.cross(side, d)
    c = np.asarray(cam["pos"]) + (depth * scale + r) * d + r * (off[0] * side + off[1] * up)
    return dict(g, pos=c.tolist(), quat=mat_quat(np.stack([side, d, up], 1)).tolist())      # the geom's z axis across the ray


def far_thin(E=4, seed=14):
    rng = np.random.default_rng(seed)
    cam = camera(0, pos=[0.02, 0.01, -0.03], quat=qmul(look([1, 0, 0]), ypr(0.02, 0.05, -0.03)))
    targets, k = [], 0
    offs = [(-0.9, 0.0), (-0.45, 0.3), (0.0, 0.0), (0.6, -0.4), (0.0, 0.9)]
    for kind in ("sphere", "capsule", "cylinder", "box"):
        for r in (0.01, 0.02, 0.05):
            for dist in (3.0, 6.0, 9.9):
                u, v = 4 + 8 * (k % 10), 6 + 12 * (k // 10)      # a 10 x 4 grid of pixels, 8 and 12 apart
                size = {"sphere": [r], "capsule": [r, 0.1], "cylinder": [r, 0.1], "box": [r, r, 1.5 * r]}[kind]
                targets.append(_aimed(cam, u, v, dist, geom(kind, size), r, offs[k % 5]))
                k += 1
    # Spheres are the one type whose bounding sphere is the shape itself, so what the per-ray bounding-sphere reject drops is a lost
    # pixel: every radius at every distance again, its centre 0.9 r beside the ray, in four directions (rows between the grid's)
    beside, edge = [], [(0.9, 0.0), (0.0, -0.9), (-0.636, 0.636), (0.636, 0.636)]
    for r in (0.01, 0.02, 0.05):
        for dist in (3.0, 6.0, 9.9):
            for off in edge:
                u, v = 4 + 6 * (len(beside) % 12), 12 + 12 * (len(beside) // 12)
                targets.append(_aimed(cam, u, v, dist, geom("sphere", [r]), r, off))
                beside.append((u, v))
    # on the three centre columns of the last row of the grid: either side of the limit, and beyond the far plane
    marks = [(36, 45, LIMIT - 0.01), (40, 45, LIMIT + 0.01), (44, 45, ZFAR + 0.05)]
    for u, v, depth in marks:
        targets.append(_aimed(cam, u, v, depth, geom("sphere", [0.05]), 0.05))
    q = [np.concatenate([pose([0, 0, 0], [1, 0, 0, 0])] * 2)]
    for e in range(1, E):
        p = pose(rng.uniform(-1, 1, 3), random_quat(rng))
        q.append(np.concatenate([p, p]))
    c = case("far and thin", make_scene([], [_cam_body(), body("targets", targets)], cam), q)
    c["aimed"] = [(4 + 8 * (i % 10), 6 + 12 * (i // 10)) for i in range(36)] + beside
    c["marks"] = marks
    return [c]


# ------------------------------------------------------------------------------------------------ capacity
def _capacity_scene(n):
    cam = camera(0, pos=[0.01, -0.02, 0.02], quat=qmul(look([1, 0, 0]), ypr(-0.03, 0.02, 0.04)))
    shapes = [geom("sphere", [0.03]), geom("box", [0.03, 0.035, 0.03]), geom("capsule", [0.025, 0.02]), geom("cylinder", [0.03, 0.03]), geom("ellipsoid", [0.035, 0.03, 0.03])]
    targets, pixels = [], []
    for k in range(n):
        u, v = (3 + 5 * (k % 16), 3 + 6 * (k // 16)) if k < 128 else (1, 1)
        targets.append(_aimed(cam, u, v, 2.5 + 0.02 * (k % 7), shapes[k % len(shapes)], 0.025))
        pixels.append((u, v))
    return make_scene([], [_cam_body(), body("targets", targets)], cam), pixels


def capacity(seed=16):
    rng = np.random.default_rng(seed)
    scene, pixels = _capacity_scene(128)
    q = [np.concatenate([pose([0, 0, 0], [1, 0, 0, 0])] * 2)]
    p = pose(rng.uniform(-1, 1, 3), random_quat(rng))
    q.append(np.concatenate([p, p]))
    c = case("128 geoms", scene, q)
    c["aimed"] = pixels
    return [c]


def capacity_overflow():
    return _capacity_scene(129)[0]


# ------------------------------------------------------------------------------------------------ cull
def cull(E=6, seed=17):
    rng = np.random.default_rng(seed)
    cam = camera(0, pos=[0.02, 0.0, 0.03], quat=look([1, 0, 0]))
    th = math.tan(math.radians(FOVY) / 2)
    probe = []
    for (u, v), shift in (((16, 16), 0.35), ((64, 16), -0.35), ((32, 32), 0.35), ((48, 16), -0.35), ((64, 32), 0.35), ((16, 32), -0.35)):
        # a sphere beside the corner (u, v) of the 16-pixel (and, at 64, the 64-pixel) tiles: its silhouette crosses the tile's edge by
        # `shift` pixels, or stays that far short of it
        depth, r = 2.0, 0.12
        px = 2 * th * depth / H                                  # metres per pixel at that depth
        d = pixel_ray(cam, u - 0.5 - (r / px) + shift, v - 0.5 - (r / px) * 0.3)
        probe.append(geom("sphere", [r], pos=(np.asarray(cam["pos"]) + depth * d).tolist()))
    probe.append(geom("sphere", [1.5], pos=(np.asarray(cam["pos"]) + 11.0 * pixel_ray(cam, 60, 12)).tolist()))      # centre beyond the limit, surface within
    world = [geom("plane", (0, 0), pos=[0, 0, -1.2]),
             geom("capsule", [0.1, 3.0], pos=[1.6, 0.9, 0.15], quat=_facing([0.8, 0.55, 0.1], 0.0, 0.0).tolist()),      # crosses the view, one end behind the eye plane
             geom("box", [3.0, 3.0, 0.05], pos=[0.5, 0.0, -0.4], quat=ypr(0.2, 0.02, -0.03)),      # wide and flat under the camera: the eye is inside its bounding sphere
             geom("box", [0.3, 0.4, 0.5], pos=[3.5, -1.0, 0.2], quat=ypr(0.5, 0.2, 0.1)), geom("mesh", mesh="ico", pos=[2.5, 0.8, -0.1]),
             geom("cylinder", [0.2, 1.5], pos=[4.5, 0.5, 0.5], quat=ypr(0.1, 0.7, 0.0)), geom("ellipsoid", [0.5, 0.3, 0.8], pos=[5.0, -2.0, 0.3])]
    q = []
    for e in range(E):
        p = pose(rng.uniform(-0.15, 0.15, 3), ypr(rng.uniform(-0.25, 0.25), rng.uniform(-0.2, 0.2), rng.uniform(-0.3, 0.3)))
        q.append(np.concatenate([p, p]))
    return [case("cull", make_scene(world, [_cam_body(), body("probe", probe)], cam), q)]


# ------------------------------------------------------------------------------------------------ layer
def layer(E=4, seed=18):
    rng = np.random.default_rng(seed)
    small = [geom("sphere", [0.08]), geom("capsule", [0.04, 0.1]), geom("ellipsoid", [0.1, 0.05, 0.07]), geom("cylinder", [0.05, 0.1]), geom("box", [0.05, 0.08, 0.06]),
             geom("mesh", mesh="tet"), geom("mesh", mesh="ico")]
    cam = camera(0, pos=[0.0, 0.02, 0.05], quat=qmul(look([1, 0, 0]), ypr(0.02, -0.03, 0.05)))

    def ahead(g, i, n, depth, spread):      # in front of the camera (body frame: +x), on a ring about the axis
        a = 2 * math.pi * i / n
        s = 0.4 if g["type"] == "mesh" else 1.0
        return dict(g, pos=[depth + 0.03 * i, spread * math.cos(a), spread * math.sin(a) + 0.05], quat=random_quat(rng).tolist()), s

    own = [ahead(g, i, len(small), 0.8, 0.3)[0] for i, g in enumerate(small)]
    carried = [ahead(g, i + 0.5, len(small), 1.3, 0.55)[0] for i, g in enumerate(small)]
    world = [geom("plane", (0, 0), pos=[0, 0, -0.8]), geom("box", [0.3, 0.3, 0.3], pos=[2.0, 0.1, 0.0], alpha=0.0),      # invisible, in front of ...
             geom("box", [0.3, 0.6, 0.4], pos=[3.0, 0.1, 0.0]), geom("sphere", [0.3], pos=[1.6, -0.5, 0.3], group=3), geom("cylinder", [0.3, 0.5], pos=[3.0, 1.5, 0.0])]
    bodies = [_cam_body(own), body("mount", carried, pos=[0.05, -0.02, 0.03], quat=ypr(0.05, 0.03, -0.02).tolist(), free=False, parent=0), body("bfree", [geom("capsule", [0.15, 0.3])])]
    rows = lambda: [np.concatenate([pose(rng.uniform(-0.2, 0.2, 3), ypr(rng.uniform(-0.4, 0.4), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2))), pose([2.2 + 0.1 * e, -1.0, 0.1], random_quat(rng))]) for e in range(E)]
    carried_case = case("geoms carried by the camera", make_scene(world, bodies, cam), rows(), then=rows())
    # the camera welded to the world: a jointless body over a floor and world geoms of every type, one free body
    every = [geom("sphere", [0.3]), geom("capsule", [0.15, 0.4]), geom("ellipsoid", [0.4, 0.25, 0.3]), geom("cylinder", [0.25, 0.3]), geom("box", [0.3, 0.25, 0.2]),
             geom("mesh", mesh="ico"), geom("mesh", mesh="tet"), geom("mesh", mesh="quad"), geom("plane", (0.5, 0.4))]
    ring = []
    for i, g in enumerate(every):
        at = [3.2 + 0.2 * (i % 2), 1.2 * (i % 3 - 1) - 0.2, 0.7 * (i // 3) + 0.45]
        quat = random_quat(rng) if g["type"] != "plane" and g["mesh"] != "quad" else _facing([-1, 0.2, 0.1], 0.2, 0.3)
        ring.append(dict(g, pos=at, quat=np.asarray(quat).tolist()))
    fixed = [body("cam", [], pos=[0.3, -0.2, 0.4], quat=ypr(0.1, 0.1, -0.15).tolist(), free=False), body("bfree", [geom("box", [0.2, 0.2, 0.2])])]
    q2 = [pose([2.0 + 0.1 * e, -0.3, 0.4], random_quat(rng)) for e in range(E)]
    return [carried_case, case("camera welded to the world", make_scene([geom("plane", (0, 0), pos=[0, 0, 0])] + ring, fixed, cam), q2)]


# ------------------------------------------------------------------------------------------------ aligned
def aligned():
    """The camera looks along +x with z up by an exact quarter-turn frame (every component of its quaternion is +-1/2), its body at the
    identity at dyadic positions: the centre pixel's ray is exactly (0, 0, -1), the centre row is parallel to the floor."""
    cam = camera(0, quat=(0.5, 0.5, -0.5, -0.5))
    world = [geom("plane", (0, 0), pos=[0, 0, -1.0]),                                              # the floor: its horizon is the centre row
             geom("box", [0.25, 0.25, 0.25], pos=[2.0, 0.0, 0.0]),                                  # face on, on the axis
             geom("box", [0.5, 0.25, 0.25], pos=[3.0, 1.5, 0.5], quat=[0, 0, 0, 1]),                # face on, half a turn
             geom("cylinder", [0.25, 0.5], pos=[3.0, -1.0, 0.5], quat=[ray_rig.S, 0, ray_rig.S, 0]),     # axis along x: an end faces the camera
             geom("capsule", [0.125, 0.25], pos=[2.5, 1.0, -0.5], quat=[ray_rig.S, 0, ray_rig.S, 0]),    # axis along x: end on
             geom("mesh", mesh="ico", pos=[3.0, 0.0, 1.0]), geom("sphere", [0.25], pos=[2.5, -1.0, -0.5]), geom("ellipsoid", [0.25, 0.125, 0.5], pos=[4.0, 0.5, 0.0])]
    # Pixel rays have rational y : z ratios (p : q with |p| <= 40, |q| <= 25), so a ray would run exactly through an edge at y : z =
    # 5 : 3.  Fine dyadic offsets (still exact in fp32) give every edge a ratio no pixel has; chosen on the reference: no grazing pixel.
    for k, (oy, oz) in {1: (1 / 64, 3 / 128), 2: (3 / 64, 1 / 128), 3: (3 / 64, 1 / 128), 4: (1 / 64, 3 / 128), 5: (1 / 128, 3 / 64), 6: (3 / 128, 1 / 64), 7: (3 / 128, 1 / 64)}.items():
        world[k]["pos"][1] += oy; world[k]["pos"][2] += oz
    q = [pose(p, [1, 0, 0, 0]) for p in ([0, 0, 0], [0.125, 0, 0], [0, -0.125, 0.0625], [-0.25, 0.125, 0])]
    return [case("aligned",make_scene(world, [_cam_body()], cam), q)]


BUILDERS = dict(types=types, near=near, large=large, list_full=list_full, far_thin=far_thin, capacity=capacity, cull=cull, layer=layer, aligned=aligned)
AIMED = ("far_thin", "capacity", "aligned")     # their pixels are aimed: no grazing pixel at all
