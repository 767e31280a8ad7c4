"""A rangefinder scan in fp64 numpy, written from MuJoCo's documented rule alone.  TEST INFRASTRUCTURE: it imports nothing of the
package, of oracle/ or of the compiler, and restates none of their intersection formulas.

The rule ([MJ] mj_ray as the rangefinder sensor calls it): a ray from the site along the site's +Z returns the nearest intersection
over all geoms with rgba[3] != 0, in any group, except the geoms of the site's own body; either side of a surface counts (from inside
a closed shape: the exit distance); a plane is hit only from its front and only inside its half sizes where they are positive; -1
when nothing is hit; after that a positive value above a positive cutoff becomes the cutoff.

The method, chosen so that an algebra slip shared with the code under test cannot cancel:
  * convex primitives are ROOTS OF A CONVEX IMPLICIT FUNCTION along the ray -- the exact signed distance of sphere, capsule, cylinder
    and box, |p / s|^2 - 1 of the ellipsoid.  It is minimised over t >= 0 by golden section (convex, so that finds the minimum); a
    positive minimum is a miss; otherwise bisection to 1e-12 for the entry (value at 0 positive) or the exit (origin inside).
  * a plane is the root of its height by the same bisection, then the half-size test;
  * a convex mesh is clipped against the half-spaces of its faces;
  * an open mesh is brute force over its triangles (the plane of the triangle, then three same-side tests).
Every function is vectorised over rays [N, 3] in the geom's frame.  `graze` of a ray is how close, in metres, it comes to changing
between hit and miss on a geom that could change its answer, or to an edge of a mesh / a rim of a box or cylinder at its hit point.

A scene is plain data (tests/ray_rig.py builds the MJCF from the same data):
  scene = dict(world=[geom ..], bodies=[dict(name, parent (index or -1), pos, quat, free, geoms=[geom ..])], laser=index of the body
               that carries the sites, sites=[(pos, quat) ..], cutoff, meshes={name: dict(vertex=[[x, y, z] ..], face=[[i, j, k] ..], convex)})
  geom  = dict(type, size, pos, quat, alpha, group, mesh)
qpos holds 7 numbers (position, wxyz quaternion) per free body, in the order of `bodies`."""
import numpy as np

GRAZE = 1e-4
_PHI = (np.sqrt(5.0) - 1.0) / 2.0


# ------------------------------------------------------------------------------------------------ poses
def _qmul(a, b):
    aw, av, bw, bv = a[..., :1], a[..., 1:], b[..., :1], b[..., 1:]
    return np.concatenate([aw * bw - np.sum(av * bv, -1, keepdims=True), aw * bv + bw * av + np.cross(av, bv)], -1)


def _unit(q):
    q = np.asarray(q, np.float64)
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def _rotate(q, v):
    """q v q* by two Hamilton products (q a unit quaternion [..., 4], v [..., 3])."""
    v = np.asarray(v, np.float64)
    vq = np.concatenate([np.zeros(v.shape[:-1] + (1,)), v], -1)
    return _qmul(_qmul(q, vq), q * np.array([1.0, -1.0, -1.0, -1.0]))[..., 1:]


def _compose(pp, pq, pos, quat):
    """(parent pose) o (pos, quat): world position and unit quaternion, batched over the leading axis of the parent."""
    quat = _unit(quat)
    return pp + _rotate(pq, np.broadcast_to(np.asarray(pos, np.float64), pp.shape)), _qmul(pq, np.broadcast_to(quat, pq.shape))


def _r32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ implicit functions
def _sdf(kind, size, p):
    if kind == "sphere":
        return np.linalg.norm(p, axis=-1) - size[0]
    if kind == "capsule":
        z = np.clip(p[..., 2], -size[1], size[1])
        return np.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2 + (p[..., 2] - z) ** 2) - size[0]
    if kind == "cylinder":
        dr, dz = np.hypot(p[..., 0], p[..., 1]) - size[0], np.abs(p[..., 2]) - size[1]
        return np.minimum(np.maximum(dr, dz), 0.0) + np.hypot(np.maximum(dr, 0.0), np.maximum(dz, 0.0))
    if kind == "box":
        q = np.abs(p) - np.asarray(size[:3])
        return np.minimum(q.max(-1), 0.0) + np.linalg.norm(np.maximum(q, 0.0), axis=-1)
    if kind == "ellipsoid":
        return np.sum((p / np.asarray(size[:3])) ** 2, -1) - 1.0
    raise ValueError(kind)


def _radius(kind, size):
    return {"sphere": lambda: size[0], "capsule": lambda: size[0] + size[1], "cylinder": lambda: np.hypot(size[0], size[1]),
            "box": lambda: np.linalg.norm(size[:3]), "ellipsoid": lambda: max(size[:3])}[kind]()


def _minimise(f, T):
    """Golden section of a convex f over [0, T] (arrays): (t of the minimum, the minimum), the end t = 0 included."""
    a, b = np.zeros_like(T), T.copy()
    for _ in range(100):
        c, d = b - _PHI * (b - a), a + _PHI * (b - a)
        left = f(c) < f(d)
        a, b = np.where(left, a, c), np.where(left, d, b)
    tm = 0.5 * (a + b)
    fm, f0 = f(tm), f(np.zeros_like(T))
    return np.where(f0 <= fm, 0.0, tm), np.minimum(f0, fm)


def _bisect(f, lo, hi, rising):
    """Root of f in [lo, hi] to 1e-12 where f changes sign: from + to - (rising False) or from - to + (rising True)."""
    lo, hi = lo.copy(), hi.copy()
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        neg = f(mid) <= 0
        up = neg if rising else ~neg       # the half to drop is the one that keeps the sign of its end
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
        if np.max(hi - lo) < 1e-13:
            break
    return 0.5 * (lo + hi)


def _convex_root(f, T):
    """(distance or -1, min of f over t >= 0, t of that minimum) for a convex implicit function with f(T) > 0."""
    tm, fm = _minimise(f, T)
    f0 = f(np.zeros_like(T))
    hit = fm <= 0
    enter = _bisect(f, np.zeros_like(T), tm, False)
    leave = _bisect(f, tm, T, True)
    return np.where(hit, np.where(f0 > 0, enter, leave), -1.0), fm, tm


def ray_convex(kind, size, lp, lv):
    """Rays lp + t lv (unit lv) in the frame of a sphere / capsule / cylinder / box / ellipsoid: (distance or -1, graze in metres)."""
    size = [float(s) for s in size]
    T = np.linalg.norm(lp, axis=-1) + _radius(kind, size) + 1.0
    x, fm, tm = _convex_root(lambda t: _sdf(kind, size, lp + t[:, None] * lv), T)
    graze = np.abs(fm) * (min(size[:3]) if kind == "ellipsoid" else 1.0)
    hitp = np.abs(lp + np.maximum(x, 0)[:, None] * lv)
    if kind == "box":      # the hit point on an edge: two of the three faces within the band
        near = np.sort(np.abs(hitp - np.asarray(size[:3])), -1)[:, 1]
        graze = np.where(x >= 0, np.minimum(graze, near), graze)
    if kind == "cylinder":  # ... on a rim
        near = np.maximum(np.abs(np.hypot(hitp[:, 0], hitp[:, 1]) - size[0]), np.abs(hitp[:, 2] - size[1]))
        graze = np.where(x >= 0, np.minimum(graze, near), graze)
    return x, graze, tm


def ray_plane(size, lp, lv):
    """The plane z = 0 from its front (z > 0), inside the half sizes that are positive."""
    T = np.full(len(lp), 1e5)
    f = lambda t: lp[:, 2] + t * lv[:, 2]
    front = (lp[:, 2] > 0) & (f(T) < 0)
    t = _bisect(f, np.zeros(len(lp)), T, False)
    p = lp + t[:, None] * lv
    inside, edge = np.ones(len(lp), bool), np.full(len(lp), np.inf)
    for k in range(2):
        if size[k] > 0:
            inside &= np.abs(p[:, k]) <= size[k]
            edge = np.minimum(edge, np.abs(np.abs(p[:, k]) - size[k]))
    return np.where(front & inside, t, -1.0), np.where(front, edge, np.inf), np.where(front, t, np.inf)


def _segment_distance(p, a, b):
    ab = b - a
    s = np.clip(np.sum((p - a) * ab, -1) / np.dot(ab, ab), 0.0, 1.0)
    return np.linalg.norm(p - a - s[:, None] * ab, axis=-1)


def _edge_distance(p, verts, faces):
    d = np.full(len(p), np.inf)
    for i, j in {tuple(sorted((f[a], f[(a + 1) % 3]))) for f in faces for a in range(3)}:
        d = np.minimum(d, _segment_distance(p, verts[i], verts[j]))
    return d


def ray_convex_mesh(verts, faces, lp, lv):
    """Half-space clipping over the faces of a closed convex mesh (any winding: the normals are turned away from the centroid)."""
    verts = np.asarray(verts, np.float64)
    cen = verts.mean(0)
    nrm = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm *= np.sign(np.sum(nrm * (verts[faces[:, 0]] - cen), 1))[:, None]
    h = np.sum(nrm * verts[faces[:, 0]], 1)
    s, dv = lp @ nrm.T - h, lv @ nrm.T          # [N, F] height above each face plane, and its rate along the ray
    with np.errstate(divide="ignore", invalid="ignore"):
        tc = -s / dv
    t_in = np.max(np.where(dv < 0, tc, -np.inf), 1)
    t_out = np.min(np.where(dv > 0, tc, np.inf), 1)
    outside_parallel = np.any((dv == 0) & (s > 0), 1)
    hit = (t_in <= t_out) & (t_out >= 0) & ~outside_parallel
    x = np.where(hit, np.where(t_in >= 0, t_in, t_out), -1.0)
    T = np.linalg.norm(lp, axis=-1) + np.linalg.norm(verts, axis=1).max() + 1.0
    tm, fm = _minimise(lambda t: np.max(s + t[:, None] * dv, 1), T)
    graze = np.abs(fm)
    edge = _edge_distance(lp + np.maximum(x, 0)[:, None] * lv, verts, faces)
    return x, np.where(x >= 0, np.minimum(graze, edge), graze), tm


def ray_triangles(verts, faces, lp, lv):
    """Brute force over the triangles of an open mesh, both sides: the plane of each triangle, then three same-side tests."""
    verts = np.asarray(verts, np.float64)
    best, graze, tnear = np.full(len(lp), np.inf), np.full(len(lp), np.inf), np.full(len(lp), np.inf)
    for f in faces:
        a, b, c = verts[f[0]], verts[f[1]], verts[f[2]]
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        rate = lv @ n
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((a - lp) @ n) / rate
        ok = np.isfinite(t) & (t >= 0)
        p = lp + np.where(ok, t, 0.0)[:, None] * lv
        side = [np.cross(v1 - v0, p - v0) @ n for v0, v1 in ((a, b), (b, c), (c, a))]
        inside = ok & (side[0] >= 0) & (side[1] >= 0) & (side[2] >= 0)
        best = np.where(inside & (t < best), t, best)
        edge = np.minimum(np.minimum(_segment_distance(p, a, b), _segment_distance(p, b, c)), _segment_distance(p, c, a))
        graze = np.where(ok, np.minimum(graze, edge), graze)
        tnear = np.where(ok, np.minimum(tnear, t), tnear)
    return np.where(np.isfinite(best), best, -1.0), graze, tnear


def ray_geom(geom, meshes, lp, lv):
    """(distance or -1, graze, t where the ray is nearest to changing its answer) of rays in the geom's frame."""
    if geom["type"] == "plane":
        return ray_plane(geom["size"], lp, lv)
    if geom["type"] == "mesh":
        m = meshes[geom["mesh"]]
        v, f = np.asarray(m["vertex"], np.float64), np.asarray(m["face"], np.int64)
        return ray_convex_mesh(v, f, lp, lv) if m["convex"] else ray_triangles(v, f, lp, lv)
    return ray_convex(geom["type"], geom["size"], lp, lv)


# ------------------------------------------------------------------------------------------------ the scan
def rounded(scene):
    """The scene with every constant rounded to fp32 (body, geom and site frames, sizes, mesh vertices)."""
    g32 = lambda g: dict(g, size=_r32(g["size"]), pos=_r32(g["pos"]), quat=_r32(g["quat"]))
    return dict(scene, world=[g32(g) for g in scene["world"]],
                bodies=[dict(b, pos=_r32(b["pos"]), quat=_r32(b["quat"]), geoms=[g32(g) for g in b["geoms"]]) for b in scene["bodies"]],
                sites=[(_r32(p), _r32(q)) for p, q in scene["sites"]],
                meshes={k: dict(m, vertex=_r32(m["vertex"])) for k, m in scene["meshes"].items()})


def body_poses(scene, qpos):
    """World position [E, 3] and unit quaternion [E, 4] of every body for qpos [E, 7 x free bodies]."""
    qpos = np.asarray(qpos, np.float64)
    E = len(qpos)
    out, adr = [], 0
    wp, wq = np.zeros((E, 3)), np.tile([1.0, 0, 0, 0], (E, 1))
    for b in scene["bodies"]:
        if b["free"]:
            assert b["parent"] < 0
            out.append((qpos[:, adr:adr + 3], _unit(qpos[:, adr + 3:adr + 7])))
            adr += 7
        else:
            pp, pq = (wp, wq) if b["parent"] < 0 else out[b["parent"]]
            out.append(_compose(pp, pq, b["pos"], b["quat"]))
    assert adr == qpos.shape[1]
    return out


def scan(scene, qpos):
    """(range [E, R], graze [E, R]) of the scene's rangefinder rays for qpos [E, nq]."""
    qpos = np.asarray(qpos, np.float64)
    E, R = len(qpos), len(scene["sites"])
    poses = body_poses(scene, qpos)
    wp, wq = np.zeros((E, 3)), np.tile([1.0, 0, 0, 0], (E, 1))
    lpos, lquat = poses[scene["laser"]]
    org, dirs = np.zeros((E, R, 3)), np.zeros((E, R, 3))
    for r, (sp, sq) in enumerate(scene["sites"]):
        p, q = _compose(lpos, lquat, sp, sq)
        org[:, r], dirs[:, r] = p, _rotate(q, np.broadcast_to([0.0, 0.0, 1.0], (E, 3)))
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    found = []
    for bi, geoms in [(-1, scene["world"])] + [(i, b["geoms"]) for i, b in enumerate(scene["bodies"])]:
        if bi == scene["laser"]:
            continue
        bp, bq = (wp, wq) if bi < 0 else poses[bi]
        for g in geoms:
            if g.get("alpha", 1.0) == 0:
                continue
            gp, gq = _compose(bp, bq, g["pos"], g["quat"])
            inv = gq * np.array([1.0, -1.0, -1.0, -1.0])
            rel = org - gp[:, None, :]
            lp = _rotate(np.repeat(inv[:, None, :], R, 1).reshape(-1, 4), rel.reshape(-1, 3))
            lv = _rotate(np.repeat(inv[:, None, :], R, 1).reshape(-1, 4), dirs.reshape(-1, 3))
            found.append(ray_geom(g, scene["meshes"], lp, lv))
    best = np.full(E * R, np.inf)
    for x, _, _ in found:
        best = np.where((x >= 0) & (x < best), x, best)
    graze = np.full(E * R, np.inf)
    for x, gz, tn in found:      # a geom's near miss (or near hit) matters where it is not behind the answer
        graze = np.where(np.where(x >= 0, x, tn) <= best + 1e-3, np.minimum(graze, gz), graze)
    out = np.where(np.isfinite(best), best, -1.0)
    if scene["cutoff"] > 0:
        out = np.where(out > scene["cutoff"], scene["cutoff"], out)
    return out.reshape(E, R), graze.reshape(E, R)


def floor(scene, qpos64):
    """The input-rounding floor: the largest change of the scan when qpos and every constant are rounded to fp32, over the rays
    that graze in neither evaluation and keep their answer's kind (hit, miss, cutoff)."""
    a, ga = scan(scene, qpos64)
    b, gb = scan(rounded(scene), _r32(qpos64))
    keep = (ga >= GRAZE) & (gb >= GRAZE) & ((a < 0) == (b < 0))
    return float(np.max(np.abs(a - b)[keep], initial=0.0))
