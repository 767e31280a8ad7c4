"""A depth-camera image in fp64 numpy, written from the rule alone.  TEST INFRASTRUCTURE: it imports numpy and tests/ray_ref.py, nothing
of the package, of oracle/ or of the compiler, and restates none of their intersection formulas.

The rule (what MuJoCo's renderer draws, read at pixel centres; oracle/smj_oracle.c and csrc/smj_render.hip state the same):
  * pixel (u, v) of a W x H image looks along the camera-frame direction (((u + .5) / W 2 - 1) tan(fovy / 2) W / H,
    (1 - (v + .5) / H 2) tan(fovy / 2), -1): x right, y up, looking down -z.  DEPTH is the parameter along that unnormalised direction,
    i.e. metres along the optical axis;
  * geoms with group <= 2 and alpha != 0 are drawn, those of the camera's own body included;
  * front faces only: of a closed convex shape the entry point, and nothing when the eye is inside it; of a plane its front, within
    its positive half sizes; of a mesh the triangles whose counter-clockwise side faces the eye;
  * a surface point counts only at depth >= znear (a shape whose entry point is nearer contributes nothing in that pixel); the
    nearest such point wins; nothing up to zfar: the raw image reads zfar.  `limited` applies a limit L > 0: nothing found, or any
    value above L, reads 0.

The method is ray_ref's: the entry root of the convex implicit functions by golden section and bisection, half-space clipping for
convex meshes, brute force over the (here one-sided) triangles of an open mesh.  No closed-form quadratic.  A bounding-sphere
prefilter (distance from the centre to the ray's line against the radius plus 1 mm) only spares the root finder rays that pass
clear of a geom by more than ten times the grazing band.

`graze` of a pixel is in metres at the geometry; a pixel grazes when it is below GRAZE.  It is the smallest of: the distance to a
change between hit and miss on a geom that could change the answer; to a mesh edge, a box edge or a cylinder rim at the hit point;
|entry depth - znear|; the eye's distance to a surface; the gap between the two nearest surfaces of different geoms (the geom id
is undecided there); and |depth - zfar| (`limited` adds |depth - L|) less the comparison bound `_bound`.

A scene is ray_ref's, plus cameras = [dict(body (index), pos, quat, fovy (degrees))]."""
import numpy as np

import ray_ref
from ray_ref import GRAZE, _bisect, _compose, _edge_distance, _minimise, _r32, _rotate, _sdf, _segment_distance

_CONJ = np.array([1.0, -1.0, -1.0, -1.0])


def _bound(z):
    """The project's ceiling for a depth comparison: a value this close to a threshold (far plane, limit) may fall on either side."""
    return 1e-4 + 1e-4 * np.abs(z)


def enter_convex(kind, size, lp, lv, tmin):
    """Entry of rays lp + t lv (unit lv) into a sphere / capsule / cylinder / box / ellipsoid from outside, at t >= tmin:
    (t or -1, graze, t where the ray is nearest to the shape)."""
    size = [float(s) for s in size]
    T = np.linalg.norm(lp, axis=-1) + ray_ref._radius(kind, size) + 1.0
    f = lambda t: _sdf(kind, size, lp + t[:, None] * lv)
    tm, fm = _minimise(f, T)
    f0 = f(np.zeros_like(T))
    scale = min(size[:3]) if kind == "ellipsoid" else 1.0
    x = _bisect(f, np.zeros_like(T), tm, False)
    hit = (f0 > 0) & (fm <= 0)
    graze = np.minimum(np.abs(fm), np.abs(f0)) * scale           # hit or miss; the eye on the surface
    graze = np.where(hit, np.minimum(graze, np.abs(x - tmin)), graze)      # the entry on the near plane
    hitp = np.abs(lp + x[:, None] * lv)
    if kind == "box":
        near = np.sort(np.abs(hitp - np.asarray(size[:3])), -1)[:, 1]
        graze = np.where(hit, np.minimum(graze, near), graze)
    if kind == "cylinder":
        near = np.maximum(np.abs(np.hypot(hitp[:, 0], hitp[:, 1]) - size[0]), np.abs(hitp[:, 2] - size[1]))
        graze = np.where(hit, np.minimum(graze, near), graze)
    return np.where(hit & (x >= tmin), x, -1.0), graze, np.where(hit, x, tm)


def enter_plane(size, lp, lv, tmin):
    x, edge, tn = ray_ref.ray_plane(size, lp, lv)
    graze = np.minimum(edge, np.abs(lp[:, 2]))                   # the rim; the eye in the plane
    graze = np.where(x >= 0, np.minimum(graze, np.abs(x - tmin)), graze)
    return np.where(x >= tmin, x, -1.0), graze, tn


def enter_convex_mesh(verts, faces, lp, lv, tmin):
    """Half-space clipping over the faces of a closed convex mesh, from outside."""
    verts = np.asarray(verts, np.float64)
    cen = verts.mean(0)
    nrm = np.cross(verts[faces[:, 1]] - verts[faces[:, 0]], verts[faces[:, 2]] - verts[faces[:, 0]])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm *= np.sign(np.sum(nrm * (verts[faces[:, 0]] - cen), 1))[:, None]
    h = np.sum(nrm * verts[faces[:, 0]], 1)
    s, dv = lp @ nrm.T - h, lv @ nrm.T
    with np.errstate(divide="ignore", invalid="ignore"):
        tc = -s / dv
    t_in = np.max(np.where(dv < 0, tc, -np.inf), 1)
    t_out = np.min(np.where(dv > 0, tc, np.inf), 1)
    f0 = s.max(1)
    hit = (f0 > 0) & (t_in <= t_out) & (t_in >= 0) & ~np.any((dv == 0) & (s > 0), 1)
    T = np.linalg.norm(lp, axis=-1) + np.linalg.norm(verts, axis=1).max() + 1.0
    tm, fm = _minimise(lambda t: np.max(s + t[:, None] * dv, 1), T)
    x = np.where(hit, t_in, 0.0)
    graze = np.minimum(np.abs(fm), np.abs(f0))
    edge = np.minimum(_edge_distance(lp + x[:, None] * lv, verts, faces), np.abs(x - tmin))
    graze = np.where(hit, np.minimum(graze, edge), graze)
    return np.where(hit & (x >= tmin), x, -1.0), graze, np.where(hit, x, tm)


def enter_triangles(verts, faces, lp, lv, tmin):
    """Brute force over the triangles of an open mesh, each from its counter-clockwise side only, at t >= tmin."""
    verts = np.asarray(verts, np.float64)
    best, graze, tnear = np.full(len(lp), np.inf), np.full(len(lp), np.inf), np.full(len(lp), np.inf)
    for f in faces:
        a, b, c = verts[f[0]], verts[f[1]], verts[f[2]]
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        rate = lv @ n
        height = (lp - a) @ n                                    # of the eye above the triangle's plane: positive = its front
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -height / rate
        ok = (height > 0) & (rate < 0) & np.isfinite(t)
        p = lp + np.where(ok, t, 0.0)[:, None] * lv
        side = [np.cross(v1 - v0, p - v0) @ n for v0, v1 in ((a, b), (b, c), (c, a))]
        inside = ok & (side[0] >= 0) & (side[1] >= 0) & (side[2] >= 0)
        edge = np.minimum(np.minimum(_segment_distance(p, a, b), _segment_distance(p, b, c)), _segment_distance(p, c, a))
        edge = np.where(inside, np.minimum(edge, np.abs(t - tmin)), edge)
        edge = np.where(inside, np.minimum(edge, np.abs(height)), edge)       # the eye in the triangle's plane: front or back undecided
        take = inside & (t >= tmin) & (t < best)
        best = np.where(take, t, best)
        graze = np.where(ok, np.minimum(graze, edge), graze)
        tnear = np.where(ok, np.minimum(tnear, t), tnear)
    return np.where(np.isfinite(best), best, -1.0), graze, tnear


def enter_geom(geom, meshes, lp, lv, tmin):
    if geom["type"] == "plane":
        return enter_plane(geom["size"], lp, lv, tmin)
    if geom["type"] == "mesh":
        m = meshes[geom["mesh"]]
        v, f = np.asarray(m["vertex"], np.float64), np.asarray(m["face"], np.int64)
        return (enter_convex_mesh if m["convex"] else enter_triangles)(v, f, lp, lv, tmin)
    return enter_convex(geom["type"], geom["size"], lp, lv, tmin)


def bounding_radius(geom, meshes):
    if geom["type"] == "plane":
        return np.inf
    if geom["type"] == "mesh":
        return float(np.linalg.norm(np.asarray(meshes[geom["mesh"]]["vertex"], np.float64), axis=1).max())
    return float(ray_ref._radius(geom["type"], [float(s) for s in geom["size"]]))


def geoms_of(scene):
    """[(body index or -1, geom)] in the order of the geom-id image: the world's geoms, then every body's."""
    return [(-1, g) for g in scene["world"]] + [(i, g) for i, b in enumerate(scene["bodies"]) for g in b["geoms"]]


def rounded(scene):
    """ray_ref.rounded, and the cameras' frames and fields of view."""
    out = ray_ref.rounded(dict(scene, sites=scene.get("sites", [])))
    out["cameras"] = [dict(c, pos=_r32(c["pos"]), quat=_r32(c["quat"]), fovy=float(np.float32(c["fovy"]))) for c in scene["cameras"]]
    return out


def pixel_rays(width, height, tan_half):
    u, v = np.meshgrid(np.arange(width), np.arange(height))
    return np.stack([((u + 0.5) / width * 2 - 1) * tan_half * width / height, (1 - (v + 0.5) / height * 2) * tan_half, -np.ones(u.shape)], -1).reshape(-1, 3)


def view(scene, qpos, cam, width, height, fovy, znear, zfar, fp32_tan=False):
    """(depth [E, H, W], geom [E, H, W] (index into geoms_of, -1 = nothing up to zfar), graze [E, H, W]) of camera `cam` for
    qpos [E, nq]: the raw image.  fp32_tan: tan(fovy / 2) rounded to fp32, as a caller gets it who holds fovy in fp32 (the
    input-rounding floor)."""
    qpos = np.asarray(qpos, np.float64)
    E, N = len(qpos), width * height
    poses = ray_ref.body_poses(scene, qpos)
    wp, wq = np.zeros((E, 3)), np.tile([1.0, 0, 0, 0], (E, 1))
    c = scene["cameras"][cam]
    tan_half = np.tan(np.radians(fovy) / 2)
    if fp32_tan:
        tan_half = float(_r32(np.tan(_r32(_r32(fovy) * _r32(np.pi / 360)))))
    dc = pixel_rays(width, height, tan_half)
    scale = np.tile(np.linalg.norm(dc, axis=1), E)               # depth = t / scale for the unit direction
    eye, cq = _compose(*poses[c["body"]], c["pos"], c["quat"])
    org = np.repeat(eye, N, 0)
    dirs = _rotate(np.repeat(cq, N, 0), np.tile(dc, (E, 1)))
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    tmin = znear * scale
    found = []
    for k, (bi, g) in enumerate(geoms_of(scene)):
        if g.get("alpha", 1.0) == 0 or g.get("group", 0) > 2:
            continue
        gp, gq = _compose(*((wp, wq) if bi < 0 else poses[bi]), g["pos"], g["quat"])
        rel = org - np.repeat(gp, N, 0)
        rb = bounding_radius(g, scene["meshes"])
        idx = np.arange(E * N)
        if np.isfinite(rb):
            along = np.sum(rel * dirs, -1)
            idx = np.nonzero(np.linalg.norm(rel - along[:, None] * dirs, axis=-1) <= rb + 1e-3)[0]
        if len(idx) == 0:
            continue
        inv = np.repeat(gq * _CONJ, N, 0)[idx]
        x, gz, tn = enter_geom(g, scene["meshes"], _rotate(inv, rel[idx]), _rotate(inv, dirs[idx]), tmin[idx])
        found.append((k, idx, x, gz, tn))
    best, second, who = np.full(E * N, np.inf), np.full(E * N, np.inf), np.full(E * N, -1)
    for k, idx, x, _, _ in found:
        x = np.where(x >= 0, x, np.inf)
        b = best[idx]
        second[idx] = np.where(x < b, b, np.minimum(second[idx], x))
        who[idx] = np.where(x < b, k, who[idx])
        best[idx] = np.minimum(b, x)
    graze = np.where(np.isfinite(second), second - np.where(np.isfinite(best), best, 0.0), np.inf)
    for k, idx, x, gz, tn in found:      # a geom's near miss (or near hit) matters where it is not behind the answer
        graze[idx] = np.where(np.where(x >= 0, x, tn) <= best[idx] + 1e-3, np.minimum(graze[idx], gz), graze[idx])
    depth = best / scale
    graze = np.where(np.isfinite(depth), np.minimum(graze, np.maximum(np.abs(depth - zfar) - _bound(zfar), 0.0)), graze)
    nothing = ~(depth <= zfar)
    return (np.where(nothing, zfar, depth).reshape(E, height, width), np.where(nothing, -1, who).reshape(E, height, width),
            graze.reshape(E, height, width))


def limited(depth, geom, graze, limit, zfar):
    """The image with a limit L > 0 from the raw one: nothing found, or any value above L, reads 0; |depth - L| joins graze."""
    out = np.where((geom < 0) | (depth > limit), 0.0, depth)
    near = np.where(geom >= 0, np.maximum(np.abs(depth - limit) - _bound(limit), 0.0), np.inf)
    return out, np.where(out > 0, geom, -1), np.minimum(graze, near)


def floor(scene, qpos64, cam, width, height, fovy, znear, zfar):
    """The input-rounding floor: the largest change of the raw depth when qpos and every constant (frames, sizes, vertices, the
    field of view and its tangent) are rounded to fp32, over the pixels that graze in neither evaluation and see the same geom."""
    a, ia, ga = view(scene, qpos64, cam, width, height, fovy, znear, zfar)
    b, ib, gb = view(rounded(scene), _r32(qpos64), cam, width, height, fovy, znear, zfar, fp32_tan=True)
    keep = (ga >= GRAZE) & (gb >= GRAZE) & (ia == ib)
    return float(np.max(np.abs(a - b)[keep], initial=0.0))
