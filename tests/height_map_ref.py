"""fp64 numpy reference of smj_depth_to_heightmap (include/smj_heightmap.h), built on tests/point_cloud_ref.py.  A helper, not a test.

A cell index is a floor: a point within rounding distance of a cell edge (or of the band's limits) may legitimately land on either
side in fp32.  So the reference does not return one map but bounds.  For every valid point it takes the per-component margin
    m = EPS * S + 2^-22 * (|x - x0| + |y - y0|)
(EPS * S: the derived bound of tests/test_gpu_point_cloud.py on the point itself; the second term covers the rounding of x - x0, of
inv_cell = 1 / cell and of their product: three roundings of 2^-24 relative).  A point whose box +-m lies in ONE cell and inside the
z band is sure; one whose box lies wholly outside the grid or the band is surely dropped; any other is ambiguous, with every cell
its box meets as a candidate.  Per cell: n_lo (sure points), n_hi (n_lo + ambiguous candidates), z_lo (max z of the sure points,
-inf without any), z_hi (max over sure and ambiguous candidates), m_z (largest margin among the cell's candidates).
The comparison rule (check_map), for EVERY cell: n_lo <= count <= n_hi; height is NaN iff count == 0; a finite height lies in
[z_lo - m_z, z_hi + m_z].  The share of ambiguous points must stay small for this to mean anything: callers assert <= 1 %."""
import math
from types import SimpleNamespace

import numpy as np

EPS = 32 * 2.0 ** -24
MAX_AMBIGUOUS = 0.01


def synthetic_scene(W, H, fovy=58.0):
    """A floor at z = 0 and two walls (x = 2.1, y = 1.4) seen from a pitched, yawed camera 1.3 m up; the base frame is yawed 0.37 rad.
    Returns (depth fp32 [H, W], cam_xpos, cam_xmat, body_xpos, body_xmat): inputs of point_cloud_ref.deproject."""
    from point_cloud_ref import pixel_dirs

    def rot(axis, a):
        c, s = math.cos(a), math.sin(a)
        return np.array({"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis], np.float64)

    # MuJoCo camera: looks down -z, y up.  Start looking along +x of the world with z up, pitch 0.75 rad down, yaw 0.45
    look = np.array([[0, 0, -1], [-1, 0, 0], [0, 1, 0]], np.float64)   # columns: camera x, y, z axes in the world
    cm = (rot("z", 0.45) @ look @ rot("x", -0.75)).astype(np.float32).astype(np.float64)
    cp = np.array([0.03, -0.02, 1.3], np.float32).astype(np.float64)
    xn, yn = pixel_dirs(W, H, fovy)
    dirs = np.einsum("ij,hwj->hwi", cm, np.stack([xn, yn, -np.ones_like(xn)], -1))
    t = np.full(xn.shape, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for axis, plane in ((2, 0.0), (0, 2.1), (1, 1.4)):
            tt = (plane - cp[axis]) / dirs[..., axis]
            t = np.where((tt > 0) & (tt < t), tt, t)
    depth = np.where(np.isfinite(t) & (t < 30), t, 0.0).astype(np.float32)
    bm = rot("z", 0.37).astype(np.float32).astype(np.float64)
    bp = np.array([0.11, -0.07, 0.0], np.float32).astype(np.float64)
    return depth, cp, cm, bp, bm


def bounds(pts, S, x0, y0, cell, nx, ny, z_lo, z_hi):
    """pts [..., 3] fp64 of ONE env (NaN rows: invalid), S [...] the scale of each point -> the per-cell bounds, [ny, nx] each."""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    S = np.asarray(S, np.float64).reshape(-1)
    ok = ~np.isnan(pts).any(1)
    p, S = pts[ok], S[ok]
    m = EPS * S + 2.0 ** -22 * (np.abs(p[:, 0] - x0) + np.abs(p[:, 1] - y0))
    ixl, ixh = np.floor((p[:, 0] - m - x0) / cell), np.floor((p[:, 0] + m - x0) / cell)
    iyl, iyh = np.floor((p[:, 1] - m - y0) / cell), np.floor((p[:, 1] + m - y0) / cell)
    z = p[:, 2]
    z_in = (z - m >= z_lo) & (z + m <= z_hi)
    z_out = (z + m < z_lo) | (z - m > z_hi)
    grid_out = (ixh < 0) | (ixl >= nx) | (iyh < 0) | (iyl >= ny)
    grid_in = (ixl >= 0) & (ixh < nx) & (iyl >= 0) & (iyh < ny)
    sure = (ixl == ixh) & (iyl == iyh) & grid_in & z_in
    dropped = grid_out | z_out
    amb = ~sure & ~dropped
    n_lo = np.zeros((ny, nx), np.int64)
    zl = np.full((ny, nx), -np.inf)
    mz = np.zeros((ny, nx))
    si, sj = iyl[sure].astype(np.int64), ixl[sure].astype(np.int64)
    np.add.at(n_lo, (si, sj), 1)
    np.maximum.at(zl, (si, sj), z[sure])
    np.maximum.at(mz, (si, sj), m[sure])
    n_hi, zh = n_lo.copy(), zl.copy()
    for k in np.nonzero(amb)[0]:
        for iy in range(max(int(iyl[k]), 0), min(int(iyh[k]), ny - 1) + 1):
            for ix in range(max(int(ixl[k]), 0), min(int(ixh[k]), nx - 1) + 1):
                n_hi[iy, ix] += 1
                zh[iy, ix] = max(zh[iy, ix], z[k])
                mz[iy, ix] = max(mz[iy, ix], m[k])
    return SimpleNamespace(n_lo=n_lo, n_hi=n_hi, z_lo=zl, z_hi=zh, m_z=mz, valid=int(ok.sum()), ambiguous=int(amb.sum()),
                           sure=int(sure.sum()))


def merge(a, b):
    """Bounds of the map fused from two sets of points (two cameras, accumulate = 1)."""
    return SimpleNamespace(n_lo=a.n_lo + b.n_lo, n_hi=a.n_hi + b.n_hi, z_lo=np.maximum(a.z_lo, b.z_lo), z_hi=np.maximum(a.z_hi, b.z_hi),
                           m_z=np.maximum(a.m_z, b.m_z), valid=a.valid + b.valid, ambiguous=a.ambiguous + b.ambiguous, sure=a.sure + b.sure)


def check_map(height, count, bd):
    """The comparison rule over every cell of one env; returns the list of violations (empty: the map is inside the bounds)."""
    height, count = np.asarray(height), np.asarray(count)
    bad = []
    assert height.shape == count.shape == bd.n_lo.shape
    nan = np.isnan(height)
    h = np.where(nan, 0.0, height.astype(np.float64))
    for name, mask in (("count below n_lo", count < bd.n_lo), ("count above n_hi", count > bd.n_hi), ("NaN height with count > 0", nan & (count != 0)),
                       ("finite height with count 0", ~nan & (count == 0)), ("height below z_lo - m_z", ~nan & (h < bd.z_lo - bd.m_z)),
                       ("height above z_hi + m_z", ~nan & (h > bd.z_hi + bd.m_z)), ("height not finite", np.isinf(height))):
        for iy, ix in zip(*np.nonzero(mask)):
            bad.append((name, int(iy), int(ix), float(height[iy, ix]), int(count[iy, ix]), int(bd.n_lo[iy, ix]), int(bd.n_hi[iy, ix]),
                        float(bd.z_lo[iy, ix]), float(bd.z_hi[iy, ix])))
    return bad


def ambiguous_share(bd):
    return bd.ambiguous / max(bd.valid, 1)
