"""fp64 numpy reference of smj_lidar_to_occupancy (include/smj_occupancy.h).  A helper, not a test.

The classification of a range is a float compare on the stored value and the line between two cells is integer arithmetic: both are
exact and the reference repeats them as they stand.  What is not exact is the cell of the ray's two ends: a cell index is a floor,
so a point within rounding distance of a cell edge may legitimately land on either side in fp32.  For the origin and for the end
point of every ray the reference takes, per coordinate, the margin
    m = EPS * S + 2^-22 * (|x - x0| + |y - y0|)
(S: the sum of the magnitudes of the terms the coordinate is summed from, EPS = 32 * 2^-24 the project's bound on such a sum; the
second term covers the rounding of x - x0, of inv_cell = 1 / cell and of their product).  A ray whose two boxes +-m each lie in ONE
cell is sure and its line is exact; any other ray is ambiguous, with the line of every (start cell, end cell) combination as a
candidate.  Per cell and layer: n_lo counts the sure rays, n_hi adds one for every ambiguous ray that has a candidate line there.
The comparison rule (check_grid), for EVERY cell and both layers: n_lo <= count <= n_hi.  It means something while ambiguous rays
are few: callers assert at most MAX_AMBIGUOUS (2 %) of an env's rays, and since all rays share one origin they choose the grid's
origin so that the laser itself is off every edge (choose_origin)."""
from types import SimpleNamespace

import numpy as np

EPS = 32 * 2.0 ** -24
MAX_AMBIGUOUS = 0.02
DROP, RETURN, CLEAR = 0, 1, 2


def classify(r, r_min, r_max, no_return_clears):
    """ranges [...] -> (kind [...], length [...]): the table of include/smj_occupancy.h."""
    r = np.asarray(r, np.float64)
    kind = np.full(r.shape, DROP, np.int64)
    length = np.zeros(r.shape)
    with np.errstate(invalid="ignore"):
        ret = (r >= r_min) & (r <= r_max)
        none = ~np.isnan(r) & ~ret & ((r < 0) | (r > r_max))
    kind[ret] = RETURN
    length[ret] = r[ret]
    if no_return_clears:
        kind[none] = CLEAR
        length[none] = r_max
    return kind, length


def line_cells(ax, ay, bx, by):
    """The closed-form Bresenham line of include/smj_occupancy.h: the cells i = 0 .. n as two int64 arrays (xs, ys)."""
    dx, dy = bx - ax, by - ay
    n = max(abs(dx), abs(dy))
    if n == 0:
        return np.array([ax], np.int64), np.array([ay], np.int64)
    i = np.arange(n + 1, dtype=np.int64)
    sx, sy = (-1 if dx < 0 else 1), (-1 if dy < 0 else 1)
    if abs(dx) >= abs(dy):
        return ax + i * sx, ay + sy * ((2 * i * abs(dy) + n) // (2 * n))
    return ax + sx * ((2 * i * abs(dx) + n) // (2 * n)), ay + i * sy


def bresenham(ax, ay, bx, by):
    """The same line long-hand: a running error term, one step of the major axis at a time (the minor coordinate moves when the
    accumulated error 2 i d_min + n reaches the next multiple of 2 n).  List of (x, y)."""
    dx, dy = abs(bx - ax), abs(by - ay)
    sx, sy = (-1 if bx < ax else 1), (-1 if by < ay else 1)
    x, y, out = ax, ay, [(ax, ay)]
    if dx >= dy:
        n, err = dx, dx
        for _ in range(n):
            x += sx
            err += 2 * dy
            if err >= 2 * n:
                err -= 2 * n
                y += sy
            out.append((x, y))
    else:
        n, err = dy, dy
        for _ in range(n):
            y += sy
            err += 2 * dx
            if err >= 2 * n:
                err -= 2 * n
                x += sx
            out.append((x, y))
    return out


def ray_geometry(bp, bm, site_pos, lz, fp=None, fm=None):
    """Origins and directions of the rays of ONE env in fp64, with the scale S of every coordinate.
    bp [3], bm [3, 3]: pose of the sites' body (or [K, 3], [K, 3, 3] per ray); site_pos [K, 3]; lz [K, 3] the sites' +Z columns;
    fp, fm: pose of the frame's body, None for the world.  Returns o, d, So, Sd, each [K, 2]."""
    site_pos, lz = np.asarray(site_pos, np.float64), np.asarray(lz, np.float64)
    K = site_pos.shape[0]
    bp = np.broadcast_to(np.asarray(bp, np.float64), (K, 3))
    bm = np.broadcast_to(np.asarray(bm, np.float64), (K, 3, 3))
    o = bp + np.einsum("kij,kj->ki", bm, site_pos)
    So = np.abs(bp) + np.einsum("kij,kj->ki", np.abs(bm), np.abs(site_pos))
    d = np.einsum("kij,kj->ki", bm, lz)
    Sd = np.einsum("kij,kj->ki", np.abs(bm), np.abs(lz))
    if fm is not None:
        fp, fm = np.asarray(fp, np.float64), np.asarray(fm, np.float64)
        o, So = (o - fp) @ fm, (So + np.abs(fp)) @ np.abs(fm)       # o_F = fm' (o - fp)
        d, Sd = d @ fm, Sd @ np.abs(fm)
    return o[:, :2], d[:, :2], So[:, :2], Sd[:, :2]


def _cell_range(p, S, x0, y0, cell):
    """point [2] with scales [2] -> ((ixl, ixh), (iyl, iyh)): the cells its box +-m meets."""
    spread = 2.0 ** -22 * (abs(p[0] - x0) + abs(p[1] - y0))
    out = []
    for c, org in ((0, x0), (1, y0)):
        m = EPS * S[c] + spread
        out.append((int(np.floor((p[c] - m - org) / cell)), int(np.floor((p[c] + m - org) / cell))))
    return out


def origin_margin_cells(o, So, x0, y0, cell):
    """Distance of the origins [K, 2] to the nearest cell edge minus their margin, in metres: > 0 means every laser origin is sure."""
    worst = np.inf
    for k in range(o.shape[0]):
        spread = 2.0 ** -22 * (abs(o[k, 0] - x0) + abs(o[k, 1] - y0))
        for c, org in ((0, x0), (1, y0)):
            f = (o[k, c] - org) / cell
            worst = min(worst, min(f - np.floor(f), np.ceil(f) - f) * cell - (EPS * So[k, c] + spread))
    return worst


def bounds(o, d, So, Sd, ranges, x0, y0, cell, nx, ny, r_min, r_max, no_return_clears):
    """One env: rays (o, d, So, Sd as ray_geometry gives them) and ranges [K] -> per-cell bounds of both layers, [ny, nx] each."""
    kind, length = classify(ranges, r_min, r_max, no_return_clears)
    lo = {"hit": np.zeros((ny, nx), np.int64), "miss": np.zeros((ny, nx), np.int64)}
    hi = {"hit": np.zeros((ny, nx), np.int64), "miss": np.zeros((ny, nx), np.int64)}
    sure = amb = 0

    def layers(k, ax, ay, bx, by):
        xs, ys = line_cells(ax, ay, bx, by)
        inside = (xs >= 0) & (xs < nx) & (ys >= 0) & (ys < ny)
        last = np.zeros(len(xs), bool)
        last[-1] = kind[k] == RETURN
        return (ys[inside & last], xs[inside & last]), (ys[inside & ~last], xs[inside & ~last])

    for k in np.nonzero(kind != DROP)[0]:
        e = o[k] + length[k] * d[k]
        Se = So[k] + abs(length[k]) * Sd[k]
        (axl, axh), (ayl, ayh) = _cell_range(o[k], So[k], x0, y0, cell)
        (bxl, bxh), (byl, byh) = _cell_range(e, Se, x0, y0, cell)
        assert max(abs(axl), abs(axh), abs(ayl), abs(ayh)) < 2 ** 20 - 1, "origin near the +-2^20 guard: not a case of this reference"
        if axl == axh and ayl == ayh and bxl == bxh and byl == byh:
            sure += 1
            h, m = layers(k, axl, ayl, bxl, byl)
            lo["hit"][h] += 1; hi["hit"][h] += 1
            lo["miss"][m] += 1; hi["miss"][m] += 1
            continue
        amb += 1
        cand = {"hit": np.zeros((ny, nx), bool), "miss": np.zeros((ny, nx), bool)}
        for ax in range(axl, axh + 1):
            for ay in range(ayl, ayh + 1):
                for bx in range(bxl, bxh + 1):
                    for by in range(byl, byh + 1):
                        h, m = layers(k, ax, ay, bx, by)
                        cand["hit"][h] = True
                        cand["miss"][m] = True
        hi["hit"] += cand["hit"]
        hi["miss"] += cand["miss"]
    return SimpleNamespace(hit_lo=lo["hit"], hit_hi=hi["hit"], miss_lo=lo["miss"], miss_hi=hi["miss"], rays=len(kind), sure=sure, ambiguous=amb,
                           returns=int((kind == RETURN).sum()), clears=int((kind == CLEAR).sum()), dropped=int((kind == DROP).sum()))


def merge(a, b):
    """Bounds of the grid accumulated from two scans."""
    return SimpleNamespace(hit_lo=a.hit_lo + b.hit_lo, hit_hi=a.hit_hi + b.hit_hi, miss_lo=a.miss_lo + b.miss_lo, miss_hi=a.miss_hi + b.miss_hi,
                           rays=a.rays + b.rays, sure=a.sure + b.sure, ambiguous=a.ambiguous + b.ambiguous, returns=a.returns + b.returns,
                           clears=a.clears + b.clears, dropped=a.dropped + b.dropped)


def check_grid(hit, miss, bd):
    """The comparison rule over every cell of one env; returns the list of violations (empty: the grid is inside the bounds)."""
    bad = []
    for name, got, lo, hi in (("hit", np.asarray(hit), bd.hit_lo, bd.hit_hi), ("miss", np.asarray(miss), bd.miss_lo, bd.miss_hi)):
        assert got.shape == lo.shape
        for iy, ix in zip(*np.nonzero((got < lo) | (got > hi))):
            bad.append((name, int(iy), int(ix), int(got[iy, ix]), int(lo[iy, ix]), int(hi[iy, ix])))
    return bad


def ambiguous_share(bd):
    return bd.ambiguous / max(bd.rays, 1)


def choose_origin(candidates, envs, cell, nx, ny, r_min, r_max, no_return_clears):
    """The first (x0, y0) of `candidates` for which, in every env of `envs` (tuples (o, d, So, Sd, ranges)), every laser origin is
    off the cell edges by more than its margin and the ambiguous rays stay within MAX_AMBIGUOUS; None if there is none.
    Returns ((x0, y0), [bounds per env])."""
    for x0, y0 in candidates:
        x0, y0 = float(np.float32(x0)), float(np.float32(y0))
        if any(origin_margin_cells(o, So, x0, y0, cell) <= 0 for o, _, So, _, _ in envs):
            continue
        bds = [bounds(o, d, So, Sd, r, x0, y0, cell, nx, ny, r_min, r_max, no_return_clears) for o, d, So, Sd, r in envs]
        if all(ambiguous_share(bd) <= MAX_AMBIGUOUS for bd in bds):
            return (x0, y0), bds
    return None


def synthetic_room(K=360, seed=None):
    """A rectangle of walls (x in [-2.3, 3.1], y in [-1.7, 2.4]) around a laser at (0.31, -0.22), yawed 0.4 rad, on a body yawed
    0.25 rad at (0.11, -0.07): K rays in the laser's xy plane.  Returns bp, bm, site_pos [K, 3], lz [K, 3], ranges fp32 [K] (exact
    distances to the walls rounded to fp32) and the walls (xl, xh, yl, yh).  All inputs are fp32 values held in fp64."""
    def rz(a):
        c, s = np.cos(a), np.sin(a)
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])

    f = lambda v: np.asarray(v, np.float64).astype(np.float32).astype(np.float64)
    bm, bp = f(rz(0.25)), f([0.11, -0.07, 0.1])
    sp = f(np.tile([0.2, -0.15, 0.07], (K, 1)))
    ang = 0.15 + 2 * np.pi * np.arange(K) / K
    lz = f(np.stack([np.cos(ang), np.sin(ang), np.zeros(K)], 1))
    walls = (-2.3, 3.1, -1.7, 2.4)
    o, d, _, _ = ray_geometry(bp, bm, sp, lz)
    t = np.full(K, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        for c, plane in ((0, walls[0]), (0, walls[1]), (1, walls[2]), (1, walls[3])):
            tt = (plane - o[:, c]) / d[:, c]
            t = np.where((tt > 0) & (tt < t), tt, t)
    return bp, bm, sp, lz, t.astype(np.float32), walls
