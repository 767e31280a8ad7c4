"""numpy reference of smj_scan_to_pose (include/smj_scanmatch.h).  A helper, not a test.  Two parts, as the entry has two:

decide() -- everything after the points have their cells: integers (the sums S, the scores J, the first of the (J descending, i
ascending) order, the status), and the output pose, which is one fused multiply-add and one sum of fp32 values.  It is exact and the
device must equal it bit for bit.

place() -- the cell of every point and rotation, in fp64, with a MARGIN per point and coordinate.  The header lists the fp32
operations:
    p = o + r d                                  (frame_points: the end of the ray in the robot's frame)
    theta_t = theta + angle[t]                   (one fp32 sum: repeated here in fp32, so it adds nothing)
    gx = x + c px - s py,  ix = floor((gx - x0) / cell)     (gy, iy alike; c = cosf(theta_t), s = sinf(theta_t))
The margin is the sum of
  * tests/occupancy_ref.py's margin of the end point in the frame, EPS * (So + |r| Sd) per coordinate (So, Sd: the sums of the
    magnitudes o and d are summed from), carried through the rotation: (|c| mx + |s| my, |s| mx + |c| my);
  * tests/drive_ref.py's terms for the transform and the cell: EPS * (|x| + |px| + |py|) + 2^-22 * |g - x0|.
A point whose box +-m lies in ONE cell (or wholly outside the band of 32 cells round the grid) is SURE: fp32 must give that cell (or
none).  Any other point is UNSURE and has up to four candidates.  A ray that is no return, and every ray of a pose that is not
finite, has no cell, surely.  The comparison means something while unsure points are few: callers assert at most
occupancy_ref.MAX_AMBIGUOUS of an env's points per rotation table."""
from types import SimpleNamespace

import numpy as np

import occupancy_ref
from occupancy_ref import EPS, MAX_AMBIGUOUS  # noqa: F401

NO_CELL = -32768
OK, FEW, OFF = 0, 1, 2
BAND = 32


def frame_points(o, d, So, Sd, ranges, r_min, r_max):
    """One env: rays (o, d, So, Sd [K, 2] as occupancy_ref.ray_geometry gives them in the robot's frame) and ranges [K] (fp32 values)
    -> p [K, 2] (NaN where the ray does not count), margin [K, 2], counts [K] bool."""
    kind, length = occupancy_ref.classify(ranges, float(np.float32(r_min)), float(np.float32(r_max)), 0)
    p = o + length[:, None] * d
    m = EPS * (So + np.abs(length)[:, None] * Sd)
    counts = (kind == occupancy_ref.RETURN) & np.isfinite(p).all(-1)
    return np.where(counts[:, None], p, np.nan), np.where(counts[:, None], m, 0.0), counts


def turned(pose, angles):
    """theta_t [B, T] as the entry forms it: one fp32 sum."""
    return (np.asarray(pose, np.float32)[2][:, None] + np.asarray(angles, np.float32)[None, :]).astype(np.float32)


def place(points, margins, pose, angles, x0, y0, cell, nx, ny):
    """points, margins [B, K, 2] (frame_points per env), pose [3, B] (x, y, theta; fp32 values), angles [T] -> cell [B, T, K, 2] int64
    ((ix, iy) of the fp64 point, NO_CELL twice where it has none), sure [B, T, K] bool, cand [B, T, K, 4, 2] (the cells the point's
    box meets, all of them `cell` where sure), n [B] the counting rays."""
    x0, y0, cell = (float(np.float32(q)) for q in (x0, y0, cell))
    pose = np.asarray(pose, np.float32).astype(np.float64)
    pts, mar = np.asarray(points, np.float64), np.asarray(margins, np.float64)
    B, K = pts.shape[:2]
    counts = np.isfinite(pts).all(-1)                                  # [B, K]
    th = turned(pose, angles).astype(np.float64)[:, :, None]           # [B, T, 1]
    x, y = pose[0][:, None, None], pose[1][:, None, None]
    px, py = np.where(counts, pts[..., 0], 0.0)[:, None, :], np.where(counts, pts[..., 1], 0.0)[:, None, :]
    mx, my = mar[..., 0][:, None, :], mar[..., 1][:, None, :]
    org = np.array([x0, y0])
    lim = np.array([nx, ny])
    with np.errstate(invalid="ignore"):
        c, s = np.cos(th), np.sin(th)
        g = np.stack((x + c * px - s * py, y + s * px + c * py), -1)      # [B, T, K, 2]
        S = np.stack((np.abs(x) + np.abs(px) + np.abs(py), np.abs(y) + np.abs(px) + np.abs(py)), -1) + 0 * g
        carried = np.stack((np.abs(c) * mx + np.abs(s) * my, np.abs(s) * mx + np.abs(c) * my), -1)
        m = EPS * S + 2.0 ** -22 * np.abs(g - org) + carried
        finite = np.isfinite(g).all(-1) & np.isfinite(pose).all(0)[:, None, None] & counts[:, None, :]
        gz, mz = np.where(finite[..., None], g, 0.0), np.where(finite[..., None], m, 0.0)
        lo = np.floor((gz - mz - org) / cell)
        hi = np.floor((gz + mz - org) / cell)
        mid = np.floor((gz - org) / cell)
    assert (hi - lo <= 1).all(), "a margin wider than a cell: not a case of this reference"

    def cells(f):
        placed = ((f >= -BAND) & (f < lim + BAND)).all(-1) & finite
        return np.where(placed[..., None], np.where(placed[..., None], f, 0).astype(np.int64), NO_CELL)

    cand = np.stack([cells(np.stack((a[..., 0], b[..., 1]), -1)) for a in (lo, hi) for b in (lo, hi)], -2)
    sure = (cand == cand[..., :1, :]).all((-1, -2))
    return SimpleNamespace(cell=cells(mid), sure=sure, cand=cand, margin=m, n=counts.sum(1), B=B, K=K, T=th.shape[1])


def unsure_share(pl):
    """Per env the share of unsure (rotation, ray) pairs."""
    return (~pl.sure).reshape(pl.B, -1).mean(1)


def check_cells(got, pl):
    """The comparison rule of the float stage: every sure point equals the reference cell, every unsure one is among its candidates.
    Returns the list of violations (b, t, k, got, candidates)."""
    got = np.asarray(got).astype(np.int64).reshape(pl.cell.shape)
    ok = np.where(pl.sure, (got == pl.cell).all(-1), (got[..., None, :] == pl.cand).all(-1).any(-1))
    return [(int(b), int(t), int(k), got[b, t, k].tolist(), pl.cand[b, t, k].tolist()) for b, t, k in np.argwhere(~ok)]


def index(t, dy, dx, wx, wy):
    return (t * (2 * wy + 1) + (dy + wy)) * (2 * wx + 1) + (dx + wx)


def unindex(i, wx, wy):
    """i -> (t, dy, dx)."""
    WX, WY = 2 * wx + 1, 2 * wy + 1
    return i // (WX * WY), (i // WX) % WY - wy, i % WX - wx


def decide(cells, field, pose, angles, cell, n, *, wx, wy, bias=None, shift_weight=0, min_points=30):
    """cells [B, T, K, 2] ((ix, iy), NO_CELL twice for none), field uint8 [B, ny, nx], pose fp32 [3, B], angles fp32 [T], n [B] the
    counting rays.  Returns score int32 [B, T, 2 wy + 1, 2 wx + 1], best int32 [B, 4] (i, J, n, status) and pose fp32 [3, B].
    The output pose: dx cell is exact in fp64 (6 bits by 24), and its sum with x is exact there too while the two exponents lie
    within 20 of each other (asserted), so rounding that sum to fp32 rounds once, like the fused multiply-add."""
    cells = np.asarray(cells).astype(np.int64)
    B, T, K, _ = cells.shape
    field = np.asarray(field)
    assert field.dtype == np.uint8 and field.shape[0] == B
    ny, nx = field.shape[1:]
    flat = field.reshape(B, -1).astype(np.int64)
    pose = np.asarray(pose, np.float32)
    angles = np.asarray(angles, np.float32)
    b = np.zeros(T, np.int64) if bias is None else np.clip(np.asarray(bias).astype(np.int64), 0, 1 << 20)
    ix, iy = cells[..., 0], cells[..., 1]
    score = np.zeros((B, T, 2 * wy + 1, 2 * wx + 1), np.int64)
    for dy in range(-wy, wy + 1):
        for dx in range(-wx, wx + 1):
            sx, sy = ix + dx, iy + dy
            on = (sx >= 0) & (sx < nx) & (sy >= 0) & (sy < ny)
            v = np.take_along_axis(flat, np.where(on, sy * nx + sx, 0).reshape(B, -1), 1).reshape(B, T, K)
            score[:, :, dy + wy, dx + wx] = np.where(on, v, 0).sum(-1) - b[None, :] - shift_weight * (dx * dx + dy * dy)
    assert score.min() > -(1 << 22) and score.max() < 1 << 18
    first = score.reshape(B, -1).argmax(1)      # numpy's argmax returns the first of equal maxima: the smallest i
    J = score.reshape(B, -1)[np.arange(B), first]
    n = np.asarray(n).astype(np.int64)
    status = np.where(~np.isfinite(pose).all(0), OFF, np.where(n < min_points, FEW, OK))
    ok = status == OK
    t, dy, dx = unindex(first, wx, wy)
    c64 = float(np.float32(cell))
    out = pose.copy()
    theta_t = turned(pose, angles)[np.arange(B), t]
    for e in np.nonzero(ok)[0]:
        for row, shift in ((0, dx[e]), (1, dy[e])):
            prod, prior = float(shift) * c64, float(pose[row, e])
            assert prod == 0 or prior == 0 or abs(np.frexp(prod)[1] - np.frexp(prior)[1]) <= 20, "the fp64 sum may round: not a case of this reference"
            out[row, e] = np.float32(prod + prior)
        out[2, e] = theta_t[e]
    best = np.stack((np.where(ok, first, -1), np.where(ok, J, 0), n, status), 1).astype(np.int32)
    return SimpleNamespace(score=score.astype(np.int32), best=best, pose=out, winner=first, status=status.astype(np.int32))


# ---- the synthetic room of the recovery tests: walls and two boxes, seen by rays cast in fp64
WALLS = (-2.31, 2.13, -1.72, 1.88)                                      # xl, xh, yl, yh
BOXES = ((0.62, 1.13, 0.41, 0.79), (-1.52, -1.21, -1.03, -0.18))
ROOM_GRID = SimpleNamespace(nx=128, ny=128, cell=0.05, origin=(-3.2, -3.2))
ROOM_POSES = np.array([(0.0, 0.0, 0.0), (-0.3, 0.2, 0.5), (-0.5, -0.3, -0.7)])   # the poses the map is made from
ROOM_EXTRA_POSE = np.array((0.4, -0.6, 2.0))                                     # a pose that is not in the map
ROOM_OFFSETS = ((3, -2, 4), (-7, 5, -6), (0, 0, 0), (10, -10, 10))                # priors off by (x, y, theta) lattice steps
ROOM_STEP = np.deg2rad(0.5)
ROOM_WINDOW = 10


def _segments():
    out = []
    for xl, xh, yl, yh in (WALLS,) + BOXES:
        out += [((xl, yl), (xh, yl)), ((xh, yl), (xh, yh)), ((xh, yh), (xl, yh)), ((xl, yh), (xl, yl))]
    return np.array(out)                                                # [12, 2, 2]


def cast(origin, direction):
    """Rays origin + t direction ([K, 2] each) against the room: the smallest t > 0 per ray, inf where nothing is hit."""
    seg = _segments()
    a, e = seg[:, 0][None], (seg[:, 1] - seg[:, 0])[None]             # [1, 12, 2]
    o, d = np.asarray(origin, np.float64)[:, None], np.asarray(direction, np.float64)[:, None]
    den = d[..., 0] * e[..., 1] - d[..., 1] * e[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((a[..., 0] - o[..., 0]) * e[..., 1] - (a[..., 1] - o[..., 1]) * e[..., 0]) / den
        u = ((a[..., 0] - o[..., 0]) * d[..., 1] - (a[..., 1] - o[..., 1]) * d[..., 0]) / den
    hit = (den != 0) & (t > 0) & (u >= 0) & (u <= 1)
    return np.where(hit, t, np.inf).min(1)


def room_scan(pose, o, d):
    """The ranges [K] (fp64) a robot at pose (x, y, theta) measures along the rays (o, d [K, 2]) of its own frame."""
    x, y, th = (float(q) for q in pose)
    c, s = np.cos(th), np.sin(th)
    R = np.array([[c, -s], [s, c]])
    return cast(np.array([x, y]) + o @ R.T, d @ R.T)


def unit_rays(K=360):
    """A lidar at the robot's origin: K unit directions, as fp32 values; (o, d, So, Sd) of occupancy_ref.ray_geometry."""
    a = 2 * np.pi * np.arange(K) / K
    d = np.stack((np.cos(a), np.sin(a)), 1).astype(np.float32).astype(np.float64)
    return np.zeros((K, 2)), d, np.zeros((K, 2)), np.abs(d)


def hit_cells(poses, scans, o, d, grid, r_min, r_max):
    """bool [ny, nx]: the cells the returns of the scans end in, each scan laid out from its own pose (fp64)."""
    occ = np.zeros((grid.ny, grid.nx), bool)
    for pose, r in zip(poses, scans):
        keep = (r >= r_min) & (r <= r_max)
        p = o[keep] + r[keep, None] * d[keep]
        c, s = np.cos(pose[2]), np.sin(pose[2])
        g = np.stack((pose[0] + c * p[:, 0] - s * p[:, 1], pose[1] + s * p[:, 0] + c * p[:, 1]), 1)
        ij = np.floor((g - np.array(grid.origin)) / grid.cell).astype(np.int64)
        ok = (ij[:, 0] >= 0) & (ij[:, 0] < grid.nx) & (ij[:, 1] >= 0) & (ij[:, 1] < grid.ny)
        occ[ij[ok, 1], ij[ok, 0]] = True
    return occ


def dist2_of(occ):
    """int32 [ny, nx]: the squared distance in cells to the nearest True cell, brute force; 1 << 30 on a grid without one."""
    ny, nx = occ.shape
    oy, ox = np.nonzero(occ)
    if len(oy) == 0:
        return np.full((ny, nx), 1 << 30, np.int32)
    yy, xx = np.mgrid[0:ny, 0:nx]
    out = np.full((ny, nx), 1 << 30, np.int64)
    for k in range(0, len(oy), 256):
        d2 = (yy[..., None] - oy[k:k + 256]) ** 2 + (xx[..., None] - ox[k:k + 256]) ** 2
        out = np.minimum(out, d2.min(-1))
    return out.astype(np.int32)


def spoil(ranges, r_min, r_max, seed):
    """A copy of ranges [K, ...] (fp32) with one ray in eleven replaced by what a scan may also hold: NaN, -1 (nothing hit), a range
    below r_min, one above r_max, +inf."""
    out = np.array(ranges, np.float32)
    rng = np.random.default_rng(seed)
    bad = np.array([np.nan, -1.0, 0.5 * r_min, 1.5 * r_max, np.inf], np.float32)
    flat = out.reshape(out.shape[0], -1)
    for col in range(flat.shape[1]):
        rows = np.arange(int(rng.integers(0, 11)), flat.shape[0], 11)
        flat[rows, col] = bad[rng.integers(0, len(bad), len(rows))]
    return flat.reshape(out.shape)


# The float stage of tests/test_gpu_scanmatch.py: its grids, its rotation table and the priors it lays over them (off the truth the
# scans were cast from by a few cells and degrees); tests/test_scanmatch_ref.py asserts the cap on unsure points for these with the
# rays of the model's lidar in the frame of their own body.
FLOAT_STAGE = SimpleNamespace(grids=((128, 96, (-3.187, -2.379)), (37, 29, (-0.913, -0.707))), cell=0.05, limits=(0.2, 5.0),
                              angles=np.array([0.0, -0.021, 0.021, -0.35, 0.35], np.float32),
                              truth=ROOM_POSES,
                              prior=np.array([[0.1337, -0.1411, 0.0532], [-0.2287, 0.2532, 0.4561], [-0.469, -0.38, -0.69]], np.float32))


def float_stage_inputs(geoms, seed=5):
    """geoms: per env (o, d, So, Sd) of the rays in the robot's frame.  Returns the spoiled fp32 scan [K, B] cast in the room from
    FLOAT_STAGE.truth, and per env the points, margins and counting flags of frame_points."""
    fs = FLOAT_STAGE
    scan = np.stack([room_scan(fs.truth[e], g[0], g[1]) for e, g in enumerate(geoms)], 1).astype(np.float32)
    scan = spoil(scan, *fs.limits, seed)
    per = [frame_points(*g, scan[:, e].astype(np.float64), *fs.limits) for e, g in enumerate(geoms)]
    return scan, np.stack([p[0] for p in per]), np.stack([p[1] for p in per])
