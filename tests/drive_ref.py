"""numpy reference of smj_navigation_to_velocity (include/smj_drive.h).  A helper, not a test.  Two parts, as the entry has two:

decide() -- everything after the points have their cells: integers, and the two fp32 compares of the dynamic window, which need no
rounding.  It is exact and the device must equal it bit for bit.

place() -- the cell of every point, in fp64, with a MARGIN per point and coordinate.  The header lists the fp32 operations:
    wx = x + c px - s py,   ix = floor((wx - x0) / cell)        (wy, iy alike; c = cosf(theta), s = sinf(theta))
The inputs are fp32 values, held here in fp64, so the fp64 result w is exact to ~1e-16.  What fp32 adds, per coordinate:
  * c and s: the accurate sincosf is within 2 ulp of a value <= 1, i.e. 2^-22 absolute, times |px| + |py|;
  * two products and two sums, each rounded once (or fused): at most 2^-24 of the magnitude at hand, which never exceeds
    S = |x| + |px| + |py|; in all below 7 * 2^-24 * S, taken as EPS * S with EPS = 32 * 2^-24, the project's bound on such sums
    (tests/occupancy_ref.py);
  * d = wx - x0 rounds once (2^-24 |d|) and the quotient d / cell is within 2.5 ulp (the library's fp32 division): together below
    2^-22 |d| relative, which moves the point by 2^-22 |d| metres at most.
So the margin is  m = EPS * S + 2^-22 * |w - x0|.  A point whose box +-m lies in ONE cell is SURE: fp32 must give that cell.  Any
other point is UNSURE and has up to four candidate cells (those its box meets; a cell off the grid counts as -1, outside).  A pose
that is not finite puts every point outside, surely.  The comparison means something while unsure points are few: callers assert at
most occupancy_ref.MAX_AMBIGUOUS of an env's points."""
from types import SimpleNamespace

import numpy as np

from occupancy_ref import EPS, MAX_AMBIGUOUS  # noqa: F401

NAV_NONE = 1 << 30
NO_SCORE = np.iinfo(np.int64).max
OK, ARRIVED, BLOCKED, OFF_GRID = 0, 1, 2, 3


def place(pose, points, x0, y0, cell, nx, ny):
    """pose [3, B] (x, y, theta; fp32 values), points [K, P, 2] -> cell [B, K, P] int64 (the fp64 cell, -1 outside), sure [B, K, P]
    bool, cand [B, K, P, 4] int64 (the cells the point's box meets, repeated to fill four; all of them `cell` where sure) and
    margin [B, K, P, 2] in metres."""
    x0, y0, cell = (float(np.float32(q)) for q in (x0, y0, cell))      # the entry takes them as fp32
    pose = np.asarray(pose, np.float64)
    pts = np.asarray(points, np.float64)
    B = pose.shape[1]
    K, P = pts.shape[:2]
    x, y, th = (pose[i][:, None, None] for i in range(3))
    px, py = pts[None, ..., 0], pts[None, ..., 1]
    with np.errstate(invalid="ignore"):
        c, s = np.cos(th), np.sin(th)
        w = np.stack((x + c * px - s * py, y + s * px + c * py), -1)      # [B, K, P, 2]
        S = np.stack((np.abs(x) + np.abs(px) + np.abs(py), np.abs(y) + np.abs(px) + np.abs(py)), -1)
        org = np.array([x0, y0], np.float64)
        m = EPS * S + 2.0 ** -22 * np.abs(w - org)
        finite = np.isfinite(w).all(-1) & np.isfinite(pose).all(0)[:, None, None]
        wz, mz = np.where(finite[..., None], w, 0.0), np.where(finite[..., None], m, 0.0)
        lo = np.floor((wz - mz - org) / cell).astype(np.int64)
        hi = np.floor((wz + mz - org) / cell).astype(np.int64)
        mid = np.floor((wz - org) / cell).astype(np.int64)
    assert (hi - lo <= 1).all(), "a margin wider than a cell: not a case of this reference"
    lim = np.array([nx, ny])

    def linear(ij):
        inside = ((ij >= 0) & (ij < lim)).all(-1) & finite
        return np.where(inside, ij[..., 1] * nx + ij[..., 0], -1)

    cand = np.stack([linear(np.stack((a[..., 0], b[..., 1]), -1)) for a in (lo, hi) for b in (lo, hi)], -1)
    sure = (lo == hi).all(-1) | ~finite
    return SimpleNamespace(cell=linear(mid), sure=sure, cand=cand, margin=m, B=B, K=K, P=P)


def unsure_share(pl):
    """Per env the share of unsure points."""
    return (~pl.sure).reshape(pl.B, -1).mean(1)


def check_cells(got, pl):
    """The comparison rule of the float stage: every sure point equals the reference cell, every unsure one is among its candidates.
    Returns the list of violations (b, k, p, got, candidates)."""
    got = np.asarray(got).astype(np.int64).reshape(pl.cell.shape)
    ok = np.where(pl.sure, got == pl.cell, (got[..., None] == pl.cand).any(-1))
    return [(int(b), int(k), int(p), int(got[b, k, p]), pl.cand[b, k, p].tolist()) for b, k, p in np.argwhere(~ok)]


def decide(cells, cost, potential, command, bias=None, twist=None, *, own, pose_finite=None, lethal=253, outside_is_free=False, goal_weight=1,
           obstacle_weight=20, arrive_potential=0, max_dv=np.inf, max_dw=np.inf):
    """cells [B, K, P] (linear cells, -1 outside; the last point of a candidate is its scoring point), cost uint8 [B, ny, nx] or None,
    potential int32 [B, ny, nx], command fp32 [K, 2], bias int [K] or None, twist fp32 [2, B] or None, own [B] the robot's own cell
    (-1 outside), pose_finite [B] bool (all True if None).  Returns score [B, K] int64, chosen [B], status [B] (best is their pair)
    and cmd fp32 [2, B]."""
    cells = np.asarray(cells).astype(np.int64)
    B, K, P = cells.shape
    pot = np.asarray(potential).astype(np.int64).reshape(B, -1)
    command = np.asarray(command, np.float32)
    own = np.asarray(own).astype(np.int64)
    pose_finite = np.ones(B, bool) if pose_finite is None else np.asarray(pose_finite, bool)
    at = np.clip(cells, 0, None).reshape(B, K * P)
    inside = cells >= 0
    if cost is None:
        c = np.zeros((B, K, P), np.int64)
    else:
        c = np.take_along_axis(np.asarray(cost).astype(np.int64).reshape(B, -1), at, 1).reshape(B, K, P)
    c = np.where(inside, c, 0)
    swept_in, swept_c, goal_cell = inside[..., :P - 1], c[..., :P - 1], cells[..., P - 1]
    blocked = (swept_in & (swept_c >= lethal)).any(-1)
    if not outside_is_free:
        blocked |= (~swept_in).any(-1)
    g = np.take_along_axis(pot, np.clip(goal_cell, 0, None), 1)
    blocked |= (goal_cell < 0) | (g >= NAV_NONE)
    if twist is not None:
        tw = np.asarray(twist, np.float32)
        with np.errstate(invalid="ignore"):
            dv = np.abs(command[None, :, 0] - tw[0][:, None])      # fp32 throughout
            dw = np.abs(command[None, :, 1] - tw[1][:, None])
            assert dv.dtype == np.float32 and dw.dtype == np.float32
            blocked |= ~((dv <= np.float32(max_dv)) & (dw <= np.float32(max_dw)))
    o = swept_c.max(-1) if P > 1 else np.zeros((B, K), np.int64)
    b = np.zeros(K, np.int64) if bias is None else np.asarray(bias).astype(np.int64)
    score = np.where(blocked, NO_SCORE, goal_weight * g + obstacle_weight * o + b[None, :])
    first = score.argmin(1)      # numpy's argmin returns the first of equal minima: the smallest k
    best = score[np.arange(B), first]
    own_pot = pot[np.arange(B), np.clip(own, 0, None)]
    off = ~pose_finite | (own < 0)
    status = np.where(off, OFF_GRID, np.where(own_pot <= arrive_potential, ARRIVED, np.where(best == NO_SCORE, BLOCKED, OK)))
    chosen = np.where(status == OK, first, -1)
    cmd = np.where((status == OK)[None, :], command[first].T, np.float32(0)).astype(np.float32)
    return SimpleNamespace(score=score, chosen=chosen.astype(np.int32), status=status.astype(np.int32),
                           best=np.stack((chosen, status), 1).astype(np.int32), cmd=cmd)


# The float stage of tests/test_gpu_drive.py: three poses off the cell edges on an origin that is no multiple of the cell, and the
# two tables it places (tests/test_drive_ref.py asserts the cap on unsure points for exactly these).
FLOAT_STAGE = SimpleNamespace(nx=128, ny=96, cell=0.05, origin=(-3.187, -2.379),
                              pose=np.array([[0.3337, -1.0411, 1.271], [-0.2213, 0.7532, 1.113], [0.4, 2.3, -1.9]], np.float32))
FOOTPRINT = [(0.17, 0.17), (0.17, -0.17), (-0.17, -0.17), (-0.17, 0.17), (0.0, 0.0)]


def float_stage_tables():
    """[(name, command [K, 2], points [K, P, 2])] as fp32 numpy arrays: the default arcs, and arcs with a square footprint."""
    from stretch_mujoco_amd.utils import arc_candidates

    out = []
    for name, kw in (("default", {}), ("footprint", dict(footprint=FOOTPRINT, samples=7, horizon=2.0))):
        c = arc_candidates(device="cpu", **kw)
        out.append((name, c.command.numpy(), c.points.numpy()))
    return out
