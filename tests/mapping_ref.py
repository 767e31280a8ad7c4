"""numpy reference of smj_scan_to_map (include/smj_mapping.h).  A helper, not a test.  Two parts, as the entry has two:

integrate() -- everything after the rays have their cells: integers (the closed-form line of tests/occupancy_ref.py walked into hit
and miss, the status of an env, the gate, accumulate, the info counts).  It is exact and the device must equal it bit for bit.

place_rays() -- the cells (ax, ay, bx, by) of the two ends of every ray, in fp64, with a MARGIN per end and coordinate.  The header
lists the fp32 operations:
    o, d                                         (tests/occupancy_ref.py's ray_geometry: the ray in the robot's frame)
    p = o + len d                                (the end of the ray in the robot's frame)
    gx = x + c qx - s qy,  ix = floor((gx - x0) / cell)     (gy, iy alike; c = cosf(theta), s = sinf(theta); q = o and q = p)
The margin of an end is that of tests/scanmatch_ref.py's place():
  * tests/occupancy_ref.py's margin of the point in the frame, EPS * So for the origin and EPS * (So + |len| Sd) for the end (So, Sd:
    the sums of the magnitudes o and d are summed from), carried through the rotation: (|c| mx + |s| my, |s| mx + |c| my);
  * the terms for the transform and the cell: EPS * (|x| + |qx| + |qy|) + 2^-22 * |g - x0|.
The matcher's band of 32 cells round the grid does not apply here; the guards of the header do: the origin's index within +-2^20,
the end within 16384 cells of it in either coordinate.  A ray is SURE when both of its ends have ONE candidate cell; any other kept
ray is UNSURE, with up to four candidates per end.  A ray that is dropped by its range, and every ray of a pose that is not finite,
has no cells, surely.  The comparison means something while unsure rays are few: callers assert at most occupancy_ref.MAX_AMBIGUOUS
of an env's rays."""
from types import SimpleNamespace

import numpy as np

import occupancy_ref
from occupancy_ref import CLEAR, DROP, EPS, MAX_AMBIGUOUS, RETURN  # noqa: F401

NO_CELL = -(1 << 30)
OK, GATED, OFF = 0, 1, 2
GUARD_ORIGIN = 1 << 20
GUARD_REACH = 16384


def place_rays(o, d, So, Sd, ranges, pose, x0, y0, cell, r_min, r_max, no_return_clears):
    """One env: rays (o, d, So, Sd [K, 2] as occupancy_ref.ray_geometry gives them in the robot's frame), ranges [K] (fp32 values),
    pose (x, y, theta; fp32 values) -> kind [K] (the classification of the range), kept [K] bool, cell [K, 4] int64 ((ax, ay, bx, by)
    of the fp64 ends, NO_CELL four times where the ray is not kept), sure [K] bool, cand_a, cand_b [K, 4, 2] (the cells the box of an
    end meets), origin_sure [K] bool."""
    x0, y0, cell = (float(np.float32(q)) for q in (x0, y0, cell))
    x, y, th = (float(np.float32(q)) for q in pose)
    o, d, So, Sd = (np.asarray(q, np.float64) for q in (o, d, So, Sd))
    K = o.shape[0]
    kind, length = occupancy_ref.classify(ranges, float(np.float32(r_min)), float(np.float32(r_max)), no_return_clears)
    org = np.array([x0, y0])
    if not np.isfinite([x, y, th]).all():
        none = np.full((K, 4), NO_CELL, np.int64)
        return SimpleNamespace(kind=kind, kept=np.zeros(K, bool), cell=none, sure=np.ones(K, bool), cand_a=none.reshape(K, 2, 2).repeat(2, 1),
                               cand_b=none.reshape(K, 2, 2).repeat(2, 1), origin_sure=np.ones(K, bool))
    c, s = np.cos(th), np.sin(th)

    def laid(q, mq):
        """points q [K, 2] of the robot's frame with margins mq -> (lo, mid, hi) float indices [K, 2]"""
        g = np.stack((x + c * q[:, 0] - s * q[:, 1], y + s * q[:, 0] + c * q[:, 1]), 1)
        S = np.stack((abs(x) + np.abs(q).sum(1), abs(y) + np.abs(q).sum(1)), 1)
        carried = np.stack((abs(c) * mq[:, 0] + abs(s) * mq[:, 1], abs(s) * mq[:, 0] + abs(c) * mq[:, 1]), 1)
        m = EPS * S + 2.0 ** -22 * np.abs(g - org) + carried
        return np.floor((g - m - org) / cell), np.floor((g - org) / cell), np.floor((g + m - org) / cell)

    p = o + length[:, None] * d
    alo, amid, ahi = laid(o, EPS * So)
    blo, bmid, bhi = laid(p, EPS * (So + np.abs(length)[:, None] * Sd))
    live = kind != DROP
    assert (ahi - alo <= 1)[live].all() and (bhi - blo <= 1)[live].all(), "a margin wider than a cell: not a case of this reference"

    def guards(a, b):
        with np.errstate(invalid="ignore"):
            return (np.abs(a) <= GUARD_ORIGIN).all(1) & (np.abs(b - a) <= GUARD_REACH).all(1)

    kept = live & guards(amid, bmid)
    for a in (alo, ahi):
        for b in (blo, bhi):
            assert (guards(a, b) == guards(amid, bmid))[live].all(), "a ray within its margin of a guard: not a case of this reference"

    def cells(f):
        return np.where(kept[:, None], np.where(kept[:, None], f, 0).astype(np.int64), NO_CELL)

    def candidates(lo, hi):
        return np.stack([cells(np.stack((u[:, 0], v[:, 1]), 1)) for u in (lo, hi) for v in (lo, hi)], 1)      # [K, 4, 2]

    cand_a, cand_b = candidates(alo, ahi), candidates(blo, bhi)
    origin_sure = (cand_a == cand_a[:, :1]).all((1, 2))
    sure = origin_sure & (cand_b == cand_b[:, :1]).all((1, 2))
    return SimpleNamespace(kind=kind, kept=kept, cell=np.concatenate((cells(amid), cells(bmid)), 1), sure=sure, cand_a=cand_a, cand_b=cand_b,
                           origin_sure=origin_sure)


def unsure_share(pl):
    """The share of unsure rays among all rays of the env."""
    return float((~pl.sure).mean())


def check_cells(got, pl):
    """The comparison rule of the float stage for one env: got int [K, 4].  A sure ray equals the reference (NO_CELL four times where
    it is not kept), an unsure one has each end among its candidates.  Returns the list of violations (k, got, reference)."""
    got = np.asarray(got).astype(np.int64).reshape(-1, 4)
    in_a = (got[:, None, :2] == pl.cand_a).all(-1).any(-1)
    in_b = (got[:, None, 2:] == pl.cand_b).all(-1).any(-1)
    ok = np.where(pl.sure, (got == pl.cell).all(1), in_a & in_b)
    return [(int(k), got[k].tolist(), pl.cell[k].tolist()) for k in np.nonzero(~ok)[0]]


def status_of(pose, gate=None):
    """pose [3, B] (fp32 values), gate [B] ints or None -> status [B]: OFF for a pose that is not finite, before the gate."""
    pose = np.asarray(pose, np.float32)
    gate = np.zeros(pose.shape[1], np.int64) if gate is None else np.asarray(gate).astype(np.int64)
    return np.where(~np.isfinite(pose).all(0), OFF, np.where(gate != 0, GATED, OK)).astype(np.int32)


def integrate(cells, kind, status, nx, ny, hit=None, miss=None, accumulate=False):
    """cells [B, K, 4] ((ax, ay, bx, by), NO_CELL four times for a ray that is not kept), kind [B, K] (occupancy_ref.classify of the
    ranges), status [B] (status_of) -> hit, miss int32 [B, ny, nx] and info int32 [B, 4].  hit, miss: what the buffers hold before
    the call (None: zeros); with accumulate they are added to, without it overwritten -- zeroed for an env that is not OK."""
    cells, kind, status = np.asarray(cells).astype(np.int64), np.asarray(kind), np.asarray(status)
    B, K, _ = cells.shape
    out_h = np.zeros((B, ny, nx), np.int64) if hit is None or not accumulate else np.asarray(hit).astype(np.int64).copy()
    out_m = np.zeros((B, ny, nx), np.int64) if miss is None or not accumulate else np.asarray(miss).astype(np.int64).copy()
    info = np.zeros((B, 4), np.int64)
    info[:, 0] = status
    for e in np.nonzero(status == OK)[0]:
        kept = cells[e, :, 0] != NO_CELL
        assert (kept | (cells[e] == NO_CELL).all(1)).all() and not (kept & (kind[e] == DROP)).any()
        info[e, 1] = (kept & (kind[e] == RETURN)).sum()
        info[e, 2] = (kept & (kind[e] == CLEAR)).sum()
        info[e, 3] = (~kept & (kind[e] != DROP)).sum()
        for k in np.nonzero(kept)[0]:
            xs, ys = occupancy_ref.line_cells(*(int(v) for v in cells[e, k]))
            inside = (xs >= 0) & (xs < nx) & (ys >= 0) & (ys < ny)
            last = np.zeros(len(xs), bool)
            last[-1] = kind[e, k] == RETURN
            np.add.at(out_h[e], (ys[inside & last], xs[inside & last]), 1)
            np.add.at(out_m[e], (ys[inside & ~last], xs[inside & ~last]), 1)
    return out_h.astype(np.int32), out_m.astype(np.int32), info.astype(np.int32)


def worst_dist2(hit, truth_dist2):
    """The largest squared distance (cells) from a hit cell of `hit` [ny, nx] to the nearest obstacle of the map `truth_dist2` was made of."""
    occ = np.asarray(hit) > 0
    return int(np.asarray(truth_dist2)[occ].max()) if occ.any() else 0


# The closed loop of tests/test_mapping_ref.py and tests/test_gpu_mapping.py in the synthetic room of tests/scanmatch_ref.py: 8 true
# poses, and an odometry whose every increment is off by a constant bias.
LOOP_POSES = np.array([(0.12 * i, -0.08 * i, 0.11 * i) for i in range(8)])
LOOP_BIAS = np.array((0.07, -0.06, np.deg2rad(2.0)))
LOOP_SIGMA = 0.10
LOOP_LIMITS = (0.2, 5.0)
LOOP_MAX_DIST2 = 8          # one cell of pose error per axis plus 0.5 degrees over 5 m < one cell: two cells per axis
LOOP_DEAD_RECKONING = 100   # what the dead-reckoned map must exceed, or the test shows nothing
# One lattice step, as measured on fp32 poses.  An estimate sits on the lattice of its prior, and the prior is the estimate before it
# plus an increment: two fp32 roundings per step of values below 1 (half an ulp, 3e-8, each), seven steps: 4.2e-7 m or rad off the
# lattice a real-number loop would walk, which is 4.8e-5 steps of half a degree (8.4e-6 cells).  An error of exactly one step -- the
# biases are whole steps in theta -- may therefore measure 1 + 4.8e-5; 1e-4 is that, rounded up.
LOOP_ROUNDING = 1e-4


def within_one_step(errors):
    """The criterion of the closed loop on lattice errors (lattice_error) of any shape."""
    return bool((np.abs(np.asarray(errors)) <= 1 + LOOP_ROUNDING).all())


def lattice_error(est, truth, cell, step):
    """(x, y, theta) error of a pose in lattice steps, as floats."""
    e = np.asarray(est, np.float64) - np.asarray(truth, np.float64)
    return e / np.array([cell, cell, step])
