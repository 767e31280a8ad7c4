"""numpy reference of smj_scan_to_particles (include/smj_localize.h).  A helper, not a test.  Two parts, as the entry has two:

weights() -- the sum S of the field under the scan's points, per particle, from the cells of tests/scanmatch_ref.py's place() with
every particle as a pose and the rotation table [0] (the header: the matcher's operations at a rotation offset of 0).  place() gives
a point a margin; a point whose box lies in one cell is SURE, any other has up to four candidate cells.  So a particle has an
interval: S_lo takes the smallest field value among the candidates of every point, S_hi the largest, and S_mid the cell of the fp64
point.  The device's S_j must lie in [S_lo, S_hi]; they differ only by unsure points.  The comparison means something while unsure
(particle, point) pairs are few: callers assert at most MAX_AMBIGUOUS of an env's pairs.

resample() -- everything after S: Python ints (the best particle, cut, w, total, the sum of squares, the status, the thresholds of
systematic resampling, the ancestors, the count of distinct ancestors, the effective sample size).  It is exact and the device must
equal it bit for bit when fed the device's own S; move() applies the ancestors and the noise in fp32, one add per word.

The closed loop (LOOP, closed_loop()): the room of tests/scanmatch_ref.py mapped from ROOM_POSES, the likelihood at
mapping_ref.LOOP_SIGMA, three robots standing at the three poses of the map, and per robot LOOP.particles particles spread uniformly
over +-1 m, +-30 degrees round a centre that is LOOP.offset[e] off the truth (0.63 m and 17 degrees at the least).  LOOP.updates
updates of weigh, resample, add noise (sigma LOOP.sigma_xy, LOOP.sigma_theta), then LOOP.extra more.  Measured with this file's
S_mid, error of the best particle per update as (metres, degrees), envs 0 / 1 / 2:
    update  0: (0.070, 0.78)  (0.082, 2.63)  (0.103, 0.56)    effective sample sizes 1 / 2 / 1
    update  1: (0.017, 0.29)  (0.070, 0.08)  (0.043, 0.32)    effective sample sizes 24 / 13 / 33
    update  2: (0.018, 0.12)  (0.020, 0.26)  (0.017, 0.08)    effective sample sizes 804 / 32 / 158
    update  3: (0.010, 0.01)  (0.006, 0.12)  (0.016, 0.25)    effective sample sizes 838 / 583 / 786
    update  4: (0.010, 0.15)  (0.012, 0.10)  (0.008, 0.07)    effective sample sizes 828 / 791 / 829
    update  5: (0.003, 0.18)  (0.009, 0.03)  (0.018, 0.07)    effective sample sizes 861 / 830 / 859
    update  6: (0.012, 0.26)  (0.004, 0.27)  (0.013, 0.12)    effective sample sizes 840 / 838 / 841
    update  7: (0.012, 0.17)  (0.006, 0.10)  (0.001, 0.21)    effective sample sizes 868 / 838 / 884
    update  8: (0.009, 0.19)  (0.008, 0.04)  (0.018, 0.19)    effective sample sizes 853 / 837 / 876
    update  9: (0.018, 0.07)  (0.008, 0.01)  (0.018, 0.43)    effective sample sizes 851 / 803 / 821
    update 10: (0.011, 0.10)  (0.005, 0.11)  (0.009, 0.04)    effective sample sizes 852 / 787 / 866
The bound of tests/test_localize_ref.py on the last LOOP.extra + 1 updates is half a cell and 1 degree; the device test asserts one cell
and 2 degrees, for the device may break an unsure cell the other way and so take another branch of the resampling."""
from types import SimpleNamespace

import numpy as np

import scanmatch_ref
from scanmatch_ref import MAX_AMBIGUOUS, NO_CELL  # noqa: F401

OK, FEW, LOST = 0, 1, 2
MAX_PARTICLES, MAX_SPAN = 4096, 1 << 18
STAT_WORDS = 8
NAN_BITS = 0x7FC00000


def cells_of(points, margins, particles, x0, y0, cell, nx, ny):
    """One env: points, margins [K, 2] (scanmatch_ref.frame_points), particles [3, P] (fp32 values) -> mid [P, K, 2] (the cell of the
    fp64 point, NO_CELL twice for none), cand [P, K, 4, 2] (the cells its box meets), unsure [P, K] bool, n (the counting rays)."""
    particles = np.asarray(particles, np.float32)
    P, K = particles.shape[1], len(points)
    mid, cand, unsure = np.empty((P, K, 2), np.int64), np.empty((P, K, 4, 2), np.int64), np.empty((P, K), bool)
    n = 0
    for at in range(0, P, 512):      # chunks bound the memory of place()
        part = particles[:, at:at + 512]
        m = part.shape[1]
        pl = scanmatch_ref.place(np.broadcast_to(points, (m, K, 2)), np.broadcast_to(margins, (m, K, 2)), part, np.zeros(1, np.float32), x0, y0, cell, nx, ny)
        mid[at:at + m], cand[at:at + m], unsure[at:at + m] = pl.cell[:, 0], pl.cand[:, 0], ~pl.sure[:, 0]
        n = int(pl.n[0])
    return SimpleNamespace(mid=mid, cand=cand, unsure=unsure, n=n)


def sums(cells, field):
    """cells (cells_of) and field uint8 [ny, nx] -> S_lo, S_mid, S_hi int64 [P], with .unsure and .n of the cells."""
    field = np.asarray(field)
    assert field.dtype == np.uint8 and field.ndim == 2
    ny, nx = field.shape
    flat = field.reshape(-1).astype(np.int64)

    def value(c):
        ix, iy = c[..., 0], c[..., 1]
        on = (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny)      # NO_CELL is off every grid
        return np.where(on, flat[np.where(on, iy * nx + ix, 0)], 0)

    v = value(cells.cand)                                        # [P, K, 4]
    return SimpleNamespace(lo=v.min(-1).sum(-1), mid=value(cells.mid).sum(-1), hi=v.max(-1).sum(-1), unsure=cells.unsure, n=cells.n)


def weights(points, margins, particles, field, x0, y0, cell):
    """One env: cells_of() and sums() in one call."""
    ny, nx = np.asarray(field).shape
    return sums(cells_of(points, margins, particles, x0, y0, cell, nx, ny), field)


def unsure_share(w):
    """The share of unsure (particle, point) pairs of an env."""
    return float(w.unsure.mean())


def threshold(k, total, o, P):
    return (k * total + o) // P


def resample(S, draw, span, min_points, n, resample):
    """One env, in Python ints: S [P] the raw sums, draw the env's random word, n the counting rays -> stat (8 ints), ancestors (P
    ints), status, w (P ints)."""
    S = [int(v) for v in S]
    P = len(S)
    draw, span, n = int(draw), int(span), int(n)
    assert 1 <= P <= MAX_PARTICLES and 1 <= span <= MAX_SPAN and 0 <= draw < 1 << 32 and all(0 <= v < 1 << 18 for v in S)
    s_max = max(S)
    best = S.index(s_max)      # the first of equal maxima: the smallest j
    status = FEW if n < min_points else LOST if s_max == 0 else OK
    cut = max(s_max - span, 0)
    w = [max(v - cut, 0) for v in S]
    total, sq = sum(w), sum(v * v for v in w)
    assert total <= 1 << 30
    ancestors, distinct = list(range(P)), 0
    if status == OK and resample:
        o = (draw * total) >> 32
        C, run = [], 0
        for v in w:
            run += v
            C.append(run)
        ancestors, j = [], 0
        for k in range(P):
            u = threshold(k, total, o, P)
            assert u < total
            while C[j] <= u:      # u is non-decreasing in k: the smallest j with C_j > u_k never moves back
                j += 1
            ancestors.append(j)
        distinct = len(set(ancestors))
    ok = status == OK
    stat = [best if ok else -1, s_max, n, status, total if ok else 0, total * total // sq if ok else 0, cut, distinct]
    return SimpleNamespace(stat=stat, ancestors=ancestors, status=status, w=w, total=total, best=best)


def move(particles, ancestors, noise=None):
    """particles [3, P] fp32, ancestors [P] -> the resampled particles [3, P] fp32: the ancestor's bits, plus the noise in one fp32 add."""
    out = np.asarray(particles, np.float32)[:, np.asarray(ancestors, np.int64)]
    return out if noise is None else (out + np.asarray(noise, np.float32)).astype(np.float32)


def pose_bits(particles, stat):
    """uint32 [3]: pose_out of an env -- the best particle's bits with OK, the NaN pattern otherwise."""
    if stat[3] != OK:
        return np.full(3, NAN_BITS, np.uint32)
    return np.ascontiguousarray(np.asarray(particles, np.float32)[:, stat[0]]).view(np.uint32)


def spread(center, half_extent, P, rng):
    """[3, P] fp32: a uniform box round `center`."""
    c, h = np.asarray(center, np.float64), np.asarray(half_extent, np.float64)
    return (c[:, None] + h[:, None] * rng.uniform(-1.0, 1.0, (3, P))).astype(np.float32)


# ---- the float stage of tests/test_gpu_localize.py: the grids, scans and priors of scanmatch_ref.FLOAT_STAGE, and seeded particles
SHAPES = (1, 7, 64, 257, 1024, 4096)      # one particle; less than a wave; a wave; one past a wave; past the block of 512; the cap


def float_stage_particles(P, B=3, seed=3):
    """fp32 [3, B, P]: particles within 0.3 m and 0.3 rad of FLOAT_STAGE.prior (even slots) and .truth (odd slots) of their env; of
    every 13 one lies 50 m off the grid, of every 17 one has a NaN coordinate, of every 29 one an infinite heading."""
    fs = scanmatch_ref.FLOAT_STAGE
    rng = np.random.default_rng(seed + P)
    out = np.empty((3, B, P), np.float32)
    for e in range(B):
        base = np.where((np.arange(P) % 2 == 0)[None, :], np.asarray(fs.prior[e], np.float64)[:, None], np.asarray(fs.truth[e], np.float64)[:, None])
        out[:, e] = (base + rng.uniform(-0.3, 0.3, (3, P))).astype(np.float32)
    j = np.arange(P)
    out[0][:, j % 13 == 5] += 50.0
    out[1][:, j % 17 == 7] = np.nan
    out[2][:, j % 29 == 11] = np.inf
    return out


# ---- the closed loop of tests/test_localize_ref.py and tests/test_gpu_localize.py
LOOP = SimpleNamespace(particles=2048, updates=8, extra=3, span=4096, min_points=30, sigma_xy=0.02, sigma_theta=np.deg2rad(0.5),
                       half_extent=(1.0, 1.0, np.deg2rad(30.0)), limits=(0.2, 5.0), seed=11,
                       offset=np.array([(0.45, 0.45, np.deg2rad(17.0)), (-0.5, 0.4, np.deg2rad(-20.0)), (0.4, -0.5, np.deg2rad(18.0))]),
                       bound=(0.05, np.deg2rad(2.0)))      # one cell of ROOM_GRID, 2 degrees: what the device test asserts


def loop_field():
    """uint8 [ny, nx]: the likelihood field of the room mapped from ROOM_POSES with unit rays, at mapping_ref.LOOP_SIGMA."""
    import torch

    import mapping_ref
    from stretch_mujoco_amd.datamodels import StatusStretchDistanceField

    g = scanmatch_ref.ROOM_GRID
    o, d, _, _ = scanmatch_ref.unit_rays()
    scans = [scanmatch_ref.room_scan(p, o, d) for p in scanmatch_ref.ROOM_POSES]
    occ = scanmatch_ref.hit_cells(scanmatch_ref.ROOM_POSES, scans, o, d, g, *LOOP.limits)
    dist2 = torch.tensor(scanmatch_ref.dist2_of(occ))[None]
    df = StatusStretchDistanceField(time=None, dist2=dist2, nearest=None, origin=g.origin, cell=g.cell, frame="world")
    return df.likelihood(mapping_ref.LOOP_SIGMA).numpy()[0]


def loop_inputs(B=3):
    """The seeded inputs of the loop, the same on the CPU and on the device: truth [B, 3], centre [B, 3], the first particles
    [3, B, P] fp32, and per update the noise [3, B, P] fp32 and the draws [B] uint32."""
    rng = np.random.default_rng(LOOP.seed)
    truth = scanmatch_ref.ROOM_POSES[:B]
    center = truth + LOOP.offset[:B]
    first = np.stack([spread(center[e], LOOP.half_extent, LOOP.particles, rng) for e in range(B)], 1)
    steps = LOOP.updates + LOOP.extra
    sig = np.array([LOOP.sigma_xy, LOOP.sigma_xy, LOOP.sigma_theta])[:, None, None]
    noise = [(sig * rng.standard_normal((3, B, LOOP.particles))).astype(np.float32) for _ in range(steps)]
    draws = [rng.integers(0, 1 << 32, B, dtype=np.uint64).astype(np.uint32) for _ in range(steps)]
    return SimpleNamespace(truth=truth, center=center, first=first, noise=noise, draws=draws, steps=steps)


def pose_error(est, truth):
    """(metres, radians) between a pose estimate and the truth; the angle wrapped."""
    est, truth = np.asarray(est, np.float64), np.asarray(truth, np.float64)
    dth = (est[2] - truth[2] + np.pi) % (2 * np.pi) - np.pi
    return float(np.hypot(est[0] - truth[0], est[1] - truth[1])), float(abs(dth))


def closed_loop(rays=None):
    """The loop with this file alone (S_mid as the weight).  Returns errors [steps, B, 2] of the best particle per update (metres,
    radians), the statuses [steps, B] and the effective sample sizes [steps, B]."""
    g = scanmatch_ref.ROOM_GRID
    o, d, So, Sd = scanmatch_ref.unit_rays() if rays is None else rays
    field = loop_field()
    inp = loop_inputs()
    B = len(inp.truth)
    pts = [scanmatch_ref.frame_points(o, d, So, Sd, scanmatch_ref.room_scan(inp.truth[e], o, d).astype(np.float32).astype(np.float64), *LOOP.limits) for e in range(B)]
    particles = inp.first.copy()
    errors, statuses, ess = [], [], []
    for i in range(inp.steps):
        row_e, row_s, row_n = [], [], []
        nxt = np.empty_like(particles)
        for e in range(B):
            w = weights(pts[e][0], pts[e][1], particles[:, e], field, *g.origin, g.cell)
            res = resample(w.mid, inp.draws[i][e], LOOP.span, LOOP.min_points, w.n, 1)
            row_s.append(res.status)
            row_n.append(res.stat[5])
            row_e.append(pose_error(particles[:, e, res.best], inp.truth[e]))
            nxt[:, e] = move(particles[:, e], res.ancestors, inp.noise[i][:, e])
        particles = nxt
        errors.append(row_e)
        statuses.append(row_s)
        ess.append(row_n)
    return np.array(errors), np.array(statuses), np.array(ess)
