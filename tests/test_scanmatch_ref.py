"""The numpy reference of smj_scan_to_pose (tests/scanmatch_ref.py) on the CPU: its exact stage against a second, long-hand loop, the
tie rule on a hand-made field, the cap on unsure points for the float-stage cases the GPU tests use, the recovery of known poses in
a synthetic room, and the torch helpers of the Python layer (likelihood(), scan_angles(), offset(), fit(), refined()) on CPU
tensors."""
import os

import numpy as np
import pytest
import torch

import scanmatch_ref as ref
from conftest import ROOT
from stretch_mujoco_amd import model_blob
from stretch_mujoco_amd.datamodels import StatusStretchDistanceField, StatusStretchScanMatch
from stretch_mujoco_amd.utils import scan_angles


def _longhand(cells, field, pose, angles, cell, n, wx, wy, bias, shift_weight, min_points):
    """decide() once more, one candidate and one point at a time."""
    B, T, K, _ = cells.shape
    ny, nx = field.shape[1:]
    score = np.zeros((B, T, 2 * wy + 1, 2 * wx + 1), np.int64)
    best = np.zeros((B, 4), np.int64)
    for e in range(B):
        top = None
        for t in range(T):
            b = 0 if bias is None else min(max(int(bias[t]), 0), 1 << 20)
            for dy in range(-wy, wy + 1):
                for dx in range(-wx, wx + 1):
                    S = 0
                    for k in range(K):
                        ix, iy = int(cells[e, t, k, 0]), int(cells[e, t, k, 1])
                        if ix == ref.NO_CELL:
                            continue
                        if 0 <= ix + dx < nx and 0 <= iy + dy < ny:
                            S += int(field[e, iy + dy, ix + dx])
                    J = S - b - shift_weight * (dx * dx + dy * dy)
                    score[e, t, dy + wy, dx + wx] = J
                    i = (t * (2 * wy + 1) + dy + wy) * (2 * wx + 1) + dx + wx
                    if top is None or J > top[0]:      # strictly larger: the first of equal scores stays
                        top = (J, i)
        status = ref.OFF if not np.isfinite(pose[:, e]).all() else ref.FEW if n[e] < min_points else ref.OK
        best[e] = (top[1], top[0], n[e], status) if status == ref.OK else (-1, 0, n[e], status)
    return score, best


def test_decide_equals_a_long_hand_loop():
    rng = np.random.default_rng(11)
    B, T, K, nx, ny = 3, 4, 40, 13, 9
    field = rng.integers(0, 256, (B, ny, nx)).astype(np.uint8)
    field[1] = 255                                      # ties everywhere
    cells = np.stack((rng.integers(-40, nx + 40, (B, T, K)), rng.integers(-40, ny + 40, (B, T, K))), -1)
    gone = rng.random((B, T, K)) < 0.2
    cells[gone] = ref.NO_CELL
    cells[~gone & ((cells[..., 0] < -32) | (cells[..., 0] >= nx + 32) | (cells[..., 1] < -32) | (cells[..., 1] >= ny + 32))] = ref.NO_CELL
    pose = np.array([[0.1, -0.2, np.nan], [0.3, 0.4, 0.5], [0.0, 1.0, -1.0]], np.float32)
    angles = np.array([0.0, -0.1, 0.1, 0.25], np.float32)
    n = np.array([40, 3, 17])
    for wx, wy, bias, sw, mp in ((0, 0, None, 0, 1), (3, 2, [5, -7, 1 << 22, 0], 3, 10), (1, 4, None, 1024, 30)):
        d = ref.decide(cells, field, pose, angles, 0.05, n, wx=wx, wy=wy, bias=bias, shift_weight=sw, min_points=mp)
        score, best = _longhand(cells, field, pose, angles, 0.05, n, wx, wy, bias, sw, mp)
        assert np.array_equal(d.score, score) and np.array_equal(d.best, best), (wx, wy)
        for e in range(B):
            if d.best[e, 3] != ref.OK:
                assert d.pose[:, e].tobytes() == pose[:, e].tobytes()      # the prior, bit for bit (a NaN included)
            else:
                t, dy, dx = ref.unindex(int(d.best[e, 0]), wx, wy)
                assert ref.index(t, dy, dx, wx, wy) == d.best[e, 0]
                assert d.pose[2, e] == np.float32(pose[2, e] + angles[t])
                assert abs(float(d.pose[0, e]) - (float(pose[0, e]) + dx * float(np.float32(0.05)))) < 1e-7


def test_the_smallest_index_wins_among_equal_maxima():
    """Two points one cell apart in x, a field with two equal peaks: shifts (dy, dx) = (0, -1) and (0, +2) both collect 400; so does
    every rotation, since the cells are given.  The winner is rotation 0, dx = -1."""
    field = np.zeros((1, 5, 9), np.uint8)
    field[0, 2, 2:4] = 200
    field[0, 2, 5:7] = 200
    cells = np.zeros((1, 2, 2, 2), np.int64)
    cells[0, :, 0] = (3, 2)
    cells[0, :, 1] = (4, 2)
    d = ref.decide(cells, field, np.zeros((3, 1), np.float32), np.array([0.0, 0.1], np.float32), 0.05, [2], wx=2, wy=1, min_points=1)
    assert d.score.max() == 400 and (d.score == 400).sum() == 4
    assert ref.unindex(int(d.best[0, 0]), 2, 1) == (0, 0, -1) and d.best[0].tolist() == [ref.index(0, 0, -1, 2, 1), 400, 2, ref.OK]
    # a bias on rotation 0 hands the win to rotation 1, same shift
    d = ref.decide(cells, field, np.zeros((3, 1), np.float32), np.array([0.0, 0.1], np.float32), 0.05, [2], wx=2, wy=1, bias=[1, 0], min_points=1)
    assert ref.unindex(int(d.best[0, 0]), 2, 1) == (1, 0, -1) and d.pose[2, 0] == np.float32(0.1)


def _model_rays():
    """(o, d, So, Sd) of the shipped model's lidar in the frame of the rays' own body: site_pos and the sites' +Z columns as stored."""
    with open(os.path.join(ROOT, "stretch_mujoco_amd", "models", "stretch_scene.smjb"), "rb") as f:
        m = model_blob.loads(f.read())
    sites = np.asarray(m["sensor_lidar_site"]).reshape(-1)
    to32 = lambda v: np.asarray(v, np.float64).astype(np.float32).astype(np.float64)
    sp = to32(np.asarray(m["site_pos"]).reshape(-1, 3)[sites])
    lz = to32(np.asarray(m["k_site_mat"]).reshape(-1, 3, 3)[sites][:, :, 2])
    import occupancy_ref
    return occupancy_ref.ray_geometry(np.zeros(3), np.eye(3), sp, lz, np.zeros(3), np.eye(3))


def test_unsure_points_of_the_float_stage_cases_stay_under_the_cap():
    """A condition on the inputs of tests/test_gpu_scanmatch.py's float stage, met by the reference alone."""
    fs = ref.FLOAT_STAGE
    geom = _model_rays()
    assert geom[0].shape == (360, 2)
    scan, pts, mar = ref.float_stage_inputs([geom] * 3)
    assert np.isnan(scan).any() and (scan == -1).any() and ((scan >= 0) & (scan < fs.limits[0])).any() and (scan > fs.limits[1]).any()
    for nx, ny, (x0, y0) in fs.grids:
        pl = ref.place(pts, mar, fs.prior.T, fs.angles, x0, y0, fs.cell, nx, ny)
        share = ref.unsure_share(pl)
        print(f"{nx} x {ny}: counting rays {pl.n.tolist()}, unsure share {share.tolist()}, with a cell {int((pl.cell[..., 0] != ref.NO_CELL).sum())}")
        assert (share <= ref.MAX_AMBIGUOUS).all() and (pl.n >= 200).all()
        assert (pl.cell[..., 0] != ref.NO_CELL).sum() > 300      # not about empty tables: also the small grid holds points


@pytest.fixture(scope="module")
def room():
    """The map of the synthetic room: the hit cells of the three scans, its distance field, and the scans of all four poses."""
    g = ref.ROOM_GRID
    o, d, So, Sd = ref.unit_rays()
    poses = np.concatenate((ref.ROOM_POSES, ref.ROOM_EXTRA_POSE[None]))
    scans = [ref.room_scan(p, o, d) for p in poses]
    occ = ref.hit_cells(poses[:3], scans[:3], o, d, g, 0.2, 5.0)
    dist2 = torch.tensor(ref.dist2_of(occ))
    return dict(rays=(o, d, So, Sd), poses=poses, scans=scans, occ=occ, dist2=dist2)


@pytest.mark.parametrize("noise", [0.0, 0.01])
@pytest.mark.parametrize("sigma", [0.05, 0.10])
def test_recovery_in_a_synthetic_room(room, sigma, noise):
    """Sixteen priors (four poses by four offsets in lattice steps) per case; the winner lies within one lattice step of the truth
    in x, y and theta, and is the smallest index among the maxima of its volume."""
    g, W, step = ref.ROOM_GRID, ref.ROOM_WINDOW, ref.ROOM_STEP
    o, d, So, Sd = room["rays"]
    field1 = StatusStretchDistanceField(time=None, dist2=room["dist2"][None], nearest=None, origin=g.origin, cell=g.cell, frame="world").likelihood(sigma)[0].numpy()
    sa = scan_angles(window=2 * W * step, step=step)
    angles = sa.angles.numpy()
    assert len(angles) == 21
    rng = np.random.default_rng(3)
    cases = [(p, off) for p in range(4) for off in ref.ROOM_OFFSETS]
    pts, mar, prior = [], [], []
    for p, (ax, ay, at) in cases:
        r = room["scans"][p] + noise * rng.standard_normal(360)
        q, m, _ = ref.frame_points(o, d, So, Sd, r.astype(np.float32).astype(np.float64), 0.2, 5.0)
        pts.append(q)
        mar.append(m)
        prior.append(room["poses"][p] + np.array([ax * g.cell, ay * g.cell, at * step]))
    prior = np.array(prior, np.float32).T
    pl = ref.place(np.stack(pts), np.stack(mar), prior, angles, *g.origin, g.cell, g.nx, g.ny)
    field = np.broadcast_to(field1, (len(cases),) + field1.shape).copy()
    dec = ref.decide(pl.cell, field, prior, angles, g.cell, pl.n, wx=W, wy=W, min_points=30)
    assert (dec.status == ref.OK).all()
    k_of_row = np.round(angles / step).astype(int)
    worst, tied = 0, 0
    for b, (p, (ax, ay, at)) in enumerate(cases):
        t, dy, dx = ref.unindex(int(dec.best[b, 0]), W, W)
        err = (dx + ax, dy + ay, int(k_of_row[t]) + at)
        flat = dec.score[b].reshape(-1)
        maxima = np.flatnonzero(flat == flat.max())
        tied += len(maxima) > 1
        assert dec.best[b, 0] == maxima[0] and dec.best[b, 1] == flat.max(), (b, maxima[:4])      # the tie rule
        worst = max(worst, *(abs(v) for v in err))
        assert max(abs(v) for v in err) <= 1, (sigma, noise, p, (ax, ay, at), err)
    print(f"sigma {sigma} noise {noise}: worst error {worst} lattice steps, volumes with tied maxima {tied} of {len(cases)}")


def test_likelihood():
    d2 = torch.tensor([[[0, 1, 4], [9, 100, StatusStretchDistanceField.NONE]]], dtype=torch.int32)
    f = StatusStretchDistanceField(time=None, dist2=d2, nearest=None, origin=(0, 0), cell=0.05, frame="world")
    got = f.likelihood(0.10)
    want = [int(np.floor(255 * np.exp(-v * 0.05 ** 2 / (2 * 0.10 ** 2)) + 0.5)) for v in (0, 1, 4, 9, 100)] + [0]
    assert got.dtype == torch.uint8 and got.reshape(-1).tolist() == want and want[0] == 255 and want[1] == 225
    assert f.likelihood().equal(got)
    for bad in (0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            f.likelihood(bad)


def test_scan_angles():
    a = scan_angles()
    assert a.angles.dtype == torch.float32 and a.bias.dtype == torch.int32 and a.angles.shape == a.bias.shape == (21,)
    k = [0] + [s * j for j in range(1, 11) for s in (-1, 1)]
    assert a.angles.tolist() == [float(np.float32(j * 0.008727)) for j in k] and a.bias.tolist() == [0] * 21
    assert scan_angles(weight=7).bias.tolist() == [7 * abs(j) for j in k]
    assert scan_angles(window=0.0).angles.tolist() == [0.0]
    assert scan_angles(window=0.62, step=0.01).angles.shape == (63,)
    for kw in (dict(window=0.65, step=0.01), dict(step=0.0), dict(window=-1.0), dict(weight=-1), dict(window=float("nan")), dict(weight=1 << 20)):
        with pytest.raises(ValueError):
            scan_angles(**kw)


def _match(score, best, pose, angles, window, cell=0.05, **kw):
    return StatusStretchScanMatch(time=None, pose=pose, best=best, score=score, cells=None, angles=angles, window=window, origin=(0.0, 0.0), cell=cell,
                                  frame="world", **kw)


def test_offset_fit_and_refined_on_a_quadratic_volume():
    """J = 4000 - (4 dx - 5)^2 - (2 dy + 1)^2 - (8 a - 3)^2 with a the rotation in steps: integers, a separable quadratic whose
    maximum lies at dx = 1.25, dy = -0.5, a = 0.375; the parabola through the winner (1, 0 or -1, 0) and its neighbours finds it."""
    sa = scan_angles(window=0.06, step=0.01)                      # rows 0, -1, +1, -2, +2, -3, +3 steps
    k = np.round(sa.angles.numpy().astype(np.float64) / 0.01)
    wx, wy = 3, 2
    dx, dy = np.arange(-wx, wx + 1), np.arange(-wy, wy + 1)
    J = 4000 - (4 * dx[None, None, :] - 5) ** 2 - (2 * dy[None, :, None] + 1) ** 2 - (8 * k[:, None, None] - 3) ** 2
    score = torch.tensor(np.stack((J, J, J)).astype(np.int32))
    first = int(J.reshape(-1).argmax())
    t, wdy, wdx = ref.unindex(first, wx, wy)
    assert (wdx, k[t]) == (1, 0) and wdy in (-1, 0)
    best = torch.tensor([[first, int(J.max()), 100, 0], [-1, 0, 5, 1], [-1, 0, 100, 2]], dtype=torch.int32)
    prior = np.array([[0.3, -0.7, 0.2], [1.0, 2.0, 3.0], [np.nan, 0.0, 0.0]], np.float32).T
    pose = prior.copy()
    pose[:, 0] += np.array([wdx * 0.05, wdy * 0.05, sa.angles[t].item()], np.float32)
    m = _match(score, best, torch.tensor(pose), sa.angles, (wx, wy))
    assert m.ok().tolist() == [True, False, False] and m.status.tolist() == [0, 1, 2]
    assert m.offset().tolist() == [[wdx, wdy, t], [0, 0, 0], [0, 0, 0]]
    r = m.refined()
    assert r.dtype == torch.float32 and r.shape == (3, 3)
    want = np.array([0.3 + 1.25 * 0.05, -0.7 - 0.5 * 0.05, 0.2 + 0.375 * 0.01])
    assert np.abs(r[:, 0].numpy() - want).max() < 2e-7, (r[:, 0], want)
    assert r[:, 1:].numpy().tobytes() == pose[:, 1:].tobytes()      # not ok: the pose as it is
    # on the window's border the winner itself stays: with rotation 0 as the only row theta stays and x is still refined
    mb = _match(score[:, :1], torch.tensor([[ref.index(0, wdy, wdx, wx, wy), int(J.max()), 100, 0]] * 3, dtype=torch.int32), torch.tensor(pose),
                sa.angles[:1], (wx, wy))
    rb = mb.refined()
    assert rb[2, 0] == torch.tensor(pose)[2, 0] and abs(float(rb[0, 0]) - want[0]) < 2e-7
    # fit: S / (255 n) with the bias and the shift's weight taken out again
    mf = _match(None, torch.tensor([[first, 255 * 80 - 9 - 2 * (wdx ** 2 + wdy ** 2), 100, 0]], dtype=torch.int32), torch.zeros(3, 1), sa.angles, (wx, wy),
                bias=torch.full((7,), 9, dtype=torch.int32), shift_weight=2)
    assert abs(float(mf.fit()[0]) - 0.8) < 1e-6
    with pytest.raises(ValueError):
        mf.refined()
