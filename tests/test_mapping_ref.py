"""The numpy reference of smj_scan_to_map (tests/mapping_ref.py) on the CPU: its exact stage against a second, long-hand loop, the cap
on unsure rays for the float-stage cases the GPU tests use, and the closed loop -- match, integrate, distance field, match again --
in the synthetic room of tests/scanmatch_ref.py, against a map made by dead reckoning."""
import numpy as np
import torch

import mapping_ref as ref
import occupancy_ref
import scanmatch_ref
from stretch_mujoco_amd.datamodels import StatusStretchDistanceField
from stretch_mujoco_amd.utils import scan_angles
from test_scanmatch_ref import _model_rays


def _longhand(cells, kind, pose, gate, nx, ny, hit, miss, accumulate):
    """integrate() once more: one env, one ray and one Bresenham step at a time."""
    B, K, _ = cells.shape
    h = hit.astype(np.int64).copy() if accumulate else np.zeros((B, ny, nx), np.int64)
    m = miss.astype(np.int64).copy() if accumulate else np.zeros((B, ny, nx), np.int64)
    info = np.zeros((B, 4), np.int64)
    for e in range(B):
        if not all(np.isfinite(float(v)) for v in pose[:, e]):
            info[e, 0] = ref.OFF
            continue
        if gate is not None and gate[e] != 0:
            info[e, 0] = ref.GATED
            continue
        for k in range(K):
            if kind[e, k] == ref.DROP:
                continue
            if cells[e, k, 0] == ref.NO_CELL:
                info[e, 3] += 1
                continue
            info[e, 1 if kind[e, k] == ref.RETURN else 2] += 1
            line = occupancy_ref.bresenham(*(int(v) for v in cells[e, k]))
            for i, (x, y) in enumerate(line):
                if 0 <= x < nx and 0 <= y < ny:
                    if kind[e, k] == ref.RETURN and i == len(line) - 1:
                        h[e, y, x] += 1
                    else:
                        m[e, y, x] += 1
    return h, m, info


def test_integrate_equals_a_long_hand_loop():
    rng = np.random.default_rng(17)
    B, K, nx, ny = 4, 60, 23, 17
    a = np.stack((rng.integers(-6, nx + 6, (B, K)), rng.integers(-6, ny + 6, (B, K))), -1)
    b = a + np.stack((rng.integers(-12, 13, (B, K)), rng.integers(-12, 13, (B, K))), -1)
    b[:, :5] = a[:, :5]                                        # n = 0
    cells = np.concatenate((a, b), -1)
    kind = rng.integers(0, 3, (B, K))
    guarded = (rng.random((B, K)) < 0.1) | (kind == ref.DROP)
    cells[guarded] = ref.NO_CELL
    pose = np.array([[0.1, -0.2, 0.3], [0.0, np.nan, 0.0], [1.0, 2.0, 3.0], [0.5, 0.5, np.inf]], np.float32).T
    hit0, miss0 = rng.integers(0, 9, (B, ny, nx)).astype(np.int32), rng.integers(0, 9, (B, ny, nx)).astype(np.int32)
    for gate in (None, np.array([0, 1, -7, 0])):
        status = ref.status_of(pose, gate)
        assert status.tolist() == ([ref.OK, ref.OFF, ref.OK, ref.OFF] if gate is None else [ref.OK, ref.OFF, ref.GATED, ref.OFF])      # the pose comes before the gate
        for accumulate in (False, True):
            h, m, info = ref.integrate(cells, kind, status, nx, ny, hit0, miss0, accumulate)
            wh, wm, winfo = _longhand(cells, kind, pose, gate, nx, ny, hit0, miss0, accumulate)
            assert np.array_equal(h, wh) and np.array_equal(m, wm) and np.array_equal(info, winfo), (gate, accumulate)
            for e in np.nonzero(status != ref.OK)[0]:      # keeps its bits, or is zeroed
                assert np.array_equal(h[e], hit0[e] if accumulate else 0 * hit0[e]) and info[e, 1:].tolist() == [0, 0, 0]
            assert info[0, 1] > 5 and info[0, 2] > 5 and info[0, 3] > 0 and h[0].sum() - (hit0[0].sum() if accumulate else 0) > 3


def test_unsure_rays_of_the_float_stage_cases_stay_under_the_cap():
    """A condition on the inputs of tests/test_gpu_mapping.py's float stage, met by the reference alone: every laser origin is sure
    and the unsure rays stay within 2 % per env, clearing rays included."""
    fs = scanmatch_ref.FLOAT_STAGE
    geom = _model_rays()
    scan, _, _ = scanmatch_ref.float_stage_inputs([geom] * 3)
    for nx, ny, (x0, y0) in fs.grids:
        for poses in (fs.prior, fs.truth):
            for nrc in (0, 1):
                for e in range(3):
                    pl = ref.place_rays(*geom, scan[:, e].astype(np.float64), poses[e], x0, y0, fs.cell, *fs.limits, nrc)
                    unsure = int((~pl.sure).sum())
                    print(f"{nx} x {ny} clears {nrc} env {e}: kept {int(pl.kept.sum())} of 360, returns {int((pl.kind == ref.RETURN).sum())}, unsure {unsure}")
                    assert pl.origin_sure.all(), (nx, ny, e)
                    assert ref.unsure_share(pl) <= ref.MAX_AMBIGUOUS, (nx, ny, nrc, e, unsure)
                    assert (pl.kind == ref.RETURN).sum() >= 200 and pl.kept.sum() >= 200 + 30 * nrc
                    assert pl.kept[pl.kind != ref.DROP].all()      # no guard is near on these grids


def _closed_loop(rays=None, bias=ref.LOOP_BIAS):
    """The loop on the CPU, with the references alone.  Returns the per-step statuses and lattice errors and the three maps."""
    g, W, step = scanmatch_ref.ROOM_GRID, scanmatch_ref.ROOM_WINDOW, scanmatch_ref.ROOM_STEP
    o, d, So, Sd = scanmatch_ref.unit_rays() if rays is None else rays
    angles = scan_angles(window=2 * W * step, step=step).angles.numpy()
    assert len(angles) == 21
    truth = ref.LOOP_POSES
    scans = [scanmatch_ref.room_scan(p, o, d).astype(np.float32).astype(np.float64) for p in truth]

    def add(maps, pose, scan):
        pl = ref.place_rays(o, d, So, Sd, scan, pose, *g.origin, g.cell, *ref.LOOP_LIMITS, 1)
        h, m, info = ref.integrate(pl.cell[None], pl.kind[None], ref.status_of(np.asarray(pose, np.float32)[:, None]), g.nx, g.ny, maps[0], maps[1], True)
        assert info[0, 0] == ref.OK and info[0, 1] > 200
        return h, m

    zeros = lambda: (np.zeros((1, g.ny, g.nx), np.int32), np.zeros((1, g.ny, g.nx), np.int32))
    loop = add(zeros(), truth[0], scans[0])
    dead = add(zeros(), truth[0], scans[0])
    true_map = add(zeros(), truth[0], scans[0])
    est, dr = truth[0].astype(np.float32), truth[0].copy()
    statuses, errors = [], []
    for i in range(1, len(truth)):
        inc = truth[i] - truth[i - 1] + bias
        prior = (est.astype(np.float64) + inc).astype(np.float32)[:, None]
        dr = dr + inc
        dist2 = torch.tensor(scanmatch_ref.dist2_of(loop[0][0] > 0))[None]
        field = StatusStretchDistanceField(time=None, dist2=dist2, nearest=None, origin=g.origin, cell=g.cell, frame="world").likelihood(ref.LOOP_SIGMA).numpy()
        pts, mar, _ = scanmatch_ref.frame_points(o, d, So, Sd, scans[i], *ref.LOOP_LIMITS)
        pl = scanmatch_ref.place(pts[None], mar[None], prior, angles, *g.origin, g.cell, g.nx, g.ny)
        dec = scanmatch_ref.decide(pl.cell, field, prior, angles, g.cell, pl.n, wx=W, wy=W, min_points=30)
        statuses.append(int(dec.status[0]))
        est = dec.pose[:, 0]
        errors.append(ref.lattice_error(est, truth[i], g.cell, step))
        loop = add(loop, est, scans[i])
        dead = add(dead, dr.astype(np.float32), scans[i])
        true_map = add(true_map, truth[i], scans[i])
    dr_error = ref.lattice_error(dr, truth[-1], g.cell, step)
    return statuses, np.array(errors), dr_error, loop, dead, true_map


def test_the_loop_closes_in_a_synthetic_room():
    """Match, integrate at the winner, distance field of hit > 0, likelihood, match again: every step's pose stays within one lattice
    step of the truth, and the map so made lies on the map made at the true poses, where the map made by dead reckoning does not."""
    statuses, errors, dr_error, loop, dead, true_map = _closed_loop()
    truth_dist2 = scanmatch_ref.dist2_of(true_map[0][0] > 0)
    worst_loop, worst_dead = ref.worst_dist2(loop[0][0], truth_dist2), ref.worst_dist2(dead[0][0], truth_dist2)
    print(f"errors per step in lattice steps {np.round(errors, 2).tolist()}, dead reckoning ends {np.round(dr_error, 1).tolist()} off; "
          f"worst squared distance to the truth-pose map: loop {worst_loop}, dead reckoning {worst_dead}")
    assert statuses == [scanmatch_ref.OK] * 7
    assert ref.within_one_step(errors), errors
    assert worst_loop <= ref.LOOP_MAX_DIST2
    assert worst_dead > ref.LOOP_DEAD_RECKONING
