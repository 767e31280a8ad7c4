"""The height-map reference (tests/height_map_ref.py) checked by itself, on the CPU: against a brute-force loop on a synthetic
scene (a floor and two walls seen from a pitched, yawed camera, base frame yawed 0.37 rad), the consistency of its bounds, and the
condition that keeps the comparison rule from hiding a failure -- at most 1 % ambiguous points -- for the parameters the GPU test
uses (cells 0.05 and 0.0625 m, origins that are not round numbers, a z band that does not start on the floor)."""
import math

import numpy as np
import pytest

import height_map_ref as ref
from point_cloud_ref import deproject, pixel_dirs

X0, Y0 = -1.613, -1.587
SMALL_ORIGIN = (0.487, -0.313)   # the 16 x 12 grid (0.8 m x 0.6 m) sits in front of the camera


def _origin(ny, nx):
    return SMALL_ORIGIN if (ny, nx) == (12, 16) else (X0, Y0)

CASES = [((37, 23), 1, 0.05, (12, 16)), ((37, 23), 1, 0.05, (64, 64)), ((424, 240), 1, 0.05, (64, 64)), ((480, 270), 3, 0.0625, (64, 64)),
         ((424, 240), 3, 0.05, (12, 16)), ((37, 23), 3, 0.0625, (96, 64))]


def _scene(W, H, stride, frame):
    depth, cp, cm, bp, bm = ref.synthetic_scene(W, H)
    pts = deproject(depth, W, H, 58.0, stride, cp, cm, frame, bp, bm)
    xn, yn = pixel_dirs(W, H, 58.0, stride)
    S = np.abs(depth[::stride, ::stride].astype(np.float64)) * (np.abs(xn) + np.abs(yn) + 1) + np.abs(cp).sum()
    if frame == "body":
        S = S + np.abs(bp).sum()
    return depth, pts, S


def _brute(pts, S, x0, y0, cell, nx, ny, z_lo, z_hi):
    n_lo, n_hi = np.zeros((ny, nx), np.int64), np.zeros((ny, nx), np.int64)
    zl, zh, mz = np.full((ny, nx), -np.inf), np.full((ny, nx), -np.inf), np.zeros((ny, nx))
    valid = amb = 0
    for (x, y, z), s in zip(pts.reshape(-1, 3), S.reshape(-1)):
        if math.isnan(x):
            continue
        valid += 1
        m = ref.EPS * s + 2.0 ** -22 * (abs(x - x0) + abs(y - y0))
        cells = set()
        outside = False
        for xx in (x - m, x + m):      # a box smaller than a cell meets exactly the cells of its corners
            for yy in (y - m, y + m):
                ix, iy = math.floor((xx - x0) / cell), math.floor((yy - y0) / cell)
                if 0 <= ix < nx and 0 <= iy < ny:
                    cells.add((iy, ix))
                else:
                    outside = True
        assert 2 * m < cell
        if z + m < z_lo or z - m > z_hi or not cells:
            continue
        crosses = not (z - m >= z_lo and z + m <= z_hi)
        if len(cells) == 1 and not outside and not crosses:
            c = next(iter(cells))
            n_lo[c] += 1
            zl[c] = max(zl[c], z)
        else:
            amb += 1
        for c in cells:
            n_hi[c] += 1
            zh[c] = max(zh[c], z)
            mz[c] = max(mz[c], m)
    return n_lo, n_hi, zl, zh, mz, valid, amb


@pytest.mark.parametrize("frame", ["world", "body"])
def test_reference_against_brute_force(frame):
    (W, H), stride, cell, (ny, nx) = CASES[0]
    for z_band in ((-0.05, 1.0), (-math.inf, math.inf)):
        _, pts, S = _scene(W, H, stride, frame)
        bd = ref.bounds(pts, S, *_origin(ny, nx), cell, nx, ny, *z_band)
        n_lo, n_hi, zl, zh, mz, valid, amb = _brute(pts, S, *_origin(ny, nx), cell, nx, ny, *z_band)
        assert valid == bd.valid > 500 and amb == bd.ambiguous
        assert np.array_equal(n_lo, bd.n_lo) and np.array_equal(n_hi, bd.n_hi)
        assert np.array_equal(zl, bd.z_lo) and np.array_equal(zh, bd.z_hi) and np.array_equal(mz, bd.m_z)
        assert 0 < bd.n_lo.sum() < bd.valid       # the small grid does not hold the whole scene: points drop out at its edge


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-s{c[1]}-c{c[2]}-{c[3][0]}x{c[3][1]}")
def test_ambiguous_share_and_consistency(case):
    (W, H), stride, cell, (ny, nx) = case
    for frame in ("world", "body"):
        _, pts, S = _scene(W, H, stride, frame)
        bd = ref.bounds(pts, S, *_origin(ny, nx), cell, nx, ny, -0.05, 1.0)
        share = ref.ambiguous_share(bd)
        print(case, frame, "valid", bd.valid, "sure", bd.sure, "ambiguous", bd.ambiguous, "share %.4f %%" % (100 * share))
        assert bd.valid > 0.5 * pts.shape[0] * pts.shape[1] and bd.sure > 0
        assert share <= ref.MAX_AMBIGUOUS
        assert (bd.n_lo <= bd.n_hi).all() and (bd.z_lo <= bd.z_hi).all() and bd.n_lo.sum() <= bd.valid
        assert bd.n_lo.sum() == bd.sure and bd.n_hi.sum() >= bd.sure + bd.ambiguous   # every ambiguous point has a candidate cell
        assert np.isneginf(bd.z_lo[bd.n_lo == 0]).all() and np.isfinite(bd.z_lo[bd.n_lo > 0]).all()


def test_comparison_rule_catches_what_it_should():
    (W, H), stride, cell, (ny, nx) = CASES[0]
    _, pts, S = _scene(W, H, stride, "world")
    bd = ref.bounds(pts, S, *_origin(ny, nx), cell, nx, ny, -0.05, 1.0)
    count = bd.n_lo.copy()
    height = np.where(count > 0, bd.z_lo, np.nan).astype(np.float32)
    assert ref.check_map(height, count, bd) == []
    iy, ix = np.argwhere(count > 0)[0]
    for dh, dc in ((1e-3, 0), (-1e-3, 0), (0, int(bd.n_hi[iy, ix] - bd.n_lo[iy, ix]) + 1), (0, -1), (np.nan, 0)):
        h2, c2 = height.copy(), count.copy()
        h2[iy, ix] += np.float32(dh)
        c2[iy, ix] += dc
        assert ref.check_map(h2, c2, bd), (dh, dc)
    iy, ix = np.argwhere(bd.n_hi == 0)[0]
    h2 = height.copy()
    h2[iy, ix] = 0.0
    assert ref.check_map(h2, count, bd)
    two = ref.merge(bd, bd)
    assert ref.check_map(height, 2 * count, two) == [] and ref.check_map(height, count, two)
