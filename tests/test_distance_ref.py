"""tests/distance_ref.py itself: the brute-force reference of the distance field against scipy's exact Euclidean transform, closed
forms, the four-fold tie, and the obstacle predicate.  CPU only."""
import numpy as np
import pytest

import distance_ref as ref


def test_dist2_equals_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    for ny, nx, p in ((1, 1, 1.0), (1, 9, 0.3), (9, 1, 0.3), (12, 16, 0.05), (83, 61, 0.01), (83, 61, 0.3), (64, 64, 0.002), (40, 200, 0.02)):
        mask = rng.random((ny, nx)) < p
        if not mask.any():
            mask[ny // 2, nx // 3] = True
        d2, near = ref.field_of_mask(mask)
        for window in (0, 1, 3):      # the list alone, and windows that leave most cells to the list: the same arrays
            other = ref.field_of_mask(mask, window=window)
            assert np.array_equal(other[0], d2) and np.array_equal(other[1], near), (ny, nx, p, window)
        want = np.rint(ndi.distance_transform_edt(~mask) ** 2).astype(np.int64)
        assert np.array_equal(d2, want), (ny, nx, p)
        jy, jx = np.divmod(near, nx)
        yy, xx = np.mgrid[0:ny, 0:nx]
        assert mask[jy, jx].all() and np.array_equal((yy - jy) ** 2 + (xx - jx) ** 2, d2)      # nearest attains dist2, on an obstacle
        assert np.array_equal(d2 == 0, mask)


def test_one_obstacle_and_none():
    ny, nx = 23, 31
    yy, xx = np.mgrid[0:ny, 0:nx]
    for j, i in ((0, 0), (0, nx - 1), (ny - 1, 0), (ny - 1, nx - 1), (11, 7)):
        mask = np.zeros((ny, nx), bool)
        mask[j, i] = True
        d2, near = ref.field_of_mask(mask)
        assert np.array_equal(d2, (yy - j) ** 2 + (xx - i) ** 2) and (near == j * nx + i).all()
        d2r, nearr = ref.field_of_mask(mask, R=5)
        inside = (yy - j) ** 2 + (xx - i) ** 2 <= 25
        assert np.array_equal(d2r, np.where(inside, d2, ref.NONE)) and np.array_equal(nearr, np.where(inside, near, -1))
    d2, near = ref.field_of_mask(np.zeros((ny, nx), bool))
    assert (d2 == ref.NONE).all() and (near == -1).all() and ref.NONE == 1 << 30


def test_ties_go_to_the_smallest_index():
    for window in (0, 2, 8):
        d2, near = ref.field_of_mask(ref.tie_grid(9, 9), window=window)
        assert d2[4, 4] == 16 and near[4, 4] == 4
    board = np.indices((13, 11)).sum(0) % 2 == 1      # ties everywhere
    assert all(np.array_equal(a, b) for a, b in zip(ref.field_of_mask(board), ref.field_of_mask(board, window=0)))
    assert d2[4, 4] == 16 and near[4, 4] == 4      # top, left, right and bottom are all 4 away: the top one has index 4
    assert near[4, 3] == 36 and d2[4, 3] == 9      # one step left of the centre the left obstacle is nearer
    two = np.zeros((1, 5), bool)
    two[0, 0] = two[0, 4] = True
    assert ref.field_of_mask(two)[1].tolist() == [[0, 0, 0, 4, 4]]      # the middle cell takes the left one
    col = np.zeros((5, 1), bool)
    col[0, 0] = col[4, 0] = True
    assert ref.field_of_mask(col)[1][:, 0].tolist() == [0, 0, 0, 4, 4]
    # R exactly at a distance keeps it: dist2 > R^2 is strict
    assert ref.field_of_mask(ref.tie_grid(9, 9), R=4)[0][4, 4] == 16 and ref.field_of_mask(ref.tie_grid(9, 9), R=3)[0][4, 4] == ref.NONE


def test_predicate():
    rng = np.random.default_rng(9)
    hit, miss = rng.integers(0, 6, (2, 7, 9)), rng.integers(0, 3, (2, 7, 9))
    hit[0, :3] = 0
    m1 = ref.obstacle_mask(hit, miss, 1, False)
    assert np.array_equal(m1, hit >= 1) and np.array_equal(ref.obstacle_mask(hit, None, 1, True), m1)      # no miss layer: nothing is "unknown"
    m3 = ref.obstacle_mask(hit, miss, 3, False)
    assert np.array_equal(m3 != m1, (hit >= 1) & (hit < 3)) and (m3 != m1).any()
    mu = ref.obstacle_mask(hit, miss, 3, True)
    assert np.array_equal(mu != m3, (hit == 0) & (miss == 0)) and (mu != m3).any()
    d2, near = ref.field(hit, miss, 3, True, R=2)
    assert d2.shape == near.shape == (2, 7, 9) and d2.dtype == near.dtype == np.int32
    assert np.array_equal(d2 == 0, mu)
