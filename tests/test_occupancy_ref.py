"""The occupancy reference (tests/occupancy_ref.py) checked by itself, on the CPU: on a synthetic room (a rectangle of walls around a
yawed, offset laser) wall cells are hit, cells between the laser and a wall are missed and never hit, cells behind a wall are
untouched; the closed-form line equals a long-hand iterative Bresenham and visits no cell twice; the classification table; and the
condition that keeps the comparison rule from hiding a failure: at most 2 % ambiguous rays with an origin chosen on a lattice."""
import numpy as np
import pytest

import occupancy_ref as ref

CELL = 0.05


def _room(frame):
    bp, bm, sp, lz, ranges, walls = ref.synthetic_room()
    fp, fm = (bp, bm) if frame == "body" else (None, None)
    return ref.ray_geometry(bp, bm, sp, lz, fp, fm), ranges, walls, (bp, bm)


def _origin(geom, ranges, nx, ny, r_max, clears, base=(-3.2, -3.2)):
    got = ref.choose_origin([(base[0] - j / 1024, base[1] - j / 1024) for j in range(64)], [(*geom, ranges)], CELL, nx, ny, 0.2, r_max, clears)
    if got is None:
        pytest.fail("no candidate origin keeps the laser off the cell edges and the ambiguous rays within 2 %")
    return got[0], got[1][0]


def test_closed_form_line_equals_iterative_bresenham_and_visits_no_cell_twice():
    for dx in range(-40, 41):
        for dy in range(-40, 41):
            ax, ay = 7, -3
            xs, ys = ref.line_cells(ax, ay, ax + dx, ay + dy)
            cells = list(zip(xs.tolist(), ys.tolist()))
            assert cells == ref.bresenham(ax, ay, ax + dx, ay + dy), (dx, dy)
            assert len(set(cells)) == len(cells) == max(abs(dx), abs(dy)) + 1
            assert cells[0] == (ax, ay) and cells[-1] == (ax + dx, ay + dy)
            steps = np.abs(np.diff(xs)) + np.abs(np.diff(ys))
            assert ((steps >= 1) & (np.abs(np.diff(xs)) <= 1) & (np.abs(np.diff(ys)) <= 1)).all()      # 8-connected


def test_classification_table():
    nan, inf = float("nan"), float("inf")
    r = np.array([nan, 0.0, -0.0, 0.1, 0.19999, 0.2, 1.0, 5.0, 5.0001, inf, -1.0, -inf, -1e-30], np.float32)
    kind, length = ref.classify(r, float(np.float32(0.2)), 5.0, True)
    D, R, C = ref.DROP, ref.RETURN, ref.CLEAR
    assert kind.tolist() == [D, D, D, D, D, R, R, R, C, C, C, C, C]
    assert length[5:8].tolist() == [float(r[5]), 1.0, 5.0] and (length[8:] == 5.0).all()
    kind, _ = ref.classify(r, float(np.float32(0.2)), 5.0, False)
    assert kind.tolist() == [D, D, D, D, D, R, R, R, D, D, D, D, D]
    kind, _ = ref.classify(np.array([0.0, -0.0], np.float32), 0.0, 5.0, False)      # r_min = 0: a zero range is a return
    assert kind.tolist() == [R, R]


@pytest.mark.parametrize("frame", ["world", "body"])
def test_room_walls_are_hit_free_space_is_missed_behind_the_walls_nothing(frame):
    (o, d, So, Sd), ranges, walls, (bp, bm) = _room(frame)
    nx = ny = 160      # 8 m x 8 m: holds the whole room
    (x0, y0), bd = _origin((o, d, So, Sd), ranges, nx, ny, 9.5, True, base=(-4.0, -4.0))
    print(frame, "origin", x0, y0, "rays", bd.rays, "sure", bd.sure, "ambiguous", bd.ambiguous, "returns", bd.returns)
    assert bd.returns == 360 and bd.dropped == 0 and bd.ambiguous <= 7
    assert (bd.hit_lo <= bd.hit_hi).all() and (bd.miss_lo <= bd.miss_hi).all()
    assert bd.hit_lo.sum() == bd.sure and bd.hit_hi.sum() >= bd.sure + bd.ambiguous
    # cell centres in the world frame
    cx, cy = np.meshgrid(x0 + (np.arange(nx) + 0.5) * CELL, y0 + (np.arange(ny) + 0.5) * CELL)
    if frame == "body":
        w = np.stack([cx, cy, np.zeros_like(cx)], -1) @ bm.T + bp
        cx, cy = w[..., 0], w[..., 1]
    xl, xh, yl, yh = walls
    depth_in = np.minimum(np.minimum(cx - xl, xh - cx), np.minimum(cy - yl, yh - cy))      # > 0 inside the room, < 0 outside
    diag = CELL * 0.7072 + 1e-4
    # every hit lies on a wall, every miss inside the room; a cell that is hit is not free, a free cell well inside is never hit
    assert (np.abs(depth_in[bd.hit_hi > 0]) <= diag).all()
    assert (depth_in[bd.miss_hi > 0] >= -diag).all()
    assert ((bd.hit_hi > 0) & (depth_in > 2 * diag)).sum() == 0
    # cells behind a wall are untouched
    behind = depth_in < -diag
    assert behind.sum() > 1000 and (bd.hit_hi[behind] == 0).all() and (bd.miss_hi[behind] == 0).all()
    # the walls are seen all around: hit cells on all four sides, and the cell of the laser is missed by every sure ray
    for side in (np.abs(cx - xl), np.abs(cx - xh), np.abs(cy - yl), np.abs(cy - yh)):
        assert ((bd.hit_lo > 0) & (side <= diag)).sum() > 10
    lx, ly = int(np.floor((o[0, 0] - x0) / CELL)), int(np.floor((o[0, 1] - y0) / CELL))
    assert bd.miss_lo[ly, lx] == bd.sure and bd.hit_hi[ly, lx] == 0
    # the open interior within 1 m of the laser is dense with rays: every cell missed
    ow = np.stack([o[0, 0], o[0, 1]]) if frame == "world" else (np.array([o[0, 0], o[0, 1], 0.0]) @ bm.T + bp)[:2]
    near = (cx - ow[0]) ** 2 + (cy - ow[1]) ** 2 < 1.0
    assert (bd.miss_lo[near] > 0).all()


@pytest.mark.parametrize("r_max,clears", [(9.5, 1), (2.0, 1), (2.0, 0), (9.5, 0)])
def test_ambiguous_share_and_consistency_for_the_grids_of_the_gpu_test(r_max, clears):
    for frame in ("world", "body"):
        geom, ranges, _, _ = _room(frame)
        for (nx, ny), base in (((16, 12), (0.1, -0.5)), ((64, 64), (-1.6, -1.6)), ((61, 83), (-1.5, -2.1)), ((64, 96), (-1.6, -2.4))):
            (x0, y0), bd = _origin(geom, ranges, nx, ny, r_max, clears, base)
            print(frame, (nx, ny), r_max, clears, "origin", x0, y0, "sure", bd.sure, "ambiguous", bd.ambiguous, "returns", bd.returns, "clears", bd.clears)
            assert ref.ambiguous_share(bd) <= ref.MAX_AMBIGUOUS
            assert bd.sure + bd.ambiguous + bd.dropped == bd.rays == 360
            assert (bd.hit_lo <= bd.hit_hi).all() and (bd.miss_lo <= bd.miss_hi).all()
            assert int(bd.hit_hi.max()) <= 360 and int((bd.hit_hi + bd.miss_hi).max()) <= 360 + bd.ambiguous
            if not clears and r_max == 2.0:
                assert bd.dropped > 0 and bd.clears == 0
            if clears:
                assert bd.dropped == 0


def test_comparison_rule_catches_what_it_should():
    geom, ranges, _, _ = _room("world")
    (x0, y0), bd = _origin(geom, ranges, 64, 64, 9.5, True, (-1.6, -1.6))
    hit, miss = bd.hit_lo.copy(), bd.miss_lo.copy()
    assert ref.check_grid(hit, miss, bd) == []
    iy, ix = np.argwhere(bd.miss_lo > 0)[0]
    for layer, delta in (("miss", int(bd.miss_hi[iy, ix] - bd.miss_lo[iy, ix]) + 1), ("miss", -1), ("hit", int(bd.hit_hi[iy, ix] - bd.hit_lo[iy, ix]) + 1)):
        h2, m2 = hit.copy(), miss.copy()
        (h2 if layer == "hit" else m2)[iy, ix] += delta
        assert ref.check_grid(h2, m2, bd), (layer, delta)
    two = ref.merge(bd, bd)
    assert ref.check_grid(2 * hit, 2 * miss, two) == [] and ref.check_grid(hit, miss, two)
