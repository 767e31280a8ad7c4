"""tests/drive_ref.py, the numpy reference of smj_navigation_to_velocity, on hand-made grids where the answer is read off; and the
cap on unsure points for exactly the poses and tables tests/test_gpu_drive.py places.  CPU only."""
import numpy as np

import drive_ref as ref

NONE = ref.NAV_NONE
# A 5 x 5 grid of unit cells, origin (0, 0).  Three candidates from a robot at the centre of cell (2, 2) facing +x: straight ahead,
# up-left, down-right; one swept point and one scoring point each, all at cell centres.
POSE = np.array([[2.5], [2.5], [0.0]], np.float32)
POINTS = np.array([[[1.0, 0.0], [2.0, 0.0]], [[1.0, 1.0], [2.0, 2.0]], [[1.0, -1.0], [2.0, -2.0]]], np.float32)
COMMAND = np.array([[0.25, 0.0], [0.16, 0.5], [0.16, -0.5]], np.float32)


def _cells(pose=POSE, points=POINTS, n=5):
    pl = ref.place(pose, points, 0.0, 0.0, 1.0, n, n)
    assert pl.sure.all()
    return pl.cell


def _own(pose=POSE, n=5):
    return ref.place(pose, np.zeros((1, 1, 2), np.float32), 0.0, 0.0, 1.0, n, n).cell[:, 0, 0]


def _potential():
    """Distance to column 4 in steps of 500: the goal is the right edge."""
    return np.tile(((4 - np.arange(5)) * 500).astype(np.int32), (1, 5, 1))


def test_place_reads_off():
    cells = _cells()
    assert cells[0].tolist() == [[2 * 5 + 3, 2 * 5 + 4], [3 * 5 + 3, 4 * 5 + 4], [1 * 5 + 3, 0 * 5 + 4]] and _own().tolist() == [12]
    quarter = np.array([[2.5], [2.5], [np.pi / 2]], np.float32)      # facing +y: forward is up, left is -x
    assert _cells(quarter)[0].tolist() == [[3 * 5 + 2, 4 * 5 + 2], [3 * 5 + 1, 4 * 5 + 0], [3 * 5 + 3, 4 * 5 + 4]]
    far = ref.place(POSE, np.array([[[2.4, 0.0], [2.6, 0.0], [-2.6, 0.0], [0.0, 2.6]]], np.float32), 0.0, 0.0, 1.0, 5, 5)
    assert far.cell[0, 0].tolist() == [14, -1, -1, -1] and far.sure.all()
    edge = ref.place(POSE, np.array([[[0.5, 0.0], [0.5, 0.5], [0.4999, 0.0]]], np.float32), 0.0, 0.0, 1.0, 5, 5)      # on an edge, on a corner, beside it
    assert edge.sure[0, 0].tolist() == [False, False, True] and sorted(set(edge.cand[0, 0, 0].tolist())) == [12, 13]
    assert sorted(set(edge.cand[0, 0, 1].tolist())) == [12, 13, 17, 18] and edge.cell[0, 0, 2] == 12
    assert ref.check_cells([[[12, 18, 12]]], edge) == [] and ref.check_cells([[[13, 12, 12]]], edge) == []
    assert [v[:4] for v in ref.check_cells([[[14, 12, 13]]], edge)] == [(0, 0, 0, 14), (0, 0, 2, 13)]
    rim = ref.place(np.array([[5.0], [2.5], [0.0]], np.float32), np.zeros((1, 1, 2), np.float32), 0.0, 0.0, 1.0, 5, 5)      # on the grid's edge: inside or outside
    assert not rim.sure.any() and sorted(set(rim.cand[0, 0, 0].tolist())) == [-1, 14]
    zero = ref.place(np.array([[0.0], [2.5], [0.0]], np.float32), np.zeros((1, 1, 2), np.float32), 0.0, 0.0, 1.0, 5, 5)      # all terms zero: exact in fp32 too
    assert zero.sure.all() and zero.cell.tolist() == [[[10]]]
    assert 0 < far.margin.max() < 2e-5 and ref.unsure_share(edge).tolist() == [2 / 3]


def test_nan_pose_is_outside_and_off_grid():
    for bad in ([np.nan, 2.5, 0.0], [2.5, np.inf, 0.0], [2.5, 2.5, np.nan]):
        pose = np.array(bad, np.float32).reshape(3, 1)
        pl = ref.place(pose, POINTS, 0.0, 0.0, 1.0, 5, 5)
        assert (pl.cell == -1).all() and pl.sure.all()
        own = _own(pose)
        d = ref.decide(pl.cell, None, _potential(), COMMAND, own=own, pose_finite=np.isfinite(pose).all(0))
        assert own.tolist() == [-1] and d.status.tolist() == [ref.OFF_GRID] and d.chosen.tolist() == [-1] and d.cmd.tolist() == [[0.0], [0.0]]
        assert (d.score == ref.NO_SCORE).all()
    # a finite pose off the grid: the candidates are still evaluated
    pose = np.array([[-0.5], [2.5], [0.0]], np.float32)
    d = ref.decide(_cells(pose), None, _potential(), COMMAND, own=_own(pose))
    assert d.status.tolist() == [ref.OFF_GRID] and d.score[0, 0] == 1500 and d.cmd.tolist() == [[0.0], [0.0]]


def test_a_wall_blocks_all_but_one_arc():
    cost = np.zeros((1, 5, 5), np.uint8)
    cost[0, 2:, 3] = 254      # a wall in column 3 from row 2 up: straight ahead and up-left touch it
    d = ref.decide(_cells(), cost, _potential(), COMMAND, own=_own())
    assert d.score.tolist() == [[ref.NO_SCORE, ref.NO_SCORE, 0]] and d.best.tolist() == [[2, ref.OK]]
    assert d.cmd.tobytes() == COMMAND[2].reshape(2, 1).tobytes()
    cost[0, 1, 3] = 253      # the last one too
    d = ref.decide(_cells(), cost, _potential(), COMMAND, own=_own())
    assert d.best.tolist() == [[-1, ref.BLOCKED]] and d.cmd.tolist() == [[0.0], [0.0]]
    d = ref.decide(_cells(), cost, _potential(), COMMAND, own=_own(), lethal=254)      # 253 passes now and costs 20 * 253
    assert d.score.tolist() == [[ref.NO_SCORE, ref.NO_SCORE, 20 * 253]] and d.best.tolist() == [[2, ref.OK]]
    d = ref.decide(_cells(), cost, _potential(), COMMAND, own=_own(), lethal=254, obstacle_weight=0, goal_weight=3, bias=[0, 0, -7])
    assert d.score[0, 2] == -7


def test_a_tie_goes_to_the_smallest_k():
    d = ref.decide(_cells(), None, _potential(), COMMAND, own=_own())
    assert d.score.tolist() == [[0, 0, 0]] and d.best.tolist() == [[0, ref.OK]]
    d = ref.decide(_cells(), None, _potential(), COMMAND, own=_own(), bias=[1, 0, 0])
    assert d.best.tolist() == [[1, ref.OK]]
    d = ref.decide(_cells(), None, _potential(), COMMAND, own=_own(), bias=[1, 0, -1])
    assert d.best.tolist() == [[2, ref.OK]]
    cost = np.zeros((1, 5, 5), np.uint8)
    cost[0, 2, 3] = 25      # 20 * 25 on the straight arc = one cell of path
    pot = _potential()
    pot[0, :, 4] = [500, 500, 0, 500, 500]
    d = ref.decide(_cells(), cost, pot, COMMAND, own=_own())
    assert d.score.tolist() == [[500, 500, 500]] and d.chosen.tolist() == [0]


def test_a_window_that_leaves_one_candidate_and_a_nan_twist():
    kw = dict(own=_own(), max_dv=0.05, max_dw=0.25)
    d = ref.decide(_cells(), None, _potential(), COMMAND, twist=np.array([[0.16], [0.5]], np.float32), **kw)
    assert d.score.tolist() == [[ref.NO_SCORE, 0, ref.NO_SCORE]] and d.best.tolist() == [[1, ref.OK]]
    d = ref.decide(_cells(), None, _potential(), COMMAND, twist=np.array([[0.25], [0.25]], np.float32), own=_own(), max_dv=0.0, max_dw=0.25)
    assert d.score.tolist() == [[0, ref.NO_SCORE, ref.NO_SCORE]]      # <= holds with equality: 0 <= 0 and 0.25 <= 0.25, exact in fp32
    d = ref.decide(_cells(), None, _potential(), COMMAND, twist=np.array([[0.25], [0.25]], np.float32), own=_own(), max_dv=0.0, max_dw=np.nextafter(np.float32(0.25), np.float32(0)))
    assert (d.score == ref.NO_SCORE).all()
    for tw in ([np.nan, 0.0], [0.16, np.nan]):
        d = ref.decide(_cells(), None, _potential(), COMMAND, twist=np.array(tw, np.float32).reshape(2, 1), own=_own())      # infinite limits, still blocked
        assert (d.score == ref.NO_SCORE).all() and d.best.tolist() == [[-1, ref.BLOCKED]]
    d = ref.decide(_cells(), None, _potential(), COMMAND, twist=np.array([[9.0], [-9.0]], np.float32), own=_own())
    assert d.score.tolist() == [[0, 0, 0]]


def test_arrive_potential_at_its_boundary():
    pot = _potential()      # 1000 at the own cell
    for arrive, status in ((999, ref.OK), (1000, ref.ARRIVED), (1001, ref.ARRIVED)):
        d = ref.decide(_cells(), None, pot, COMMAND, own=_own(), arrive_potential=arrive)
        assert d.status.tolist() == [status] and d.score.tolist() == [[0, 0, 0]] and (d.chosen.tolist() == [0]) == (status == ref.OK)
    pot[0, 2, 2] = NONE      # no path from here, but candidates that end where there is one
    d = ref.decide(_cells(), None, pot, COMMAND, own=_own(), arrive_potential=NONE - 1)
    assert d.best.tolist() == [[0, ref.OK]]


def test_outside_is_free_both_ways():
    pose = np.array([[3.5], [0.5], [0.0]], np.float32)      # bottom row, facing the right edge; scoring points one cell ahead
    points = np.array([[[0.0, -1.0], [1.0, 0.0]], [[0.0, 1.0], [1.0, 0.0]], [[0.0, 1.0], [2.0, 0.0]]], np.float32)
    cells = _cells(pose, points)
    assert cells[0].tolist() == [[-1, 4], [8, 4], [8, -1]]
    cost = np.full((1, 5, 5), 7, np.uint8)
    command = COMMAND
    d = ref.decide(cells, cost, _potential(), command, own=_own(pose))
    assert d.score.tolist() == [[ref.NO_SCORE, 140, ref.NO_SCORE]] and d.chosen.tolist() == [1]
    d = ref.decide(cells, cost, _potential(), command, own=_own(pose), outside_is_free=True)
    assert d.score.tolist() == [[0, 140, ref.NO_SCORE]] and d.chosen.tolist() == [0]      # an outside swept point counts 0; an outside scoring point still blocks


def test_a_scoring_point_without_a_path():
    pot = _potential()
    pot[0, 2, 4] = NONE
    d = ref.decide(_cells(), None, pot, COMMAND, own=_own())
    assert d.score.tolist() == [[ref.NO_SCORE, 0, 0]] and d.chosen.tolist() == [1]
    pot[0, 2, 4] = NONE - 1      # the largest finite value is a score like any other
    d = ref.decide(_cells(), None, pot, COMMAND, own=_own(), goal_weight=65535, obstacle_weight=65535, bias=[2 ** 31 - 1, 0, 0])
    assert d.score[0, 0] == 65535 * (NONE - 1) + 2 ** 31 - 1 and d.chosen.tolist() == [1]
    points = POINTS[:, 1:]      # P = 1: no swept point at all
    d = ref.decide(_cells(points=points), np.full((1, 5, 5), 255, np.uint8), _potential(), COMMAND, own=_own())
    assert d.score.tolist() == [[0, 0, 0]]


def test_the_gpu_float_stage_meets_the_cap_by_the_reference_alone():
    fs = ref.FLOAT_STAGE
    assert fs.pose.dtype == np.float32 and fs.pose.shape == (3, 3)
    q = (fs.pose[:2].astype(np.float64) - np.array(fs.origin)[:, None]) / fs.cell
    assert (np.abs(q - np.round(q)) > 0.05).all()      # the robots themselves are off the cell edges
    own = ref.place(fs.pose, np.zeros((1, 1, 2), np.float32), *fs.origin, fs.cell, fs.nx, fs.ny)
    assert own.sure.all() and (own.cell >= 0).all()
    for name, command, points in ref.float_stage_tables():
        pl = ref.place(fs.pose, points, *fs.origin, fs.cell, fs.nx, fs.ny)
        share = ref.unsure_share(pl)
        print(name, points.shape, "unsure share per env", share.tolist(), "largest margin [m]", float(pl.margin.max()))
        assert (share <= ref.MAX_AMBIGUOUS).all() and pl.margin.max() < 1e-3 * fs.cell
        assert ((pl.cell >= 0).reshape(3, -1).mean(1) > 0.9).all()      # and on the grid
