"""The reference of the navigation tests (tests/navigation_ref.py) against what can be known without it: the closed form of a free
grid, symmetry, a synchronous relaxation written independently, a wall with one gap, the no-corner-cutting rule on a 3 x 3 case worked
by hand, skipped goals, and that following `next` reaches a goal with strictly falling potential.  CPU only."""
import numpy as np
import pytest

import navigation_ref as ref

NONE = ref.NONE


@pytest.mark.parametrize("neutral", [1, 3])
def test_free_grid_closed_form(neutral):
    ny, nx = 12, 16
    for gy, gx in ((5, 3), (0, 0), (11, 15), (0, 15)):
        p = ref.potential(np.zeros((ny, nx), np.uint8), [gy * nx + gx], neutral=neutral)
        assert np.array_equal(p, ref.free_closed_form(ny, nx, gy, gx, neutral))
    assert ref.potential(np.zeros((1, 2), np.uint8), [0], neutral=1)[0, 1] == 10
    assert ref.potential(np.zeros((2, 2), np.uint8), [0], neutral=1)[1, 1] == 14


def test_symmetry_between_random_cell_pairs():
    rng = np.random.default_rng(5)
    cost = rng.integers(0, 200, (20, 20)).astype(np.uint8)
    cost[rng.random((20, 20)) < 0.2] = 254
    free = np.flatnonzero(cost.ravel() < 253)
    finite = 0
    for _ in range(8):
        a, b = (int(v) for v in rng.choice(free, 2, replace=False))
        ab, ba = ref.potential(cost, [a]).ravel()[b], ref.potential(cost, [b]).ravel()[a]
        assert ab == ba
        finite += ab < NONE
    assert finite >= 4


def test_synchronous_relaxation_gives_the_same_arrays():
    rng = np.random.default_rng(6)
    for ny, nx in ((9, 13), (31, 33)):
        cost = np.where(rng.random((ny, nx)) < 0.3, 254, rng.integers(0, 253, (ny, nx))).astype(np.uint8)
        goals = [int(np.flatnonzero(cost.ravel() < 253)[0]), ny * nx - 1, -1]
        for neutral, lethal in ((50, 253), (1, 253), (255, 256)):
            p = ref.potential(cost, goals, lethal, neutral)
            q, _ = ref.synchronous_relaxation(cost, goals, lethal, neutral)
            assert np.array_equal(p, q)
    s = ref.serpentine(31, 33)
    p = ref.potential(s, [0], neutral=1)
    q, sweeps = ref.synchronous_relaxation(s, [0], neutral=1)
    reach = int((p < NONE).sum())
    assert np.array_equal(p, q) and reach == 16 * 33 + 15 and sweeps >= reach - 33      # about one sweep per cell of the path


def test_serpentine_128_reaches_8256_cells():
    p = ref.potential(ref.serpentine(128, 128), [0], neutral=1)
    assert int((p < NONE).sum()) == 8256 and p[127, 0] == p[p < NONE].max()


def test_wall_with_one_gap():
    ny, nx = 7, 9
    cost = np.zeros((ny, nx), np.uint8)
    cost[:, 4] = 254
    cost[5, 4] = 0
    p = ref.potential(cost, [0], neutral=1)
    assert (p[:, 4][[0, 1, 2, 3, 4, 6]] == NONE).all()
    assert p[5, 3] == 3 * 14 + 2 * 10 and p[5, 4] == p[5, 3] + 10 and p[5, 5] == p[5, 4] + 10      # straight through the gap: no diagonal into or out of it
    assert p[0, 5] == p[5, 5] + 5 * 10 and p[4, 5] == p[5, 5] + 10 and p[4, 6] == p[5, 5] + 14
    cost[5, 4] = 254
    assert (ref.potential(cost, [0], neutral=1)[:, 5:] == NONE).all()


def test_no_corner_cutting_by_hand():
    """3 x 3, neutral 1, goal at (0, 0), lethal at (0, 1):   G X .
                                                             . . .
                                                             . . .
    (1, 1) may not step diagonally to the goal past the lethal cell: it goes (1, 0) then up, 10 + 10.  (0, 2) is reached from (1, 1)
    only through (1, 2): the diagonal (1, 1) -> (0, 2) passes the lethal cell too."""
    cost = np.zeros((3, 3), np.uint8)
    cost[0, 1] = 254
    p = ref.potential(cost, [0], neutral=1)
    want = np.array([[0, NONE, 40], [10, 20, 30], [20, 24, 34]])
    assert np.array_equal(p, want)
    n = ref.next_of(cost, p, neutral=1)
    assert np.array_equal(n, np.array([[0, -1, 5], [0, 3, 4], [3, 3, 4]]))
    # with the lethal cell free again the diagonal is back
    assert ref.potential(np.zeros((3, 3), np.uint8), [0], neutral=1)[1, 1] == 14


def test_checkerboard_leaves_only_the_goal():
    cost = np.where(np.indices((6, 7)).sum(0) % 2 == 1, 254, 0).astype(np.uint8)
    p = ref.potential(cost, [0], neutral=1)
    assert p[0, 0] == 0 and int((p < NONE).sum()) == 1


def test_skipped_goals():
    cost = np.zeros((4, 5), np.uint8)
    cost[2, 2] = 253
    none = np.full((4, 5), NONE)
    for goals in ([-1], [20], [-7, 10 ** 6], [12], [-1, 12, 20]):
        p = ref.potential(cost, goals)
        assert np.array_equal(p, none) and (ref.next_of(cost, p) == -1).all()
    p = ref.potential(cost, [-1, 12, 19], neutral=1)
    assert p[3, 4] == 0 and p[2, 2] == NONE and p[3, 0] == 40 and p[0, 4] == 30
    assert p[0, 1] == 2 * 14 + 2 * 10      # the straight diagonal (1, 2) -> (2, 3) would cut the corner of the lethal (2, 2)
    assert np.array_equal(ref.potential(cost, [19, 19, 0], neutral=1), np.minimum(ref.potential(cost, [19], neutral=1), ref.potential(cost, [0], neutral=1)))
    # lethal = 256: cost 255 is passable, weight neutral + 255
    c = np.full((1, 3), 255, np.uint8)
    assert ref.potential(c, [0], lethal=256, neutral=255).tolist() == [[0, 5100, 10200]] and (ref.potential(c, [0], lethal=255) == NONE).all()


def test_following_next_reaches_a_goal_with_strictly_falling_potential():
    rng = np.random.default_rng(8)
    ny, nx = 23, 29
    cost = np.where(rng.random((ny, nx)) < 0.25, 254, rng.integers(0, 253, (ny, nx))).astype(np.uint8)
    free = np.flatnonzero(cost.ravel() < 253)
    goals = [int(free[0]), int(free[-1]), int(free[len(free) // 2])]
    p = ref.potential(cost, goals)
    n = ref.next_of(cost, p)
    flat = p.ravel()
    assert ((n == -1) == (p >= NONE)).all() and all(n.ravel()[g] == g for g in goals)
    reachable = np.flatnonzero(flat < NONE)
    assert len(reachable) > ny * nx // 2
    for start in reachable[:: max(1, len(reachable) // 60)]:
        path = ref.follow(n, start, ny * nx)
        assert path[-1] in goals and all(flat[a] > flat[b] for a, b in zip(path, path[1:]))
        for a, b in zip(path, path[1:]):      # each step is a move of the rule and accounts exactly for the fall
            dy, dx = b // nx - a // nx, b % nx - a % nx
            assert max(abs(dy), abs(dx)) == 1 and flat[a] - flat[b] == (7 if dy and dx else 5) * (100 + int(cost.ravel()[a]) + int(cost.ravel()[b]))
