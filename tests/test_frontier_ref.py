"""The reference of the frontier tests (tests/frontier_ref.py) against what can be known without it: a 5 x 5 map worked out by hand,
the maps without a frontier, diagonal contact, the states of StatusStretchOccupancyGrid.occupancy() and the sizes of the shared maps.
CPU only."""
import numpy as np

import frontier_ref as ref

U, F, O = -1, 0, 1
MAP = np.array([[F, F, U, F, F],
                [F, F, U, F, O],
                [F, F, F, F, F],
                [O, O, F, U, U],
                [F, F, F, U, F]], np.int8)


def test_five_by_five_by_hand():
    """Frontier cells (c = 5 y + x): 1, 3, 6, 8 beside the unknown column, 12 below it, 13, 14, 17, 22 beside the unknown block and 24
    inside it.  6 and 8 touch 12 diagonally, so all but 24 are one region: 9 cells, sx = 21, sy = 15; (9 x - 21)^2 + (9 y - 15)^2 is
    18 at cell 12 = (2, 2) and at least 45 elsewhere."""
    hit, miss = ref.counts_of(MAP)
    mask = ref.frontier_mask(hit, miss)
    assert np.flatnonzero(mask).tolist() == [1, 3, 6, 8, 12, 13, 14, 17, 22, 24]
    lab, goal, region, count = ref.frontiers(hit, miss, min_size=1, max_regions=3)
    want = np.full(25, -1)
    want[[1, 3, 6, 8, 12, 13, 14, 17, 22]] = 1
    want[24] = 24
    assert np.array_equal(lab.ravel(), want)
    assert goal.tolist() == [12, 24, -1] and region.tolist() == [[1, 9, 21, 15], [24, 1, 4, 4], [-1, 0, 0, 0]] and count.tolist() == [2, 10]
    lab2, goal, region, count = ref.frontiers(hit, miss, min_size=2, max_regions=3)
    assert np.array_equal(lab2, lab) and goal.tolist() == [12, -1, -1] and count.tolist() == [1, 10]      # the labels keep the small region
    _, goal, region, count = ref.frontiers(hit, miss, min_size=1, max_regions=1)
    assert goal.tolist() == [12] and region.tolist() == [[1, 9, 21, 15]] and count.tolist() == [2, 10]      # the count is not capped
    # cell 12 lethal: {1, 6}, {3, 8, 13, 14, 17, 22} (17 touches 13 diagonally) and {24}; larger first
    cost = np.zeros((5, 5), np.uint8)
    cost[2, 2] = 253
    lab, goal, region, count = ref.frontiers(hit, miss, cost, min_size=1, max_regions=4)
    assert sorted(set(lab.ravel().tolist())) == [-1, 1, 3, 24] and lab[2, 2] == -1 and count.tolist() == [3, 9]
    assert region[:, 0].tolist() == [3, 1, 24, -1] and region[:, 1].tolist() == [6, 2, 1, 0]
    assert region[0].tolist() == [3, 6, 17, 12]      # x: 3 3 3 4 2 2, y: 0 1 2 2 3 4; 6 (x, y) - (17, 12) is (1, 0) at cell 13 = (3, 2)
    assert goal.tolist() == [13, 1, 24, -1]      # {1, 6}: both cells equally near their centroid, the smaller index wins
    assert np.array_equal(ref.frontiers(hit, miss, cost, lethal=254, min_size=1)[0], ref.frontiers(hit, miss, min_size=1)[0])


def test_no_unknown_or_no_free_cell_means_no_frontier():
    for fill in (F, U, O):
        hit, miss = ref.counts_of(np.full((6, 7), fill, np.int8))
        lab, goal, region, count = ref.frontiers(hit, miss, min_size=1, max_regions=2)
        assert (lab == -1).all() and goal.tolist() == [-1, -1] and count.tolist() == [0, 0] and region.tolist() == [[-1, 0, 0, 0]] * 2
    # unknown beside occupied only: still none
    s = np.full((4, 4), U, np.int8)
    s[1:3, 1:3] = O
    assert not ref.frontier_mask(*ref.counts_of(s)).any()


def test_diagonal_contact_is_one_region():
    s = np.full((4, 4), O, np.int8)
    s[0, 0] = s[1, 1] = F
    s[0, 1] = s[1, 0] = U
    lab, goal, region, count = ref.frontiers(*ref.counts_of(s), min_size=1, max_regions=2)
    assert lab[0, 0] == lab[1, 1] == 0 and (lab >= 0).sum() == 2 and count.tolist() == [1, 2] and goal.tolist() == [0, -1]


def test_states_follow_the_occupancy_rule():
    """min_hits = 2, counts 0 .. 3: hit 2, 3 occupied; else miss > 0 free; else unknown -- hit 1 with miss 0 included."""
    hit, miss = np.meshgrid(np.arange(4), np.arange(4), indexing="ij")
    s = ref.states(hit, miss, 2)
    assert (s[2:] == 1).all() and (s[:2, 1:] == 0).all() and (s[:2, 0] == -1).all()
    rng = np.random.default_rng(5)
    hit, miss = rng.integers(0, 4, (9, 11)), rng.integers(0, 4, (9, 11))
    occ = np.where(hit >= 2, 100, np.where(miss > 0, 0, -1))      # StatusStretchOccupancyGrid.occupancy(2)
    mask = ref.frontier_mask(hit, miss, min_hits=2)
    for y in range(9):
        for x in range(11):
            near = [occ[yy, xx] for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)) if 0 <= yy < 9 and 0 <= xx < 11]
            assert mask[y, x] == (occ[y, x] == 0 and -1 in near)
    assert mask.any() and not np.array_equal(mask, ref.frontier_mask(hit, miss, min_hits=1))


def test_the_shared_maps():
    for n, cells in ((128, 8255), (256, 32895)):
        lab, goal, region, count = ref.frontiers(*ref.counts_of(ref.serpentine(n, n)), min_size=1, max_regions=2)
        assert count.tolist() == [1, cells] and region[0, :2].tolist() == [0, cells]
    lab, goal, region, count = ref.frontiers(*ref.counts_of(ref.isolated(5, 7)), min_size=1, max_regions=64)
    assert count.tolist() == [12, 12] and goal[:12].tolist() == [0, 2, 4, 6, 14, 16, 18, 20, 28, 30, 32, 34] and (goal[12:] == -1).all()
    s = ref.spiral(12, 16)
    lab, goal, region, count = ref.frontiers(*ref.counts_of(s), min_size=1, max_regions=2)
    assert count[0] == 1 and count[1] == (s == 0).sum() - 3 > 60      # one corridor, every cell of it beside unknown but three corners on the rim
    lab, goal, region, count = ref.frontiers(*ref.counts_of(ref.disc(12, 16)), min_size=1, max_regions=2)
    assert count[0] == 1 and lab[6 - 4, 8] == lab[6 + 4, 8] >= 0 and lab[6, 8] == -1
    lab, goal, region, count = ref.frontiers(*ref.counts_of(ref.rooms(12, 16)), min_size=1, max_regions=4)
    assert count[0] == 2 and region[0, 1] > region[1, 1] > 0
