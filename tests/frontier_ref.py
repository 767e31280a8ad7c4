"""Reference for smj_occupancy_to_frontiers (include/smj_frontier.h), written from the header's definitions: numpy for the states and
the frontier mask, a flood fill for the labels, Python integers for the representative's key.  Plus the maps the tests share, as
state arrays (1 occupied, 0 free, -1 unknown: the signs of StatusStretchOccupancyGrid.occupancy())."""
import numpy as np


def counts_of(state):
    """(hit, miss) int32 of a state array: one hit on an occupied cell, one miss on a free one, nothing on an unknown one."""
    state = np.asarray(state)
    return (state > 0).astype(np.int32), (state == 0).astype(np.int32)


def states(hit, miss, min_hits=1):
    """int8: 1 occupied (hit >= min_hits), else 0 free (miss > 0), else -1 unknown."""
    return np.where(np.asarray(hit) >= min_hits, 1, np.where(np.asarray(miss) > 0, 0, -1)).astype(np.int8)


def frontier_mask(hit, miss, cost=None, min_hits=1, lethal=253):
    """bool [ny, nx]: free, an unknown cell among the 4 neighbours inside the grid, and cost < lethal where there is a cost."""
    s = states(hit, miss, min_hits)
    unknown = np.pad(s == -1, 1)      # outside the grid: not unknown
    near = unknown[:-2, 1:-1] | unknown[2:, 1:-1] | unknown[1:-1, :-2] | unknown[1:-1, 2:]
    m = (s == 0) & near
    if cost is not None:
        m &= np.asarray(cost).astype(np.int64) < lethal
    return m


def labels(mask):
    """int32 [ny, nx]: the smallest linear index of the cell's 8-connected component of `mask`, -1 off it.  Cells are visited in
    ascending index, so the seed of a fill is its component's smallest cell."""
    ny, nx = mask.shape
    lab = np.full(ny * nx, -1, np.int32)
    todo = mask.ravel().copy()
    for seed in np.flatnonzero(todo).tolist():
        if not todo[seed]:
            continue
        todo[seed] = False
        lab[seed] = seed
        stack = [seed]
        while stack:
            c = stack.pop()
            y, x = divmod(c, nx)
            for yy in range(max(y - 1, 0), min(y + 2, ny)):
                for xx in range(max(x - 1, 0), min(x + 2, nx)):
                    n = yy * nx + xx
                    if todo[n]:
                        todo[n] = False
                        lab[n] = seed
                        stack.append(n)
    return lab.reshape(ny, nx)


def frontiers(hit, miss, cost=None, min_hits=1, lethal=253, min_size=4, max_regions=16):
    """One env: (label [ny, nx], goal [G], region [G, 4], count [2]), int32."""
    lab = labels(frontier_mask(hit, miss, cost, min_hits, lethal))
    ny, nx = lab.shape
    flat = lab.ravel()
    cells = np.flatnonzero(flat >= 0)
    roots, sizes = np.unique(flat[cells], return_counts=True)
    kept = sorted((int(-s), int(r)) for r, s in zip(roots, sizes) if s >= min_size)
    goal = np.full(max_regions, -1, np.int32)
    region = np.tile(np.array([-1, 0, 0, 0], np.int32), (max_regions, 1))
    for k, (neg, r) in enumerate(kept[:max_regions]):
        mine = [int(c) for c in cells[flat[cells] == r]]
        s, sx, sy = len(mine), sum(c % nx for c in mine), sum(c // nx for c in mine)
        assert s == -neg
        goal[k] = min(mine, key=lambda c: ((s * (c % nx) - sx) ** 2 + (s * (c // nx) - sy) ** 2, c))      # Python integers: exact
        region[k] = (r, s, sx, sy)
    return lab, goal, region, np.array([len(kept), len(cells)], np.int32)


def batch(hit, miss, cost=None, **kw):
    """[B, ..] inputs -> (label [B, ny, nx], goal [B, G], region [B, G, 4], count [B, 2])."""
    out = [frontiers(hit[e], miss[e], None if cost is None else cost[e], **kw) for e in range(len(hit))]
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


# ------------------------------------------------------------------ maps, as state arrays

def disc(ny, nx):
    """A free disc of radius min(nx, ny) // 3 about the centre, in unknown."""
    yy, xx = np.mgrid[0:ny, 0:nx]
    r = min(nx, ny) // 3
    return np.where((yy - ny // 2) ** 2 + (xx - nx // 2) ** 2 <= r * r, 0, -1).astype(np.int8)


def serpentine(ny, nx):
    """A free corridor between unknown walls: the rows y = 1, 3, 5, .. unknown except one gap at alternating ends (the right end
    first), every other cell free -- the map of navigation_ref.serpentine."""
    s = np.zeros((ny, nx), np.int8)
    for k, y in enumerate(range(1, ny, 2)):
        s[y, :] = -1
        s[y, nx - 1 if k % 2 == 0 else 0] = 0
    return s


def spiral(ny, nx):
    """A free corridor one cell wide that winds inwards from cell (0, 0), its turns two cells apart, in unknown."""
    s = np.full((ny, nx), -1, np.int8)
    y = x = 0
    dy, dx = 0, 1
    s[0, 0] = 0
    turns = 0
    while turns < 2:
        y2, x2 = y + 2 * dy, x + 2 * dx
        y1, x1 = y + dy, x + dx
        ahead_free = 0 <= y2 < ny and 0 <= x2 < nx and s[y2, x2] == 0
        if 0 <= y1 < ny and 0 <= x1 < nx and s[y1, x1] != 0 and not ahead_free:
            y, x = y1, x1
            s[y, x] = 0
            turns = 0
        else:
            dy, dx = dx, -dy      # right, down, left, up
            turns += 1
    return s


def isolated(ny, nx):
    """Free at even x and even y, otherwise unknown."""
    yy, xx = np.mgrid[0:ny, 0:nx]
    return np.where((yy % 2 == 0) & (xx % 2 == 0), 0, -1).astype(np.int8)


def rooms(ny, nx):
    """Two free rooms of different size, one cell inside the rim of an unknown grid: the left one takes a third of the width and
    ends at a column of occupied cells (its frontier is a U), an unknown column lies between that and the right one (a ring)."""
    s = np.full((ny, nx), -1, np.int8)
    a = max(nx // 3, 1)
    s[1:ny - 1, 1:a] = 0
    s[:, a:a + 1] = 1
    s[1:ny - 1, a + 2:nx - 1] = 0
    return s
