"""Reference for smj_costmap_to_navigation (include/smj_navigation.h): a heap Dijkstra from the goals over the rule of the header, in
plain Python on numpy int64, and `next` by its definition from the potential.  It shares nothing with the kernel's scheme (sweeps
along rows and columns until nothing changes).

Rule: cell c is passable iff cost[c] < lethal, weight w(c) = neutral + cost[c]; 8 neighbours, passable cells only; an axial move costs
5 (w(a) + w(b)), a diagonal one 7 (w(a) + w(b)) and exists only if the two cells it passes between are passable."""
import heapq

import numpy as np

NONE = 1 << 30
# the 8 neighbours in ascending linear index
MOVES = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def moves_of(ok, y, x):
    """(j, i, diagonal) of the moves of a passable cell (y, x) of the bool grid ok, in ascending linear index."""
    ny, nx = ok.shape
    for dy, dx in MOVES:
        j, i = y + dy, x + dx
        if not (0 <= j < ny and 0 <= i < nx) or not ok[j, i]:
            continue
        if dy and dx and not (ok[j, x] and ok[y, i]):
            continue
        yield j, i, bool(dy and dx)


def potential(cost, goals, lethal=253, neutral=50):
    """int64 [ny, nx] of one env: cost uint8 [ny, nx], goals an iterable of linear indices (bad ones are skipped)."""
    cost = np.asarray(cost)
    ny, nx = cost.shape
    ok = cost.astype(np.int64) < lethal
    w = neutral + cost.astype(np.int64)
    pot = np.full((ny, nx), NONE, np.int64)
    heap = []
    for g in goals:
        g = int(g)
        if 0 <= g < ny * nx and ok[g // nx, g % nx] and pot[g // nx, g % nx] != 0:
            pot[g // nx, g % nx] = 0
            heap.append((0, g))
    heapq.heapify(heap)
    okl, wl, potl = ok.tolist(), w.tolist(), pot.tolist()      # python lists: several times faster than numpy scalars
    while heap:
        d, c = heapq.heappop(heap)
        y, x = divmod(c, nx)
        if d > potl[y][x]:
            continue
        wc = wl[y][x]
        for dy, dx in MOVES:
            j, i = y + dy, x + dx
            if not (0 <= j < ny and 0 <= i < nx) or not okl[j][i]:
                continue
            if dy and dx and not (okl[j][x] and okl[y][i]):
                continue
            nd = d + (7 if dy and dx else 5) * (wc + wl[j][i])
            if nd < potl[j][i]:
                potl[j][i] = nd
                heapq.heappush(heap, (nd, j * nx + i))
    return np.array(potl, np.int64).reshape(ny, nx)


def next_of(cost, pot, lethal=253, neutral=50):
    """int64 [ny, nx]: per cell the neighbour that minimises move + potential, the smallest linear index among equals; the cell
    itself on a goal (potential 0); -1 where potential is NONE.  Vectorised over the 8 moves in ascending index order."""
    cost = np.asarray(cost)
    ny, nx = cost.shape
    ok = cost.astype(np.int64) < lethal
    w = neutral + cost.astype(np.int64)
    okp = np.zeros((ny + 2, nx + 2), bool)
    okp[1:-1, 1:-1] = ok
    wp = np.zeros((ny + 2, nx + 2), np.int64)
    wp[1:-1, 1:-1] = w
    pp = np.full((ny + 2, nx + 2), NONE, np.int64)
    pp[1:-1, 1:-1] = pot
    idx = np.arange(ny * nx, dtype=np.int64).reshape(ny, nx)
    best = np.full((ny, nx), np.iinfo(np.int64).max, np.int64)
    at = np.full((ny, nx), -1, np.int64)
    for dy, dx in MOVES:
        sl = (slice(1 + dy, ny + 1 + dy), slice(1 + dx, nx + 1 + dx))
        allow = ok & okp[sl] & (pp[sl] < NONE)
        if dy and dx:
            allow &= okp[1 + dy:ny + 1 + dy, 1:nx + 1] & okp[1:ny + 1, 1 + dx:nx + 1 + dx]
        s = pp[sl] + (7 if dy and dx else 5) * (w + wp[sl])
        take = allow & (s < best)      # strict: the first of equals in ascending index stays
        best = np.where(take, s, best)
        at = np.where(take, idx + dy * nx + dx, at)
    at = np.where(pot == 0, idx, at)
    return np.where(pot >= NONE, -1, at)


def field(cost, goals, lethal=253, neutral=50):
    """(potential, next) as int64 [B, ny, nx] for cost uint8 [B, ny, nx] and goals int [B, G]."""
    cost = np.asarray(cost)
    goals = np.asarray(goals).reshape(cost.shape[0], -1)
    pots = [potential(c, g, lethal, neutral) for c, g in zip(cost, goals)]
    return np.stack(pots), np.stack([next_of(c, p, lethal, neutral) for c, p in zip(cost, pots)])


def free_closed_form(ny, nx, gy, gx, neutral):
    """The potential of a free zero-cost grid with one goal: neutral (14 min(|dx|, |dy|) + 10 (max - min))."""
    yy, xx = np.mgrid[0:ny, 0:nx]
    a, b = np.abs(yy - gy), np.abs(xx - gx)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return neutral * (14 * lo + 10 * (hi - lo))


def synchronous_relaxation(cost, goals, lethal=253, neutral=50):
    """(potential, sweeps): every cell from its neighbours' previous values, until a sweep changes nothing."""
    cost = np.asarray(cost)
    ny, nx = cost.shape
    ok = cost.astype(np.int64) < lethal
    w = np.where(ok, neutral + cost.astype(np.int64), 0)
    P = np.full((ny + 2, nx + 2), NONE, np.int64)
    okp = np.zeros((ny + 2, nx + 2), bool)
    okp[1:-1, 1:-1] = ok
    wp = np.zeros((ny + 2, nx + 2), np.int64)
    wp[1:-1, 1:-1] = w
    for g in goals:
        g = int(g)
        if 0 <= g < ny * nx and ok[g // nx, g % nx]:
            P[1 + g // nx, 1 + g % nx] = 0
    sweeps = 0
    while True:
        sweeps += 1
        best = P[1:-1, 1:-1].copy()
        for dy, dx in MOVES:
            sl = (slice(1 + dy, ny + 1 + dy), slice(1 + dx, nx + 1 + dx))
            allow = okp[sl] & ok & (P[sl] < NONE)
            if dy and dx:
                allow &= okp[1 + dy:ny + 1 + dy, 1:nx + 1] & okp[1:ny + 1, 1 + dx:nx + 1 + dx]
            cand = P[sl] + (7 if dy and dx else 5) * (w + wp[sl])
            best = np.where(allow & (cand < best), cand, best)
        if (best == P[1:-1, 1:-1]).all():
            return best, sweeps
        P[1:-1, 1:-1] = best


def serpentine(ny, nx, lethal_cost=254):
    """uint8 [ny, nx]: the rows y = 1, 3, 5, .. lethal except one gap at alternating ends (the right end first)."""
    c = np.zeros((ny, nx), np.uint8)
    for k, y in enumerate(range(1, ny, 2)):
        c[y, :] = lethal_cost
        c[y, nx - 1 if k % 2 == 0 else 0] = 0
    return c


def follow(nxt, start, max_steps):
    """The cells visited from linear index `start` along next [ny, nx], the start included, until a cell points at itself, -1 is
    met or max_steps moves are done."""
    flat = np.asarray(nxt).reshape(-1)
    path = [int(start)]
    for _ in range(max_steps):
        n = int(flat[path[-1]])
        if n < 0 or n == path[-1]:
            break
        path.append(n)
    return path
