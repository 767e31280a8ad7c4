"""Reference of the distance field (smj_occupancy_to_distance, include/smj_distance.h): per cell the minimum over ALL obstacle cells
of the lexicographic key (d^2, index), in int64 numpy.  No decomposition into rows and columns, no early stop, no bit mask: nothing
of the kernel's scheme is shared.

The obstacle cells are enumerated in two ways that give the same minimum.  By list: every cell against every obstacle, chunked so
that the key tensor stays under about 1 GiB.  That alone is the definition, but on a dense grid of 65536 cells it is 10^9 keys and
more.  So first by offset: every cell against every obstacle within `window` cells in y and in x ((2 window + 1)^2 shifted copies of
the mask).  A cell whose minimum over that window is d^2 <= window^2 is done -- an obstacle with a key no larger has |dy|, |dx| <= window and
was among those enumerated; every other cell goes through the list.  window = 0 is the list alone, and tests/test_distance_ref.py
holds the two against each other."""
import numpy as np

NONE = 1 << 30
BUDGET = 1 << 30      # bytes of one chunk's int64 keys
SHIFT = 17            # key = d^2 * 2^17 + index: index < 2^16, d^2 < 2^25, far inside int64
BIG = np.int64(NONE) << SHIFT


def obstacle_mask(hit, miss=None, min_hits=1, unknown_is_obstacle=False):
    """bool [..., ny, nx]: hit >= min_hits, or -- with unknown_is_obstacle and a miss layer -- hit == 0 and miss == 0."""
    hit = np.asarray(hit)
    ob = hit >= min_hits
    if unknown_is_obstacle and miss is not None:
        ob = ob | ((hit == 0) & (np.asarray(miss) == 0))
    return ob


def apply_bound(dist2, nearest, R):
    """The R rule: a cell whose dist2 > R^2 has none.  R = 0: no bound."""
    if R <= 0:
        return dist2, nearest
    far = dist2 > R * R
    return np.where(far, NONE, dist2).astype(np.int32), np.where(far, -1, nearest).astype(np.int32)


def _keys_by_list(cy, cx, oy, ox, nx):
    """min over the listed obstacles of the key, for the cells (cy, cx)."""
    out = np.empty(cy.size, np.int64)
    idx = oy * nx + ox
    step = max(1, int(BUDGET // (8 * oy.size)))
    for c0 in range(0, cy.size, step):
        y, x = cy[c0:c0 + step, None], cx[c0:c0 + step, None]
        out[c0:c0 + step] = ((((y - oy[None, :]) ** 2 + (x - ox[None, :]) ** 2) << SHIFT) + idx[None, :]).min(-1)
    return out


def field_of_mask(mask, R=0, window=8):
    """(dist2, nearest) int32 [ny, nx] of one bool grid."""
    mask = np.asarray(mask, bool)
    ny, nx = mask.shape
    key = np.full((ny, nx), BIG, np.int64)
    oy, ox = (v.astype(np.int64) for v in np.nonzero(mask))
    if oy.size:
        if window > 0:
            W = window
            padded = np.zeros((ny + 2 * W, nx + 2 * W), bool)
            padded[W:W + ny, W:W + nx] = mask
            here = np.arange(ny, dtype=np.int64)[:, None] * nx + np.arange(nx, dtype=np.int64)[None, :]
            for dy in range(-W, W + 1):
                for dx in range(-W, W + 1):
                    there = padded[W + dy:W + dy + ny, W + dx:W + dx + nx]      # is (y + dy, x + dx) an obstacle
                    k = (np.int64(dy * dy + dx * dx) << SHIFT) + here + (dy * nx + dx)
                    key = np.where(there & (k < key), k, key)
        rest = (key >> SHIFT) > window * window
        cy, cx = (v.astype(np.int64) for v in np.nonzero(rest))
        if cy.size:
            key[rest] = _keys_by_list(cy, cx, oy, ox, nx)
    dist2 = (key >> SHIFT).astype(np.int32)
    near = np.where(key == BIG, -1, key & ((1 << SHIFT) - 1)).astype(np.int32)
    return apply_bound(dist2, near, R)


def field(hit, miss=None, min_hits=1, unknown_is_obstacle=False, R=0):
    """(dist2, nearest) int32 [B, ny, nx] of int grids [B, ny, nx]."""
    ob = obstacle_mask(hit, miss, min_hits, unknown_is_obstacle)
    out = [field_of_mask(m, R) for m in ob]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def tie_grid(ny, nx):
    """Obstacles at the middles of the four edges: the centre of an odd square grid is equally far from all four."""
    m = np.zeros((ny, nx), bool)
    m[0, nx // 2] = m[ny - 1, nx // 2] = m[ny // 2, 0] = m[ny // 2, nx - 1] = True
    return m
