/* smj_frontier.h -- frontier regions of occupancy grids: where exploration should go next (libsmj.so, HIP / gfx950).
 *
 * Part of the C-ABI: smj_navigation.h includes this file, smj_distance.h includes that one, smj_occupancy.h that one and smj.h that
 * one, so a caller includes smj.h alone.  It is a header of its own because existing tests fix the include list of smj.h and the
 * contents of the headers before it; what is declared here is listed in lib.FRONTIER_EXPORTS and held to the library by
 * tests/test_frontier_capi.py.  Same rules as smj.h: caller-owned device pointers, 0 on success, a negative code and smj_last_error
 * otherwise, asynchronous on the caller's stream.
 */
#ifndef SMJ_FRONTIER_H
#define SMJ_FRONTIER_H
#include "smj.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Per env the frontier of an occupancy grid -- the free cells that border unseen space -- grouped into regions, with one goal cell
 * per region: the goal_dev of smj_costmap_to_navigation.  Integers only.  num_envs is the context's; the entry needs no bound slot
 * and no model tables.
 * hit_dev, miss_dev: int32 [num_envs][ny][nx], both required, row-major, rows follow y, linear index c = y nx + x: the counts of
 * smj_lidar_to_occupancy.  cost_dev: uint8 [num_envs][ny][nx], any alignment, or null.
 * 1 <= min_hits, 1 <= lethal <= 256, 1 <= min_size, 1 <= max_regions <= 64; nx, ny in [1, 4096] and nx ny <= 65536 (the limits of
 * smj_costmap_to_navigation).
 * Cell states: occupied iff hit >= min_hits; otherwise free iff miss > 0; otherwise unknown (so a cell with 0 < hit < min_hits and
 * miss == 0 is unknown).  Cells outside the grid are not unknown: an all-free grid has no frontier.
 * Frontier cell: a free cell with at least one unknown cell among its 4 neighbours inside the grid and, with cost_dev given,
 * cost[c] < lethal -- the passability test of smj_costmap_to_navigation, so a goal is never a cell that entry would skip.
 * Regions: the 8-connected components of the frontier cells.
 * label_dev: int32 [num_envs][ny][nx], required.  The smallest linear index in the cell's region; -1 on every cell off the frontier.
 * Every frontier cell is labelled, those of regions below min_size too.
 * Kept regions: those with size >= min_size, ordered by size descending, then by label ascending; the first max_regions are reported.
 * goal_dev: int32 [num_envs][max_regions], required.  Row k holds the representative cell of kept region k, -1 past the last one.
 * With s, sx, sy the region's cell count and the integer sums of its cells' x and y, the representative is the cell OF THE REGION that
 * minimises (s x - sx)^2 + (s y - sy)^2, computed in 64 bits; AMONG EQUAL VALUES THE SMALLEST LINEAR INDEX WINS.  It is a frontier
 * cell, hence free and passable; the centroid of a curved frontier need not be.
 * region_dev: int32 [num_envs][max_regions][4], or null: label, size, sx, sy per kept region, -1, 0, 0, 0 on unused rows
 * (sx <= 65536 * 4095 < 2^28).
 * count_dev: int32 [num_envs][2], or null: the number of regions with size >= min_size (it may exceed max_regions) and the number of
 * frontier cells.
 * A null region_dev or count_dev is left untouched.  Every output is unique, so two calls give identical arrays whatever the order
 * of evaluation; the inputs are unchanged; nothing outside the outputs is written.  No workspace is allocated; the outputs may hold
 * intermediate values while the kernel runs (one workgroup per env; the labels live in LDS up to 16384 cells, in label_dev itself
 * above that).  Four-byte alignment suffices (16-byte aligned pointers may take wide stores, same values).
 * Errors: -1 for a null or misaligned hit_dev / miss_dev / label_dev / goal_dev, a misaligned region_dev / count_dev, nx or ny < 1,
 * nx or ny > 4096, nx * ny > 65536, min_hits < 1, lethal outside [1, 256], min_size < 1, max_regions outside [1, 64], an output
 * range that overlaps an input range or another output.  A refused call writes nothing. */
int smj_occupancy_to_frontiers(smj_ctx* ctx, const void* hit_dev, const void* miss_dev, const void* cost_dev,
                               int nx, int ny, int min_hits, int lethal, int min_size, int max_regions,
                               void* label_dev, void* goal_dev, void* region_dev, void* count_dev, void* stream);

#ifdef __cplusplus
}
#endif
#include "smj_drive.h"
#endif
