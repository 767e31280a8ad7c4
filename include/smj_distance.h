/* smj_distance.h -- exact distance fields of occupancy grids (libsmj.so, HIP / gfx950).
 *
 * Part of the C-ABI: smj_occupancy.h includes this file and smj.h includes that one, so a caller includes smj.h alone.  It is a
 * header of its own because existing tests fix the include list of smj.h and the declarations of smj_occupancy.h; what is declared
 * here is listed in lib.DISTANCE_EXPORTS and held to the library by tests/test_distance_capi.py.  Same rules as smj.h: caller-owned
 * device pointers, 0 on success, a negative code and smj_last_error otherwise, asynchronous on the caller's stream.
 */
#ifndef SMJ_DISTANCE_H
#define SMJ_DISTANCE_H
#include "smj.h"
#ifdef __cplusplus
extern "C" {
#endif

/* dist2 of a cell with no obstacle (in reach) */
#define SMJ_DIST_NONE (1 << 30)

/* Per cell of an occupancy grid the squared Euclidean distance, in cells, to the nearest obstacle cell, and which cell that is: the
 * layer a costmap, a clearance reward or a planner is built on.  Integers only.
 * hit_dev, miss_dev: int32 [num_envs][ny][nx], row-major, rows follow y: exactly what smj_lidar_to_occupancy writes (any counts
 * will do: a 0 / 1 mask as hit with min_hits = 1).  miss_dev may be null.  num_envs is the context's; the entry needs no bound slot
 * and no lidar tables.
 * Cell c is an obstacle iff hit[c] >= min_hits, or unknown_is_obstacle is set and hit[c] == 0 && miss[c] == 0 (no ray has seen the
 * cell).  Nothing outside the grid is an obstacle.
 * dist2_dev: int32 [num_envs][ny][nx].  dist2[y][x] = the minimum over the obstacle cells (j, i) of the env's grid of
 * (y - j)^2 + (x - i)^2; 0 on an obstacle; SMJ_DIST_NONE when the grid has no obstacle.
 * nearest_dev: int32 [num_envs][ny][nx], or null (not wanted).  nearest[y][x] = the linear index j nx + i of the obstacle that attains
 * the minimum; AMONG EQUAL DISTANCES THE SMALLEST LINEAR INDEX WINS; -1 where dist2 is SMJ_DIST_NONE.
 * max_dist_cells = R > 0 bounds the search: a cell whose true dist2 > R^2 gets SMJ_DIST_NONE and -1 (the inflation radius of a
 * costmap; it also keeps the search short on sparse maps).  R = 0: no bound.
 * How it is computed: the lexicographic minimum of (dist2, index) separates exactly into a pass along the rows -- per cell the
 * nearest obstacle of its row, the left one of two equally near -- and a pass along the columns -- the minimum over rows j of
 * (dx[j][x]^2 + (y - j)^2, j nx + x + dx[j][x]), searched outward from row y until dy^2 > best, strictly, so that an equal distance
 * on a lower row is still seen.  There is no float anywhere: the result does not depend on any order of evaluation and two calls
 * give identical arrays.
 * Four-byte alignment suffices for all four pointers (16-byte aligned ones take wide stores, same values).  No workspace is
 * allocated.
 * Errors: -1 for a null or misaligned hit_dev / dist2_dev, a misaligned miss_dev / nearest_dev, nx or ny < 1, nx or ny > 4096 (row
 * offsets fit 16 bits, dist2 < 2^25), nx * ny > 65536, min_hits < 1, max_dist_cells < 0, unknown_is_obstacle without miss_dev, an
 * output range that overlaps an input range or the other output (several workgroups of an env read the grid while others store).
 * A refused call writes nothing. */
int smj_occupancy_to_distance(smj_ctx* ctx, const void* hit_dev, const void* miss_dev, int nx, int ny,
                              int min_hits, int unknown_is_obstacle, int max_dist_cells,
                              void* dist2_dev, void* nearest_dev, void* stream);

#ifdef __cplusplus
}
#endif
#include "smj_navigation.h"
#endif
