/* smj_navigation.h -- exact cost-to-goal fields (navigation functions) of costmaps (libsmj.so, HIP / gfx950).
 *
 * Part of the C-ABI: smj_distance.h includes this file, smj_occupancy.h includes that one and smj.h that one, so a caller includes
 * smj.h alone.  It is a header of its own because existing tests fix the include list of smj.h and the tail of smj_occupancy.h; what
 * is declared here is listed in lib.NAVIGATION_EXPORTS and held to the library by tests/test_navigation_capi.py.  Same rules as
 * smj.h: caller-owned device pointers, 0 on success, a negative code and smj_last_error otherwise, asynchronous on the caller's
 * stream.
 */
#ifndef SMJ_NAVIGATION_H
#define SMJ_NAVIGATION_H
#include "smj.h"
#ifdef __cplusplus
extern "C" {
#endif

/* potential of a cell from which no goal can be reached */
#define SMJ_NAV_NONE (1 << 30)

/* Per cell of a costmap the cheapest path cost to the nearest goal cell (the navigation function) and the neighbour to step to: the
 * layer a shaping reward, a "distance remaining" observation or a grid-following base controller is built on.  Integers only.
 * cost_dev: uint8 [num_envs][ny][nx], row-major, rows follow y, linear index c = y nx + x; any alignment; e.g. what
 * StatusStretchDistanceField.inflated_cost() gives.  Null means cost 0 everywhere (and nothing lethal).  num_envs is the context's;
 * the entry needs no bound slot and no model tables.
 * goal_dev: int32 [num_envs][num_goals], 1 <= num_goals <= 64: linear indices of goal cells.  A value outside [0, nx ny) is skipped
 * (-1 is the "unused" value), and so is a goal on an impassable cell; an env with no goal left gets the "none" values everywhere.
 * Cell c is passable iff cost[c] < lethal (1 <= lethal <= 256; 256: every cell is passable); its weight is
 * w(c) = neutral + cost[c], 1 <= neutral <= 255.
 * Moves go to the 8 neighbours inside the grid, between passable cells only.  An axial move a - b costs 5 (w(a) + w(b)), a diagonal
 * one 7 (w(a) + w(b)); a diagonal move between (y, x) and (y + dy, x + dx) exists only if both (y + dy, x) and (y, x + dx) are
 * passable: no corner is cut.  The rule is symmetric, so the cost from the goal equals the cost to it.  On a zero-cost map with
 * neutral = 1 a straight step costs 10 and a diagonal one 14.
 * potential_dev: int32 [num_envs][ny][nx].  potential[c] = the minimum over all paths from c to any used goal of the sum of the move
 * costs; 0 on a goal; SMJ_NAV_NONE on an impassable cell and on a cell from which no goal can be reached.  The largest finite value
 * is at most 65535 * 7 * 1020 = 467 919 900 < 2^30 = SMJ_NAV_NONE (a path of at most 65535 moves, each at most 7 (510 + 510)).
 * next_dev: int32 [num_envs][ny][nx], or null (not wanted: that buffer is left untouched).  next[c] = the linear index of the
 * neighbour n, over the moves of c, that minimises move(c, n) + potential[n]; AMONG EQUAL SUMS THE SMALLEST LINEAR INDEX WINS; a goal
 * cell points at itself; -1 wherever potential is SMJ_NAV_NONE.  The minimum equals potential[c], so following next from a reachable
 * cell reaches a goal with strictly decreasing potential.
 * How it is computed: the potential is relaxed in place until nothing changes (one workgroup per env; in LDS up to 16384 cells, in
 * potential_dev itself above that).  The minimum over paths of an integer path cost is unique, so the result does not depend on any
 * order of evaluation and two calls give identical arrays.
 * Four-byte alignment suffices for the three int32 pointers (16-byte aligned ones take wide stores, same values).  No workspace is
 * allocated.
 * Errors: -1 for a null goal_dev or potential_dev, a misaligned goal_dev / potential_dev / next_dev, nx or ny < 1, nx or ny > 4096,
 * nx * ny > 65536, num_goals outside [1, 64], lethal outside [1, 256], neutral outside [1, 255], an output range that overlaps an
 * input range or the other output.  A refused call writes nothing. */
int smj_costmap_to_navigation(smj_ctx* ctx, const void* cost_dev, const void* goal_dev, int num_goals, int nx, int ny,
                              int lethal, int neutral, void* potential_dev, void* next_dev, void* stream);

#ifdef __cplusplus
}
#endif
#include "smj_frontier.h"
#endif
