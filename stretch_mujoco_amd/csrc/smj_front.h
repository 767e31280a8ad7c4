// Frontier regions of occupancy grids (smj_occupancy_to_frontiers, include/smj_frontier.h): the state of a cell, the frontier predicate,
// the union of one cell with its backward neighbours, the schedule, the codes a root's slot carries while the regions are counted and
// the representative's key, as plain inline functions (the store's groups: smj_grid.h).  The kernel of smj_front.hip calls exactly
// these; the header also compiles under a host compiler, so tests/front/front_check.cpp runs the shipped code serially against its own
// flood fill.  Integers only.
//
// The rule.  A cell is occupied iff hit >= min_hits, otherwise free iff miss > 0, otherwise unknown.  A frontier cell is a free cell
// with cost < lethal and an unknown cell among its 4 neighbours inside the grid.  Regions are the 8-connected components of the
// frontier cells; a cell's label is the smallest linear index of its region, -1 off the frontier.
//
// Storage.  One int32 per cell, reached through an accessor S with int get(int c), void set(int c, int v),
// int cas(int c, int expected, int v) (returns the value found) and int add(int c, int v): LDS or label_dev itself in the kernel, a
// vector in the host harness.  The same word holds, phase after phase, the cell's state code, the code with the frontier flag, the
// label, and -- in a root's slot, while the regions are counted and chosen -- the region's size or its row among the kept ones.
#pragma once
#include "smj_grid.h"   // SMJ_GRID_HD and the store's 16-byte groups

// The largest grid, the longest side and the most regions reported per env (those of the navigation entry, whose goal_dev the goals
// feed), and the cells whose labels fit LDS: 16384 int32 labels are 64 KiB, so TWO workgroups share a CU's 160 KiB and one runs
// while the other waits at a barrier or for an atomic; 32768 cells (128 KiB) would leave one workgroup per CU for every grid of the
// LDS build, the default 128 x 128 included, and nothing to hide those waits.
enum { SMJ_FRONT_MAX_CELLS = 65536, SMJ_FRONT_MAX_SIDE = 4096, SMJ_FRONT_MAX_REGIONS = 64, SMJ_FRONT_LDS_CELLS = 16384 };

// The state of a cell; BLOCKED is a free cell whose cost is lethal (free for its neighbours' sake, never a frontier cell itself).
// The codes fit two bits; SMJ_FRONT_FLAG marks a frontier cell beside them.
enum { SMJ_FRONT_OCCUPIED = 0, SMJ_FRONT_FREE = 1, SMJ_FRONT_UNKNOWN = 2, SMJ_FRONT_BLOCKED = 3, SMJ_FRONT_FLAG = 4 };
SMJ_GRID_HD int smj_front_state(int hit, int miss, int min_hits) {
  return hit >= min_hits ? SMJ_FRONT_OCCUPIED : miss > 0 ? SMJ_FRONT_FREE : SMJ_FRONT_UNKNOWN;
}
SMJ_GRID_HD bool smj_front_passable(int cost, int lethal) { return cost < lethal; }
SMJ_GRID_HD int smj_front_code(int hit, int miss, int cost, int min_hits, int lethal) {
  const int s = smj_front_state(hit, miss, min_hits);
  return s == SMJ_FRONT_FREE && !smj_front_passable(cost, lethal) ? SMJ_FRONT_BLOCKED : s;
}

// The frontier predicate of cell (y, x), from the codes (the low two bits of the store: a neighbour's flag may or may not be there yet).
template <class S>
SMJ_GRID_HD bool smj_front_is_frontier(const S& s, int nx, int ny, int y, int x) {
  const int c = y * nx + x;
  if ((s.get(c) & 3) != SMJ_FRONT_FREE) return false;
  const int l = s.get(x > 0 ? c - 1 : c), r = s.get(x + 1 < nx ? c + 1 : c), u = s.get(y > 0 ? c - nx : c), d = s.get(y + 1 < ny ? c + nx : c);
  return (l & 3) == SMJ_FRONT_UNKNOWN || (r & 3) == SMJ_FRONT_UNKNOWN || (u & 3) == SMJ_FRONT_UNKNOWN || (d & 3) == SMJ_FRONT_UNKNOWN;   // the cell itself is free, so a stand-in never counts
}

// Labels: a forest over the frontier cells.  label[c] <= c always, label[c] == c on a root, and label[c] is a cell of c's region;
// a cell off the frontier holds -1.  find walks to the root and halves the path on its way (each store puts a cell's grandparent in
// place of its parent: still a cell of the region, still below the cell, and only ever stored into a cell that is no root).
// Bound: the walk goes from a cell to a strictly smaller one, so it ends within c steps whatever other threads store meanwhile.
template <class S>
SMJ_GRID_HD int smj_front_find(S& s, int c) {
  int prev = c, curr = s.get(c);
  for (int i = 0; i < c && curr < prev; i++) {
    const int next = s.get(curr);
    if (next >= curr) break;   // curr is a root
    s.set(prev, next);
    prev = curr;
    curr = next;
  }
  return curr;
}

// union of the regions of a and b: the larger root is hung below the smaller one by a compare-and-swap that succeeds only while it
// still is a root; a failed one returns the cell another thread hung it below, and the union goes on from there.  Only roots are
// ever swapped and only non-roots stored into by find, so neither undoes the other.
// Bound: after a failed swap a becomes the value found, which is below a, and b was below a already: the larger of the two falls
// with every retry, so there are at most max(a, b) retries -- fewer than SMJ_FRONT_MAX_CELLS.  The bound never changes a result.
template <class S>
SMJ_GRID_HD void smj_front_union(S& s, int a, int b) {
  for (int i = 0; i < SMJ_FRONT_MAX_CELLS; i++) {
    a = smj_front_find(s, a);
    b = smj_front_find(s, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int found = s.cas(a, a, b);
    if (found == a) return;
    a = found;
  }
}

// One cell's step of the labelling: the union with each of its four BACKWARD neighbours (W, NW, N, NE: every 8-neighbour pair is met
// once, from its larger cell) that lies inside the grid and on the frontier.  After every cell has taken this step once, in any
// order or all at once, the roots are the smallest cells of the regions: no sweeps, no "until nothing changes".
template <class S>
SMJ_GRID_HD void smj_front_link(S& s, int nx, int y, int x) {
  const int c = y * nx + x;
  if (s.get(c) < 0) return;
  if (x > 0 && s.get(c - 1) >= 0) smj_front_union(s, c, c - 1);
  if (y > 0) {
    if (x > 0 && s.get(c - nx - 1) >= 0) smj_front_union(s, c, c - nx - 1);
    if (s.get(c - nx) >= 0) smj_front_union(s, c, c - nx);
    if (x + 1 < nx && s.get(c - nx + 1) >= 0) smj_front_union(s, c, c - nx + 1);
  }
}

// Flattening, once every union is done (no root changes any more): one jump of one cell, label[c] = label[label[c]], stored by the
// cell's own thread only; returns whether the label fell.  Jumps are repeated until a round changes nothing: then every frontier
// cell holds a root.  Values only fall here, so a stale read merely delays a fall.
// Bound: a round replaces every cell's parent by its grandparent (or by something nearer the root, where the parent has jumped
// already), so a cell d links away from its root is at most ceil(d / 2) away afterwards; d < 65536 = 2^16 gives depth 1 after 16
// rounds, and the 17th changes nothing.
template <class S>
SMJ_GRID_HD bool smj_front_jump(S& s, int c) {
  const int v = s.get(c);
  if (v < 0) return false;
  const int w = s.get(v);
  if (w >= v) return false;   // the parent is a root
  s.set(c, w);
  return true;
}
SMJ_GRID_HD int smj_front_max_jumps() { return 17; }

// The schedule: every pass hands cell k nthreads + t to thread t in its round k, so consecutive lanes touch consecutive words; the
// owner of a cell (the thread that rescans after one of its roots was chosen) follows from it.
SMJ_GRID_HD int smj_front_cell(int t, int k, int nthreads) { return k * nthreads + t; }
SMJ_GRID_HD int smj_front_rounds(int ncell, int nthreads) { return (ncell + nthreads - 1) / nthreads; }

// What a root's slot carries once the labels are flat (every frontier cell holds its root, >= 0; the rest -1): -1 - size while the
// cells are counted (<= -2), and SMJ_FRONT_CHOSEN - k once the region is row k of the kept ones (<= -2^20, below every size code).
enum { SMJ_FRONT_CHOSEN = -(1 << 20) };
SMJ_GRID_HD int smj_front_size_code(int size) { return -1 - size; }
SMJ_GRID_HD bool smj_front_is_size_code(int v) { return v <= -2 && v > SMJ_FRONT_CHOSEN; }
SMJ_GRID_HD int smj_front_code_size(int v) { return -1 - v; }
SMJ_GRID_HD int smj_front_row_code(int k) { return SMJ_FRONT_CHOSEN - k; }
SMJ_GRID_HD bool smj_front_is_row_code(int v) { return v <= SMJ_FRONT_CHOSEN; }
SMJ_GRID_HD int smj_front_code_row(int v) { return SMJ_FRONT_CHOSEN - v; }
// The row of the kept regions a frontier cell belongs to, -1 if its region is not among them: v is the cell's own word.
template <class S>
SMJ_GRID_HD int smj_front_row_of(const S& s, int v) {
  if (v == -1) return -1;
  const int code = v >= 0 ? s.get(v) : v;
  return smj_front_is_row_code(code) ? smj_front_code_row(code) : -1;
}

// The order of the kept regions as one number, larger = earlier: size descending, then label ascending.  size <= 65536, label < 65536;
// 0 is "none" (a size is at least 1).
SMJ_GRID_HD uint64_t smj_front_order_key(int size, int label) { return ((uint64_t)size << 16) | (uint64_t)(0xffff - label); }
SMJ_GRID_HD int smj_front_key_size(uint64_t key) { return (int)(key >> 16); }
SMJ_GRID_HD int smj_front_key_label(uint64_t key) { return 0xffff - (int)(key & 0xffff); }

// The representative's key of cell (y, x) in a region of s cells with coordinate sums sx, sy: the squared distance to the centroid
// times s^2.  |s x - sx| <= 65536 * 4095 < 2^28, so the sum of the two squares stays below 2^57.
SMJ_GRID_HD uint64_t smj_front_rep_key(int s, int sx, int sy, int y, int x) {
  const long long dx = (long long)s * x - sx, dy = (long long)s * y - sy;
  return (uint64_t)(dx * dx + dy * dy);
}

#if defined(__HIPCC__)
// Launch (smj_front.hip).  cost, region and count may be null.
void smj_launch_front(int num_envs, const int* hit, const int* miss, const uint8_t* cost, int nx, int ny, int min_hits, int lethal,
                      int min_size, int max_regions, int* label, int* goal, int* region, int* count, hipStream_t stream);
#endif
