// Exact cost-to-goal fields (navigation functions) of costmaps (smj_costmap_to_navigation, include/smj_navigation.h): the passability
// predicate, the move cost, the diagonal rule, "relax one cell from its neighbours", "next of one cell" and the sweep schedule as plain
// inline functions (the store's groups: smj_grid.h).  The kernel of smj_nav.hip calls exactly these; the header also compiles under a host
// compiler, so tests/nav/nav_check.cpp runs the shipped code serially against its own Dijkstra.  Integers only.
//
// The rule.  A cell c is passable iff cost[c] < lethal; its weight is w(c) = neutral + cost[c] (1 .. 510).  Moves go to the 8
// neighbours inside the grid, between passable cells: an axial move a-b costs 5 (w(a) + w(b)), a diagonal one 7 (w(a) + w(b)), and a
// diagonal move between (y, x) and (y + dy, x + dx) exists only if (y + dy, x) and (y, x + dx) are passable too (no corner cutting).
// potential[c] is the minimum over all paths from c to a goal of the sum of the move costs, 0 on a goal, SMJ_NAV_NONE where there is
// no path; at most 65535 * 7 * 1020 = 467 919 900 < 2^30.  next[c] is the neighbour n that minimises move(c, n) + potential[n], the
// smallest linear index among equals; c itself on a goal; -1 where potential is SMJ_NAV_NONE.
//
// Storage.  The weights are uint16, 0 for an impassable cell (a passable one has w >= neutral >= 1), so one read answers "passable"
// and "weight".  The potential is reached through an accessor P with int get(int c) const and void set(int c, int v): LDS or global
// memory in the kernel, a vector in the host harness.
#pragma once
#include "smj_grid.h"   // SMJ_GRID_HD and the store's 16-byte groups

// SMJ_NAV_NONE: the potential of a cell without a path to a goal -- the public header's macro, token for token, so that a translation
// unit may include both.  The largest grid, the longest side, the most goals per env, and the cells whose potential fits LDS (int32:
// 64 KiB, beside 32 KiB of weights).
#define SMJ_NAV_NONE (1 << 30)
enum { SMJ_NAV_MAX_CELLS = 65536, SMJ_NAV_MAX_SIDE = 4096, SMJ_NAV_MAX_GOALS = 64, SMJ_NAV_LDS_CELLS = 16384 };

// Passable iff cost < lethal; the stored weight, 0 = impassable.
SMJ_GRID_HD bool smj_nav_passable(int cost, int lethal) { return cost < lethal; }
SMJ_GRID_HD uint16_t smj_nav_weight(int cost, int lethal, int neutral) { return smj_nav_passable(cost, lethal) ? (uint16_t)(neutral + cost) : (uint16_t)0; }

// The cost of a move between two passable cells of weights wa, wb.
SMJ_GRID_HD int smj_nav_move(int wa, int wb, bool diagonal) { return (diagonal ? 7 : 5) * (wa + wb); }

// The diagonal rule: the move exists iff the two cells it passes between are passable (their stored weights are not 0).
SMJ_GRID_HD bool smj_nav_diagonal_open(int w_row_neighbour, int w_col_neighbour) { return w_row_neighbour != 0 && w_col_neighbour != 0; }

// Is a goal entry used: inside the grid and on a passable cell.
SMJ_GRID_HD bool smj_nav_goal_used(int g, int ncell, const uint16_t* w) { return g >= 0 && g < ncell && w[g] != 0; }

// The 8 neighbours in ascending linear index: k = 0 .. 7 -> (dy, dx); odd |dy| + |dx| = axial.
SMJ_GRID_HD int smj_nav_dy(int k) { return k < 3 ? -1 : k < 5 ? 0 : 1; }
SMJ_GRID_HD int smj_nav_dx(int k) { return k < 3 ? k - 1 : k == 3 ? -1 : k == 4 ? 1 : k - 6; }

// The 8 neighbours of (y, x): n[k] is neighbour k's linear index -- the cell's own where the neighbour lies outside the grid, so that
// every n[k] may be read without a branch -- and wn[k] its stored weight, 0 outside the grid, with a diagonal neighbour whose move
// does not exist set to 0 as well: wn[k] != 0 iff the move from (y, x) to neighbour k exists (given that (y, x) itself is passable).
// All eight reads are issued before any is used: a walk is a chain of dependent cells, and its pace is the latency of one read.
struct smj_nav_nbr_t { int n[8], wn[8]; };
SMJ_GRID_HD smj_nav_nbr_t smj_nav_neighbours(const uint16_t* w, int nx, int ny, int y, int x) {
  smj_nav_nbr_t b;
  const int c = y * nx + x;
  const int up = y > 0 ? -nx : 0, down = y + 1 < ny ? nx : 0, left = x > 0 ? -1 : 0, right = x + 1 < nx ? 1 : 0;
  bool in[8];
  for (int k = 0; k < 8; k++) {
    const int dy = smj_nav_dy(k), dx = smj_nav_dx(k);
    const int oy = dy < 0 ? up : dy > 0 ? down : 0, ox = dx < 0 ? left : dx > 0 ? right : 0;
    in[k] = (dy == 0 || oy != 0) && (dx == 0 || ox != 0);
    b.n[k] = in[k] ? c + oy + ox : c;
  }
  int raw[8];
  for (int k = 0; k < 8; k++) raw[k] = w[b.n[k]];
  for (int k = 0; k < 8; k++) b.wn[k] = in[k] ? raw[k] : 0;
  if (!smj_nav_diagonal_open(b.wn[3], b.wn[1])) b.wn[0] = 0;
  if (!smj_nav_diagonal_open(b.wn[4], b.wn[1])) b.wn[2] = 0;
  if (!smj_nav_diagonal_open(b.wn[3], b.wn[6])) b.wn[5] = 0;
  if (!smj_nav_diagonal_open(b.wn[4], b.wn[6])) b.wn[7] = 0;
  return b;
}

// Relax one cell from its neighbours: potential[c] = min(potential[c], min over the moves of c of move + potential[n]), reading the
// neighbours' current values (stale ones are fine: values only fall).  Returns whether the cell's value fell.  An impassable cell
// never changes; a goal holds 0 and cannot fall.
template <class P>
SMJ_GRID_HD bool smj_nav_relax(P& pot, const uint16_t* w, int nx, int ny, int y, int x) {
  const int c = y * nx + x, wc = w[c];
  if (!wc) return false;
  const smj_nav_nbr_t b = smj_nav_neighbours(w, nx, ny, y, x);
  const int old = pot.get(c);
  int pn[8];
  for (int k = 0; k < 8; k++) pn[k] = pot.get(b.n[k]);
  int best = old;
  for (int k = 0; k < 8; k++) {
    const int cand = pn[k] + smj_nav_move(wc, b.wn[k], smj_nav_dy(k) != 0 && smj_nav_dx(k) != 0);
    if (b.wn[k] && pn[k] < SMJ_NAV_NONE && cand < best) best = cand;
  }
  if (best < old) { pot.set(c, best); return true; }
  return false;
}

// next of one cell, from the converged potential: -1 where there is no path, the cell itself on a goal (potential 0: every move
// costs at least 10), else the neighbour with the smallest move + potential, the first of equals in ascending linear index.
template <class P>
SMJ_GRID_HD int smj_nav_next(const P& pot, const uint16_t* w, int nx, int ny, int y, int x) {
  const int c = y * nx + x, wc = w[c];
  if (!wc) return -1;
  const int own = pot.get(c);
  if (own >= SMJ_NAV_NONE) return -1;
  if (own == 0) return c;
  const smj_nav_nbr_t b = smj_nav_neighbours(w, nx, ny, y, x);
  int pn[8];
  for (int k = 0; k < 8; k++) pn[k] = pot.get(b.n[k]);
  int best = 0x7fffffff, at = -1;
  for (int k = 0; k < 8; k++) {
    const int sum = pn[k] + smj_nav_move(wc, b.wn[k], smj_nav_dy(k) != 0 && smj_nav_dx(k) != 0);
    if (b.wn[k] && pn[k] < SMJ_NAV_NONE && sum < best) { best = sum; at = b.n[k]; }
  }
  return at;
}

// The schedule.  Sweep s relaxes every cell once forward and once backward along lines: the rows for even s, the columns for odd s.
// A line is cut into runs of equal length (the last one may be shorter), each owned by one thread for the whole sweep, which walks
// it from its first cell to its last and back.  Runs per line: one -- the thread owns the whole line, and a value crosses a free
// corridor along it within one sweep, whatever its length -- unless there are so few lines that threads would idle AND the lines are
// long: then as many runs as there are threads per line, of at least SMJ_NAV_MIN_RUN cells each.  (A grid of 4 x 4096 has 4 columns
// of 4096 cells: 32 runs of 128.  A value then crosses a run per sweep, in sweeps 32 times shorter.)  128 x 128 keeps whole lines.
// smj_nav_lines: the lines of sweep s; smj_nav_line_len: their length; smj_nav_line_cell: the (y, x) of position i on line l;
// smj_nav_runs: the runs per line; run r of the sweep is run r % runs of line r / runs, the positions [i0, i1) of smj_nav_run.
enum { SMJ_NAV_MIN_RUN = 128 };
SMJ_GRID_HD int smj_nav_lines(int nx, int ny, int s) { return s & 1 ? nx : ny; }
SMJ_GRID_HD int smj_nav_line_len(int nx, int ny, int s) { return s & 1 ? ny : nx; }
SMJ_GRID_HD void smj_nav_line_cell(int s, int l, int i, int* y, int* x) {
  if (s & 1) { *y = i; *x = l; }
  else { *y = l; *x = i; }
}
SMJ_GRID_HD int smj_nav_runs(int nx, int ny, int s, int nthreads) {
  const int per_line = nthreads / smj_nav_lines(nx, ny, s), by_len = smj_nav_line_len(nx, ny, s) / SMJ_NAV_MIN_RUN;
  const int r = per_line < by_len ? per_line : by_len;
  return r < 1 ? 1 : r;
}
SMJ_GRID_HD void smj_nav_run(int nx, int ny, int s, int runs, int r, int* l, int* i0, int* i1) {
  const int len = smj_nav_line_len(nx, ny, s), per = (len + runs - 1) / runs;
  *l = r / runs;
  *i0 = (r - *l * runs) * per;
  *i1 = *i0 + per < len ? *i0 + per : len;
}
// One thread's walk of the positions [i0, i1) of line l in sweep s: forward over i0 .. i1 - 1, backward over i1 - 2 .. i0.  Returns
// whether any cell fell.
template <class P>
SMJ_GRID_HD bool smj_nav_walk_run(P& pot, const uint16_t* w, int nx, int ny, int s, int l, int i0, int i1) {
  bool changed = false;
  int y, x;
  for (int i = i0; i < i1; i++) {
    smj_nav_line_cell(s, l, i, &y, &x);
    changed |= smj_nav_relax(pot, w, nx, ny, y, x);
  }
  for (int i = i1 - 2; i >= i0; i--) {
    smj_nav_line_cell(s, l, i, &y, &x);
    changed |= smj_nav_relax(pot, w, nx, ny, y, x);
  }
  return changed;
}
// The hard bound on the number of sweeps: every sweep relaxes every cell at least once from values no older than the previous
// sweep's, so after k sweeps every cell whose cheapest path has at most k moves is final, and a path has fewer than nx ny moves.
SMJ_GRID_HD int smj_nav_max_sweeps(int nx, int ny) { return nx * ny; }

#if defined(__HIPCC__)
// Launch (smj_nav.hip).  cost and next may be null.
void smj_launch_nav(int num_envs, const uint8_t* cost, const int* goal, int num_goals, int nx, int ny, int lethal, int neutral,
                    int* potential, int* next, hipStream_t stream);
#endif
