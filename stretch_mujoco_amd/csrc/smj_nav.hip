// smj_costmap_to_navigation: a uint8 cost layer and up to 64 goal cells per env -> per cell the cheapest path cost to a goal (the
// navigation function) and, if wanted, the neighbour to step to (smj_nav.h has the predicate, the move cost, the diagonal rule, the
// relaxation of one cell, next of one cell and the schedule).  One kernel, integers only, no read-modify-write, no workspace:
// the potential is relaxed until nothing changes, and the fixed point of "every cell is the minimum over its moves" is unique, so the
// arrays do not depend on the schedule, on which stale values a thread happened to read, or on the storage mode, and two calls give
// identical bits.
//
// Grid.  One workgroup of 256 threads per env.  (1) The workgroup reads the env's cost bytes once, consecutive lanes consecutive
// bytes, and keeps per cell the uint16 weight neutral + cost, 0 for an impassable cell, in LDS; the potential starts as SMJ_NAV_NONE
// and the used goals get 0.  (2) Sweeps until one changes nothing.  (3) The stores.
//
// Storage.  A grid of at most SMJ_NAV_LDS_CELLS = 16384 cells (128 x 128, the default costmap) keeps its potential in LDS: 64 KiB of
// int32 beside 32 KiB of weights, 96 KiB and a few bytes for the workgroup-wide OR, so ONE workgroup per CU (a CU has 160 KiB; two
// would need 80 KiB each, which the potential and one byte per cell alone already fill).  A larger grid, up to 65536 cells, keeps
// 128 KiB of weights in LDS -- one workgroup per CU again -- and relaxes in potential_dev itself, 256 KiB per env, which stays in L2.
// Both run the same code, templated on where the potential lives; every access to it is a relaxed atomic load / store at workgroup
// scope on the global path (the workgroup's waves share the CU's L1, so nothing bypasses a cache), a plain load / store in LDS, and
// a barrier separates the sweeps: the compiler keeps no neighbour's value in a register across them.  Each cell is written by one
// thread per sweep only, values only fall, and a stale read only delays a fall: hence no read-modify-write.
//
// Schedule (smj_nav_walk_run).  Sweep s walks lines: the rows for even s, the columns for odd s.  A thread owns a whole line for the
// sweep (lines t, t + 256, ..) and relaxes it from its first cell to its last and back.  A value therefore crosses a free corridor
// along a line in one sweep, whatever its length, and turns a corner with the next sweep: the serpentine of 128 x 128 (8256
// reachable cells, 8256 sweeps of plain Jacobi) takes 64 sweeps, a free grid 3, a 30 % random map 20 (host harness, lock step:
// profiles/navigation_cost.txt).  The price: only max(nx, ny) threads work (128 of 256 at 128 x 128), each serially over its line.
// Only where threads would idle AND the lines are long is a line cut into runs of at least 128 cells, one thread each (4 x 4096:
// 32 runs per column).
// Tried and dropped: the first version walked whole lines always and read a neighbour's potential only where the move exists (a
// branch per neighbour, the eight reads waiting for one another).  The 4 x 4096 maps of the GPU test -- the serpentine among them,
// 2018 sweeps, every other one four threads walking 8191 cells -- took 18.3 s with it and take 1.8 s now, most of that the test's own
// reference (both changes together; the same arrays).  Now all eight weights and all eight potentials are read without a branch,
// an outside neighbour standing in as the cell itself.  Considered and not built: runs shorter than a line on the square grids (more
// threads busy, but a corridor then takes one sweep per run: the serpentine's sweeps multiply by the runs per row); all four
// directions at once by four groups of threads (a cell would have several writers per sweep, and a late larger store could undo a
// smaller one: the ownership rule is what makes plain stores safe); dynamic LDS sized by the grid, which would let six 64 x 64
// envs share a CU.
//
// Termination.  A sweep relaxes every cell; __syncthreads_or of "one of my cells fell" ends the loop after the first sweep without a
// fall -- that sweep stored nothing, so each of its reads saw the final values.  The loop is bounded by nx ny sweeps
// (smj_nav_max_sweeps): a cheapest path has fewer moves than that, so the bound never changes a result.
//
// Stores.  A thread owns one 16-byte group of an output -- four consecutive cells whose first address is a multiple of 16, wherever
// the buffer starts -- and stores an int4; the groups cut by the env's ends store their cells one by one.  In global mode the
// potential is already in place.  next is computed in this pass from the converged potential, only when wanted.
//
// Measured (profiles/navigation_cost.txt, 4096 envs, lethal 253, neutral 50, potential alone; next adds 1 - 15 %): the inflated
// costmap of a lidar scan 6.7 ms at 64 x 64, 18.2 ms at 128 x 128, 36.3 ms at 256 x 256; an empty map 4.3 / 11.6 / 24.2 ms; 30 %
// lethal with random costs 17.7 / 85 / 353 ms; the serpentine 70 / 287 / 1136 ms.  smj_occupancy_to_distance on the scan's grid,
// R = 0, takes 0.29 / 1.72 / 6.19 ms: this kernel is 6 - 23 x dearer on the scan and far dearer on mazes.  The empty 128 x 128 grid
// gives the pace of the walk: 3 sweeps of 255 steps per env, 16 envs per CU one after the other, about 0.9 us per cell -- a chain of
// dependent instructions with one workgroup on the CU and nothing to hide it.  Plain LDS loads instead of atomic ones (NavPot) let the
// eight reads issue together and moved that grid from 11.7 to 11.6 ms: the chain is bound by its instructions, not by those waits.
#include "smj_nav.h"

static constexpr int NAV_THREADS = 256;

struct NavArgs {
  const uint8_t* cost;
  const int* goal;
  int* potential;
  int* next;
  int num_goals, nx, ny, lethal, neutral;
};

// The potential.  In potential_dev every access is a relaxed atomic at workgroup scope.  In LDS the loads and stores are plain ones,
// so that the eight neighbour reads of a cell issue together and are waited for once (as atomics the compiler kept them in program
// order with a wait after each: the walk, a chain of dependent cells, ran at a third of the pace); the barrier between sweeps still
// forces every value to be read again, and within a sweep a value the compiler kept is merely a stale one.
template <bool LDS>
struct NavPot {
  int* p;
  __device__ __forceinline__ int get(int c) const { return LDS ? p[c] : __hip_atomic_load(p + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  __device__ __forceinline__ void set(int c, int v) {
    if (LDS) p[c] = v;
    else __hip_atomic_store(p + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};

// one output of an env by 16-byte groups; value(c) gives cell c's int
template <class F>
__device__ __forceinline__ void nav_store(int* out, int ncell, int tid, F value) {
  const int al = (int)(((uintptr_t)out >> 2) & 3u);
  const int ngroups = smj_grid_groups(ncell);
  for (int k = tid; k < ngroups; k += NAV_THREADS) {
    const int first = smj_grid_group_first(k, al);
    if (first >= ncell) continue;
    if (first >= 0 && first + 4 <= ncell) {
      *reinterpret_cast<int4*>(out + first) = make_int4(value(first), value(first + 1), value(first + 2), value(first + 3));
    } else {
      for (int i = 0; i < 4; i++) {
        const int c = first + i;
        if (c >= 0 && c < ncell) out[c] = value(c);
      }
    }
  }
}

template <bool LDS>
__global__ __launch_bounds__(NAV_THREADS) void smj_nav_kernel(const NavArgs a) {
  __shared__ uint16_t w[LDS ? SMJ_NAV_LDS_CELLS : SMJ_NAV_MAX_CELLS];
  __shared__ int lpot[LDS ? SMJ_NAV_LDS_CELLS : 1];
  const int tid = threadIdx.x, env = blockIdx.x;
  const int nx = a.nx, ny = a.ny, ncell = nx * ny;   // <= SMJ_NAV_MAX_CELLS, and <= SMJ_NAV_LDS_CELLS if LDS
  const long long e0 = (long long)env * ncell;
  int* gpot = a.potential + e0;
  NavPot<LDS> pot{LDS ? lpot : gpot};

  // (1) weights, the empty potential, the goals
  const uint8_t* cost = a.cost ? a.cost + e0 : nullptr;
  for (int c = tid; c < ncell; c += NAV_THREADS) {
    w[c] = smj_nav_weight(cost ? cost[c] : 0, a.lethal, a.neutral);
    pot.set(c, SMJ_NAV_NONE);
  }
  __syncthreads();
  if (tid < a.num_goals) {
    const int g = a.goal[(long long)env * a.num_goals + tid];
    if (smj_nav_goal_used(g, ncell, w)) pot.set(g, 0);
  }
  __syncthreads();

  // (2) sweeps until one changes nothing
  const int smax = smj_nav_max_sweeps(nx, ny);
  for (int s = 0; s < smax; s++) {
    bool changed = false;
    const int runs = smj_nav_runs(nx, ny, s, NAV_THREADS), items = smj_nav_lines(nx, ny, s) * runs;
    for (int r = tid; r < items; r += NAV_THREADS) {
      int l, i0, i1;
      smj_nav_run(nx, ny, s, runs, r, &l, &i0, &i1);
      changed |= smj_nav_walk_run(pot, w, nx, ny, s, l, i0, i1);
    }
    if (!__syncthreads_or(changed)) break;   // its barrier also stands between this sweep's stores and the next one's loads
  }

  // (3) the stores
  if (LDS) nav_store(gpot, ncell, tid, [&](int c) { return lpot[c]; });
  if (a.next) {
    nav_store(a.next + e0, ncell, tid, [&](int c) {
      const int y = c / nx;
      return smj_nav_next(pot, w, nx, ny, y, c - y * nx);
    });
  }
}

void smj_launch_nav(int num_envs, const uint8_t* cost, const int* goal, int num_goals, int nx, int ny, int lethal, int neutral,
                    int* potential, int* next, hipStream_t stream) {
  NavArgs a;
  a.cost = cost; a.goal = goal; a.potential = potential; a.next = next;
  a.num_goals = num_goals; a.nx = nx; a.ny = ny; a.lethal = lethal; a.neutral = neutral;
  const dim3 grid((unsigned)num_envs), block(NAV_THREADS);
  if (nx * ny <= SMJ_NAV_LDS_CELLS) hipLaunchKernelGGL(smj_nav_kernel<true>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(smj_nav_kernel<false>, grid, block, 0, stream, a);
}
