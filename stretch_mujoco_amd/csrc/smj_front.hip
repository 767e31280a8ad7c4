// smj_occupancy_to_frontiers: the hit / miss counts of an occupancy grid (and, if given, a uint8 cost layer) -> per cell the label of
// its frontier region, and per env the goal cells, sizes and coordinate sums of the largest regions (smj_front.h has the state of a
// cell, the frontier predicate, find / union, the jump, the schedule, the codes of a root's slot and the representative's key).  One
// kernel, integers only, no workspace.  Every output is defined without reference to an order -- the smallest index of a component,
// exact integer sums, a total order of the regions, the smallest index among equal keys -- so the arrays do not depend on which thread
// won a compare-and-swap, on stale reads or on the storage mode, and two calls give identical bits.
//
// Grid.  One workgroup of 256 threads per env; every pass hands cell k 256 + t to thread t in its round k (consecutive lanes,
// consecutive words) and passes are separated by barriers.  The env's grid has ONE int32 word per cell, which holds in turn:
//   (1) the cell's state code, from one coalesced read of hit, miss and cost;
//   (2) the code plus the frontier flag, from the codes of the 4 neighbours (a writer keeps the code's bits, so no copy is needed);
//   (3) the label: the cell's own index on the frontier, -1 off it;
//   (4) the union of every frontier cell with its backward neighbours W, NW, N, NE (compare-and-swap on roots, path halving);
//   (5) jumps label[c] = label[label[c]] until a round changes nothing (at most 17 rounds): every cell holds its root -- label_dev;
//   (6) in the roots' slots the regions' sizes (-1 - size, integer atomic adds), from which the kept regions are counted and the
//       largest max_regions chosen, one workgroup-wide arg-max per row: every thread keeps the best key among its own roots and
//       only the winner rescans its cells, so a row costs two atomics and a barrier for all threads but one;
//   (7) in the chosen roots' slots their row: one pass adds up x and y per row, one takes the minimum of the representative's key
//       (64-bit atomic min in LDS), one the smallest cell among those that have it.
// Storage.  Up to SMJ_FRONT_LDS_CELLS = 16384 cells (128 x 128, the default map) the words live in LDS: 64 KiB, so two workgroups
// share a CU (smj_front.h has the reason for the limit); label_dev is stored after (5) through the 16-byte groups of smj_grid.h and
// (6), (7) then scribble over the LDS copy.  Above it, up to 65536 cells, the words are label_dev itself, 256 KiB per env that stay
// in L2; (6) and (7) borrow the roots' slots and the last pass puts label[r] = r back.  Both run the same code, templated on the
// accessor: relaxed atomic loads, stores and read-modify-writes, at workgroup scope in LDS and at agent scope in label_dev (its
// read-modify-writes are done in L2, so the loads go there too instead of to a line of the CU's L1 that predates them).
// Termination.  find, union and the jumps have hard bounds, proved beside them in smj_front.h; the selection has max_regions rows.
#include "smj_front.h"

static constexpr int FRONT_THREADS = 256;

struct FrontArgs {
  const int* hit;
  const int* miss;
  const uint8_t* cost;
  int* label;
  int* goal;
  int* region;
  int* count;
  int nx, ny, min_hits, lethal, min_size, max_regions;
};

template <bool LDS>
struct FrontLab {
  int* p;
  static constexpr int SCOPE = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
  __device__ __forceinline__ int get(int c) const { return __hip_atomic_load(p + c, __ATOMIC_RELAXED, SCOPE); }
  __device__ __forceinline__ void set(int c, int v) { __hip_atomic_store(p + c, v, __ATOMIC_RELAXED, SCOPE); }
  __device__ __forceinline__ int cas(int c, int expected, int v) {
    __hip_atomic_compare_exchange_strong(p + c, &expected, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE);
    return expected;   // the value found, whether or not the swap took place
  }
  __device__ __forceinline__ int add(int c, int v) { return __hip_atomic_fetch_add(p + c, v, __ATOMIC_RELAXED, SCOPE); }
};

// one output of an env by 16-byte groups; value(c) gives cell c's int
template <class F>
__device__ __forceinline__ void front_store(int* out, int ncell, int tid, F value) {
  const int al = (int)(((uintptr_t)out >> 2) & 3u);
  const int ngroups = smj_grid_groups(ncell);
  for (int k = tid; k < ngroups; k += FRONT_THREADS) {
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
__global__ __launch_bounds__(FRONT_THREADS) void smj_front_kernel(const FrontArgs a) {
  __shared__ int words[LDS ? SMJ_FRONT_LDS_CELLS : 1];
  __shared__ unsigned long long s_order[SMJ_FRONT_MAX_REGIONS], s_rep[SMJ_FRONT_MAX_REGIONS];
  __shared__ int s_label[SMJ_FRONT_MAX_REGIONS], s_size[SMJ_FRONT_MAX_REGIONS], s_sx[SMJ_FRONT_MAX_REGIONS], s_sy[SMJ_FRONT_MAX_REGIONS],
      s_goal[SMJ_FRONT_MAX_REGIONS], s_count[2];
  const int tid = threadIdx.x, env = blockIdx.x;
  const int nx = a.nx, ny = a.ny, ncell = nx * ny;   // <= SMJ_FRONT_MAX_CELLS, and <= SMJ_FRONT_LDS_CELLS if LDS
  const int rounds = smj_front_rounds(ncell, FRONT_THREADS), G = a.max_regions;
  const long long e0 = (long long)env * ncell;
  int* glabel = a.label + e0;
  FrontLab<LDS> lab{LDS ? words : glabel};
  // the cells of this thread, in the schedule's order
#define FRONT_MY_CELLS(c) for (int k_ = 0, c = tid; k_ < rounds && (c = smj_front_cell(tid, k_, FRONT_THREADS)) < ncell; k_++)

  // (1) the codes
  const int* hit = a.hit + e0;
  const int* miss = a.miss + e0;
  const uint8_t* cost = a.cost ? a.cost + e0 : nullptr;
  // four rounds at a time, every load issued before the first is used: this pass is the kernel's only global read, and one
  // round per wait left it waiting for memory 64 times per 128 x 128 grid
  for (int k0 = 0; k0 < rounds; k0 += 4) {
    int h[4], m[4], q[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int c = smj_front_cell(tid, k0 + j, FRONT_THREADS), at = c < ncell ? c : ncell - 1;   // a stand-in inside the grid: no branch around a load
      h[j] = hit[at];
      m[j] = miss[at];
      q[j] = cost ? cost[at] : 0;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int c = smj_front_cell(tid, k0 + j, FRONT_THREADS);
      if (c < ncell) lab.set(c, smj_front_code(h[j], m[j], q[j], a.min_hits, a.lethal));
    }
  }
  if (tid < SMJ_FRONT_MAX_REGIONS) {
    s_order[tid] = 0;
    s_rep[tid] = ~0ull;
    s_label[tid] = -1;
    s_size[tid] = s_sx[tid] = s_sy[tid] = 0;
    s_goal[tid] = 0x7fffffff;
  }
  if (tid < 2) s_count[tid] = 0;
  __syncthreads();

  // (2) the frontier flag, (3) the labels
  FRONT_MY_CELLS(c) {
    const int code = lab.get(c);
    if (code != SMJ_FRONT_FREE) continue;
    const int y = c / nx;
    if (smj_front_is_frontier(lab, nx, ny, y, c - y * nx)) lab.set(c, code | SMJ_FRONT_FLAG);
  }
  __syncthreads();
  FRONT_MY_CELLS(c) lab.set(c, lab.get(c) & SMJ_FRONT_FLAG ? c : -1);
  __syncthreads();

  // (4) the unions
  FRONT_MY_CELLS(c) {
    if (lab.get(c) < 0) continue;
    const int y = c / nx;
    smj_front_link(lab, nx, y, c - y * nx);
  }
  __syncthreads();

  // (5) jumps until a round changes nothing
  for (int j = 0; j < smj_front_max_jumps(); j++) {
    bool changed = false;
    FRONT_MY_CELLS(c) changed |= smj_front_jump(lab, c);
    if (!__syncthreads_or(changed)) break;
  }
  if (LDS) {
    front_store(glabel, ncell, tid, [&](int c) { return words[c]; });
    __syncthreads();
  }

  // (6) sizes into the roots' slots, the counts, the kept regions in order
  int nfront = 0;
  FRONT_MY_CELLS(c) {
    const int v = lab.get(c);
    nfront += v >= 0;
    if (v == c) lab.set(c, smj_front_size_code(1));
  }
  __syncthreads();
  FRONT_MY_CELLS(c) {
    const int v = lab.get(c);
    if (v >= 0) lab.add(v, -1);   // one more cell: the code -1 - size falls by one
  }
  __syncthreads();
  int nkept = 0;
  const auto best_of_mine = [&](bool count) {
    unsigned long long best = 0;
    FRONT_MY_CELLS(c) {
      const int v = lab.get(c);
      if (!smj_front_is_size_code(v)) continue;
      const int size = smj_front_code_size(v);
      if (size < a.min_size) continue;
      if (count) nkept++;
      const unsigned long long key = smj_front_order_key(size, c);
      best = key > best ? key : best;
    }
    return best;
  };
  unsigned long long mine = best_of_mine(true);
  if (nkept) atomicAdd(&s_count[0], nkept);
  if (nfront) atomicAdd(&s_count[1], nfront);
  int nrows = 0;
  for (int k = 0; k < G; k++) {
    if (mine) atomicMax(&s_order[k], mine);
    __syncthreads();
    const unsigned long long best = s_order[k];
    if (!best) break;   // the same for every thread
    nrows = k + 1;
    if (best == mine) {   // keys differ in their labels: one thread
      const int r = smj_front_key_label(best);
      s_label[k] = r;
      s_size[k] = smj_front_key_size(best);
      lab.set(r, smj_front_row_code(k));
      mine = best_of_mine(false);
    }
  }
  __syncthreads();

  // (7) the sums, the representative's key, the representative
  FRONT_MY_CELLS(c) {
    const int row = smj_front_row_of(lab, lab.get(c));
    if (row < 0) continue;
    const int y = c / nx;
    atomicAdd(&s_sx[row], c - y * nx);
    atomicAdd(&s_sy[row], y);
  }
  __syncthreads();
  FRONT_MY_CELLS(c) {
    const int row = smj_front_row_of(lab, lab.get(c));
    if (row < 0) continue;
    const int y = c / nx;
    atomicMin(&s_rep[row], (unsigned long long)smj_front_rep_key(s_size[row], s_sx[row], s_sy[row], y, c - y * nx));
  }
  __syncthreads();
  FRONT_MY_CELLS(c) {
    const int row = smj_front_row_of(lab, lab.get(c));
    if (row < 0) continue;
    const int y = c / nx;
    if (smj_front_rep_key(s_size[row], s_sx[row], s_sy[row], y, c - y * nx) == s_rep[row]) atomicMin(&s_goal[row], c);
  }
  __syncthreads();

  // the small outputs; label_dev's borrowed roots back in place
  if (tid < G) {
    const bool used = tid < nrows;
    a.goal[(long long)env * G + tid] = used ? s_goal[tid] : -1;
    if (a.region) {
      int* row = a.region + ((long long)env * G + tid) * 4;
      const int4 v = make_int4(s_label[tid], s_size[tid], s_sx[tid], s_sy[tid]);   // -1, 0, 0, 0 on an unused row
      if (((uintptr_t)row & 15u) == 0) *reinterpret_cast<int4*>(row) = v;
      else { row[0] = v.x; row[1] = v.y; row[2] = v.z; row[3] = v.w; }
    }
  }
  if (a.count && tid < 2) a.count[(long long)env * 2 + tid] = s_count[tid];
  if (!LDS) {
    FRONT_MY_CELLS(c) {
      if (lab.get(c) < -1) lab.set(c, c);
    }
  }
#undef FRONT_MY_CELLS
}

void smj_launch_front(int num_envs, const int* hit, const int* miss, const uint8_t* cost, int nx, int ny, int min_hits, int lethal,
                      int min_size, int max_regions, int* label, int* goal, int* region, int* count, hipStream_t stream) {
  FrontArgs a;
  a.hit = hit; a.miss = miss; a.cost = cost; a.label = label; a.goal = goal; a.region = region; a.count = count;
  a.nx = nx; a.ny = ny; a.min_hits = min_hits; a.lethal = lethal; a.min_size = min_size; a.max_regions = max_regions;
  const dim3 grid((unsigned)num_envs), block(FRONT_THREADS);
  if (nx * ny <= SMJ_FRONT_LDS_CELLS) hipLaunchKernelGGL(smj_front_kernel<true>, grid, block, 0, stream, a);
  else hipLaunchKernelGGL(smj_front_kernel<false>, grid, block, 0, stream, a);
}
