// smj_occupancy_to_distance: occupancy counts -> per cell the squared distance (in cells) to the nearest obstacle and that obstacle's
// linear index, ties to the smallest index (smj_edt.h has the predicate, the row and column rules and the cut into strips).  One
// kernel, integers only, no global atomics, no workspace: every cell's value is a minimum over a total order, so the arrays do not
// depend on any order of evaluation and two calls give identical bits.
//
// Grid.  One workgroup of 256 threads per (env, strip of columns).  (1) The workgroup turns the env's WHOLE grid into a bit mask in
// LDS, bit c = cell c (at most 8 KiB): a wavefront reads 64 consecutive cells, 256 contiguous bytes, and its ballot is the word -- no
// atomics.  Every strip of an env repeats this; the grid is at most 256 KiB per layer and the repeats hit in L2.  (2) Per cell of its
// strip a thread finds the nearest set bit to the left and to the right with leading- / trailing-zero counts over the row's words --
// across the strip's edges, the mask being the whole row -- and stores the signed offset as int16 in LDS, [ny][w]; the workgroup also
// reduces the first and last row that holds any offset (shuffles, then the mask's first words once nobody reads it any more).  (3) After a barrier the column search of smj_edt_column
// on the LDS offsets, and the store.
//
// Strip size.  int16 offsets, 16384 cells per strip: 32 KiB, with the mask exactly 40 KiB, so four workgroups share a CU's 160 KiB as
// the occupancy kernel's do -- not one byte of LDS more fits, which is why the row range lives in the mask.
// A 128 x 128 grid is one strip, 256 x 256 four strips of 64 columns.  Strips of columns rather than bands of rows because the
// column search of a cell may need any row of its column but only its own column; what it needs from other columns is in the
// 8 KiB mask.
//
// Store.  A thread owns one 16-byte group of dist2 -- four consecutive cells of a row whose first address is a multiple of 16,
// wherever the buffer starts -- does the four searches and stores an int4; the groups cut by a strip's or the row's ends store their
// cells one by one.  Consecutive lanes own consecutive groups.  nearest takes the same int4 where its address is aligned like
// dist2's (always, for two allocations of their own), scalar stores otherwise; same values.
//
// The column search is the outward search, not a lower-envelope scan (Meijster): outward, a cell stops after about its distance in
// rows, a handful of LDS reads on a map with filled walls; the envelope scan costs O(ny) per column whatever the content, is serial
// per column (w <= 128 threads busy out of 256) and would have to carry the index tie through the envelope's intersections.  What the
// outward search does badly is the sparse grid, two reads per row of distance; the row range [jlo, jhi] that holds any offset takes
// the empty grid (no search at all) and the single obstacle (one read per cell).
//
// Measured (profiles/distance_field_cost.txt, 4096 envs): the occupancy grid of a lidar scan, 28 obstacle cells per env, 0.29 ms at
// 64 x 64 and 1.72 ms at 128 x 128 with R = 0, 0.23 / 0.81 ms with R = 20; an empty grid 0.08 / 0.37 ms, one obstacle in a corner
// 0.12 / 0.51 ms; 256 x 256 (four strips, each rebuilding the mask) 6.2 / 3.1 / 3.0 / 3.5 ms.  The scan's grid costs more than the ray
// walk that produced it (0.19 / 0.65 ms): a lidar grid is the thin outline of what the rays hit, so most cells are tens of rows from
// an obstacle.  A variant that skips the rows without offsets by a row bitmap (512 B more LDS, hence dynamic LDS) gave the same
// arrays and was slower on every input but the corner (128 x 128 scan 2.20 ms, empty 0.52 ms): not kept.
#include "smj_edt.h"

static constexpr int EDT_THREADS = 256;

struct EdtArgs {
  const int* hit;
  const int* miss;
  int* dist2;
  int* nearest;
  int nx, ny, min_hits, unknown_is_obstacle, R, strips;
};

__global__ __launch_bounds__(EDT_THREADS) void smj_edt_kernel(const EdtArgs a) {
  __shared__ unsigned long long mask[SMJ_EDT_MASK_WORDS];
  __shared__ int16_t off[SMJ_EDT_STRIP_CELLS];
  const int tid = threadIdx.x;
  const int env = blockIdx.x / a.strips;
  const smj_edt_strip_t s = smj_edt_strip(a.nx, a.ny, blockIdx.x - env * a.strips);
  const int ncell = a.nx * a.ny;   // <= SMJ_EDT_MAX_CELLS
  const long long e0 = (long long)env * ncell;
  const int* hit = a.hit + e0;
  const int* miss = a.miss ? a.miss + e0 : nullptr;

  // (1) the obstacle mask of the whole grid: wavefront v takes the words v, v + 4, ..
  const int lane = tid & 63, nwords = (ncell + 63) >> 6;
  for (int wi = tid >> 6; wi < nwords; wi += EDT_THREADS / 64) {
    const int c = (wi << 6) + lane;
    bool ob = false;
    if (c < ncell) ob = smj_edt_obstacle(hit[c], miss && a.unknown_is_obstacle ? miss[c] : 1, miss != nullptr, a.min_hits, a.unknown_is_obstacle);
    const unsigned long long word = __ballot(ob);   // cells past the grid's end give 0 bits
    if (lane == 0) mask[wi] = word;
  }
  __syncthreads();

  // (2) the row pass over the strip's cells
  const int nstrip = a.ny * s.w;   // <= SMJ_EDT_STRIP_CELLS
  int jlo = a.ny, jhi = -1;   // first and last row in which this thread stored an offset
  for (int t = tid; t < nstrip; t += EDT_THREADS) {
    const int y = t / s.w, lx = t - y * s.w;
    const int o = smj_edt_row_offset(mask, a.nx, y, s.c0 + lx, a.R);
    off[t] = (int16_t)o;
    if (o != SMJ_EDT_NO_OFF) { jlo = min(jlo, y); jhi = max(jhi, y); }
  }
  for (int d = 32; d > 0; d >>= 1) {
    jlo = min(jlo, __shfl_xor(jlo, d));
    jhi = max(jhi, __shfl_xor(jhi, d));
  }
  __syncthreads();   // the mask has been read for the last time: its first words carry the wavefronts' row ranges
  if (lane == 0) mask[tid >> 6] = ((unsigned long long)(unsigned)jhi << 32) | (unsigned)jlo;
  __syncthreads();
  for (int v = 0; v < EDT_THREADS / 64; v++) {
    const unsigned long long r = mask[v];
    jlo = min(jlo, (int)(unsigned)r);
    jhi = max(jhi, (int)(unsigned)(r >> 32));
  }

  // (3) the column pass: one 16-byte group of dist2 per thread and step
  int* d2 = a.dist2 + e0;
  int* nr = a.nearest ? a.nearest + e0 : nullptr;
  const int gmax = smj_grid_groups(s.w);   // groups a row segment of w cells can touch, whatever its alignment
  const int nitem = a.ny * gmax;
  for (int t = tid; t < nitem; t += EDT_THREADS) {
    const int y = t / gmax, k = t - y * gmax;
    const int g0 = y * a.nx + s.c0;   // the row segment's first cell
    const int al = (int)(((uintptr_t)(d2 + g0) >> 2) & 3u);   // its word offset inside a 16-byte group
    const int l0 = smj_grid_group_first(k, al);   // first cell of the group, relative to the segment
    if (l0 >= s.w) continue;
    int d[4] = {0, 0, 0, 0}, n[4] = {0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
      const int lx = l0 + i;
      if (lx >= 0 && lx < s.w) smj_edt_column(off + lx, s.w, a.nx, y, s.c0 + lx, jlo, jhi, a.R, &d[i], &n[i]);
    }
    if (l0 >= 0 && l0 + 4 <= s.w) {
      *reinterpret_cast<int4*>(d2 + g0 + l0) = make_int4(d[0], d[1], d[2], d[3]);
      if (nr) {
        if ((((uintptr_t)(nr + g0 + l0)) & 15u) == 0) *reinterpret_cast<int4*>(nr + g0 + l0) = make_int4(n[0], n[1], n[2], n[3]);
        else for (int i = 0; i < 4; i++) nr[g0 + l0 + i] = n[i];
      }
    } else {
      for (int i = 0; i < 4; i++) {
        const int lx = l0 + i;
        if (lx >= 0 && lx < s.w) {
          d2[g0 + lx] = d[i];
          if (nr) nr[g0 + lx] = n[i];
        }
      }
    }
  }
}

void smj_launch_edt(int num_envs, const int* hit, const int* miss, int nx, int ny, int min_hits, int unknown_is_obstacle, int R,
                    int* dist2, int* nearest, hipStream_t stream) {
  EdtArgs a;
  a.hit = hit; a.miss = miss; a.dist2 = dist2; a.nearest = nearest;
  a.nx = nx; a.ny = ny; a.min_hits = min_hits; a.unknown_is_obstacle = unknown_is_obstacle; a.R = R;
  a.strips = smj_edt_strips(nx, ny);
  const dim3 grid((unsigned)((long long)num_envs * a.strips)), block(EDT_THREADS);
  hipLaunchKernelGGL(smj_edt_kernel, grid, block, 0, stream, a);
}
