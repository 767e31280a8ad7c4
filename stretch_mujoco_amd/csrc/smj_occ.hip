// smj_lidar_to_occupancy: the lidar scan -> per-cell counts of rays that end in a cell (hit) and of rays that pass through it (miss)
// on a 2-D grid in the world or a body frame (smj_occ.h has the ray, the classification and the closed-form line; smj_hmap.h the
// bands; smj_scan.h what the scan entries share: the source of the rays and the store of a band).  One kernel, no global atomics, no
// workspace: both reductions are integer sums done in LDS and the band is stored once, so the arrays do not depend on any order and
// two calls give identical bits.
//
// Grid.  One workgroup per (env, band).  The band's cells live in LDS as two int32 arrays.  The workgroup (1) sets its cells to zero,
// or with accumulate to what the outputs hold, while thread k turns ray k into a record in LDS: the pose of the site's body and of
// the frame's body read from XPOSE, origin and direction by smj_occ_ray, the range classified, the cells of the two ends by
// smj_occ_line -- all float arithmetic of a ray is done once, by one lane; a ray whose box of cells misses the band is marked
// dropped there; (2) walks the rays, integer arithmetic only, and adds 1 per visited cell of its band with no-return LDS atomics;
// (3) after a barrier stores the band, lane-contiguous (16 bytes per lane where the address allows it).  Nothing but the two
// outputs is written.
//
// Band size and workgroup size.  8 bytes per cell as the height map, so the same cut: 4096 cells (32 KiB), a 64 x 64 grid is ONE
// band; the ray records take 20 bytes x 384 more, 39.5 KiB in all, four workgroups per CU.  A scan is 360 rays and at 5 cm a ray is
// 20 - 200 cells long: 30 000 - 70 000 adds per env and band, no global traffic but 1.4 KB of ranges in and the band out.  256
// threads walk that in 120 - 270 adds each; more threads would shorten the walk but not the two barriers and the store, and four
// workgroups of four wavefronts already give every SIMD four wavefronts to hide the integer division of the line in.
//
// Split of the work: lanes over (ray, i), in groups of 32 lanes per ray.  Lane l of a group takes the cells i = l, l + 32, .. of
// its ray (the closed form of smj_occ_cell needs no predecessor), the eight groups take the rays k = g, g + 8, ...  Against a lane
// per ray: (a) the rays of a scan differ in length by a factor of ten (a wall at 0.5 m beside a corridor), and a wavefront of
// 64 rays runs as long as its longest; with groups the idle lanes are those of the last 32 cells of a ray only; (b) the lanes of a
// group touch consecutive cells of one line, which are different LDS words -- a lane per ray sends, at i = 0, all 64 lanes of a
// wavefront to the ONE cell the laser sits in.  A flat split over all (ray, i) pairs of the scan balances perfectly but needs a
// prefix sum over the rays and a search per pair; groups need neither.  32 rather than 64 lanes: at 5 cm and the reference's
// 5 m cutoff half of the rays are shorter than 64 cells.
//
// The origin cell.  All rays start in one cell, so it takes 360 adds per scan.  With groups these arrive one per ray -- at most two
// in one wavefront instruction (its two groups), against 64 with a lane per ray -- so a pre-merge would save at most one serialised
// replay per 64 lanes of work: 1 % of the adds.  It would cost a compare of every ray's first cell with a shared one (the sites may
// differ) and a second code path for rays whose origin is elsewhere.  Not built: the split already removed what it would remove.
//
// Measured (profiles/occupancy_cost.txt, 4096 envs, 5 cm cells): 0.19 ms per 64 x 64 grid with ranges to 5 m, of which 0.04 ms are start
// values, ray records and the store (the call without a miss layer); 0.67 ms for 128 x 128.  A longer r_max costs more on the same grid
// (0.25 / 0.88 ms to 9.5 m): the walk evaluates the cells a ray has outside the band before it skips them.  The closed form would give
// the i-range inside a band directly; that is not done here.
#include "smj_occ.h"
#include "smj_scan.h"

static constexpr int OCC_THREADS = 256;
static constexpr int OCC_GROUP = 32;        // lanes per ray
static constexpr int OCC_MAX_RAYS = 384;    // the capacity of smj_lidar_kernel (smj_create refuses a model with more)

struct OccArgs {
  SmjScanSource src;   // smj_scan.h
  int* hit;
  int* miss;
  int nlidar, kind, body, nx, ny, no_return_clears, accumulate, bands;
  float x0, y0, inv_cell, r_min, r_max;
};

__global__ __launch_bounds__(OCC_THREADS) void smj_occ_kernel(const OccArgs a) {
  __shared__ unsigned hits[SMJ_OCC_BAND_CELLS];
  __shared__ unsigned misses[SMJ_OCC_BAND_CELLS];
  __shared__ smj_occ_line_t rays[OCC_MAX_RAYS];
  const int tid = threadIdx.x;
  const int env = blockIdx.x / a.bands, band = blockIdx.x - env * a.bands;
  const smj_hmap_band_t b = smj_hmap_band(a.nx, a.ny, SMJ_OCC_BAND_CELLS, band);
  const int ncell = b.rows * b.cols;   // <= SMJ_OCC_BAND_CELLS
  const long long g0 = (long long)env * a.nx * a.ny + (long long)b.r0 * a.nx + b.c0;   // the band's first cell in the outputs
  int* ho = a.hit + g0;
  int* mo = a.miss ? a.miss + g0 : nullptr;

  // (1) start values and ray records
  if (a.accumulate) {
    for (int c = tid; c < ncell; c += OCC_THREADS) {
      hits[c] = (unsigned)ho[c];
      misses[c] = mo ? (unsigned)mo[c] : 0u;
    }
  } else {
    for (int c = tid; c < ncell; c += OCC_THREADS) {
      hits[c] = 0u;
      misses[c] = 0u;
    }
  }
  for (int k = tid; k < a.nlidar; k += OCC_THREADS) {
    const SmjScanSource& s = a.src;
    const int sid = s.lidar_site[k], sb = s.site_bodyid[sid];
    float bp[3], bm[9], fp[3] = {}, fm[9] = {}, o[2], d[2], len;
    for (int j = 0; j < 3; j++) bp[j] = s.xpose[(12 * sb + j) * s.ld + env];
    for (int j = 0; j < 9; j++) bm[j] = s.xpose[(12 * sb + 3 + j) * s.ld + env];
    if (a.kind == SMJ_OCC_BODY) {
      for (int j = 0; j < 3; j++) fp[j] = s.xpose[(12 * a.body + j) * s.ld + env];
      for (int j = 0; j < 9; j++) fm[j] = s.xpose[(12 * a.body + 3 + j) * s.ld + env];
    }
    const float lz[3] = {s.site_mat[9 * sid + 2], s.site_mat[9 * sid + 5], s.site_mat[9 * sid + 8]};
    smj_occ_ray(a.kind, bp, bm, s.site_pos + 3 * sid, lz, fp, fm, o, d);
    const int cls = smj_occ_classify(s.lidar[(long long)k * s.lidar_ld + env], a.r_min, a.r_max, a.no_return_clears, &len);
    smj_occ_line_t L = smj_occ_line(cls, o, d, len, a.x0, a.y0, a.inv_cell);
    // the line stays inside the box of its two ends: a ray whose box misses the band adds nothing here
    const int xl = min(L.ax, L.bx), xh = max(L.ax, L.bx), yl = min(L.ay, L.by), yh = max(L.ay, L.by);
    if (xh < b.c0 || xl >= b.c0 + b.cols || yh < b.r0 || yl >= b.r0 + b.rows) L.kind = SMJ_OCC_DROP;
    rays[k] = L;
  }
  __syncthreads();

  // (2) walk the rays
  if (mo) {
    const int grp = tid / OCC_GROUP, lane = tid - grp * OCC_GROUP;
    for (int k = grp; k < a.nlidar; k += OCC_THREADS / OCC_GROUP) {
      const smj_occ_line_t L = rays[k];
      if (L.kind == SMJ_OCC_DROP) continue;
      const int n = smj_occ_steps(L);
      for (int i = lane; i <= n; i += OCC_GROUP) {
        int ix, iy;
        smj_occ_cell(L, n, i, &ix, &iy);
        const int slot = smj_hmap_slot(b, ix, iy);   // -1 for every cell outside the band, so outside the grid too
        if (slot >= 0) atomicAdd(smj_occ_layer(L, n, i) ? &hits[slot] : &misses[slot], 1u);   // result unused: no-return LDS atomic
      }
    }
  } else {
    // without a miss layer only the last cell of a return counts: a lane per ray
    for (int k = tid; k < a.nlidar; k += OCC_THREADS) {
      const smj_occ_line_t L = rays[k];
      if (L.kind != SMJ_OCC_RETURN) continue;
      const int slot = smj_hmap_slot(b, L.bx, L.by);
      if (slot >= 0) atomicAdd(&hits[slot], 1u);
    }
  }
  __syncthreads();

  // (3) store the band once
  smj_scan_store_band<OCC_THREADS, false>(ho, hits, ncell, tid);
  if (mo) smj_scan_store_band<OCC_THREADS, false>(mo, misses, ncell, tid);
}

void smj_launch_occ(const SmjScanSource& src, int num_envs, int nlidar, int kind, int body, float x0, float y0, float cell, int nx, int ny,
                    float r_min, float r_max, int no_return_clears, int accumulate, int* hit, int* miss, hipStream_t stream) {
  OccArgs a;
  a.src = src; a.hit = hit; a.miss = miss;
  a.nlidar = nlidar; a.kind = kind; a.body = body; a.nx = nx; a.ny = ny; a.no_return_clears = no_return_clears; a.accumulate = accumulate;
  a.bands = smj_hmap_bands(nx, ny, SMJ_OCC_BAND_CELLS);
  a.x0 = x0; a.y0 = y0; a.inv_cell = 1.f / cell; a.r_min = r_min; a.r_max = r_max;
  const dim3 grid((unsigned)((long long)num_envs * a.bands)), block(OCC_THREADS);
  hipLaunchKernelGGL(smj_occ_kernel, grid, block, 0, stream, a);
}
