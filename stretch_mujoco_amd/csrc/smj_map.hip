// smj_scan_to_map: the lidar scan and a pose of every env handed in -> per-cell counts of rays that end in a cell (hit) and of rays
// that pass through it (miss) on a 2-D grid in the frame of that pose (smj_map.h has the status, the line of a ray and the part of a
// line inside a band; smj_occ.h the ray, the classification and the closed-form line; smj_hmap.h the bands; smj_scan.h the source
// of the rays and the store of a band, with smj_occ.hip).  One kernel, no global atomics, no workspace: both reductions are
// integer sums done in LDS and the band is stored once, so the arrays do not depend on any order and two calls give identical bits.
//
// Grid.  The layout smj_occ.hip measured its way to: one workgroup of 256 threads per (env, band of 4096 cells), the band's cells
// in LDS as two int32 arrays, ray records built once in LDS by one lane each, groups of 32 lanes per ray, no-return LDS atomics, the
// band stored once through the split of smj_hmap.h.  What differs:
//   (0) the status of the env -- the pose read from pose_dev, the gate word -- is resolved before any LDS work.  The workgroups of an
//       env that is not SMJ_MAP_OK store zeros (accumulate = 0) or nothing at all, band 0 its info and cells, and return;
//   (1) the pose comes from pose_dev: thread k lays origin and end of ray k into the map by smj_map_line (one sincosf per thread,
//       all float arithmetic of a ray done once, by one lane).  The records are built in chunks of 384 rays -- the capacity of the
//       lidar ray cast, so one chunk for every model it takes -- which keeps the LDS at the 39.5 KiB of smj_occ.hip and four
//       workgroups on a CU while the entry takes the matcher's 1024 rays;
//   (2) the walk is clipped to the band in closed form: along the major axis the coordinate of step i is a + i s, so the steps inside
//       the band are an interval (smj_map_range) and the lanes of a group stride over that interval alone.  smj_occ.hip evaluates
//       the cells a ray has outside the band before it skips them; here only the minor coordinate is still tested per cell;
//   (3) band 0 also writes the env's info (three LDS counters) and the cells of every ray.
//
// Measured (profiles/mapping_cost.txt, 4096 envs, 128 x 128 cells of 5 cm, 85 returns and 243 clearing rays per scan; beside
// smj_lidar_to_occupancy(world) in the same run): 0.56 ms with ranges to 5 m and 0.56 ms to 9.5 m against 0.65 ms and 0.87 ms -- the
// longer range costs nothing here; 0.136 ms against 0.129 ms without a miss layer (no walk to clip: the second transformed end, the
// sincosf and the counters show); 0.36 ms with a random half of the envs gated, but 0.56 ms with every other env gated: those
// workgroups are blocks 4 .. 7 of every eight, which the round-robin deal of blocks puts on four of the eight XCDs.
#include "smj_map.h"
#include "smj_scan.h"

static constexpr int MAP_THREADS = 256;
static constexpr int MAP_GROUP = 32;     // lanes per ray
static constexpr int MAP_CHUNK = 384;    // ray records in LDS at a time

struct MapArgs {
  SmjScanSource src;   // smj_scan.h
  const float* pose;
  const int* gate;
  long gate_ld;
  int* hit;
  int* miss;
  int* info;
  int* cell_out;
  int num_envs, nlidar, body, nx, ny, no_return_clears, accumulate, bands;
  float x0, y0, cell, r_min, r_max;
};

// the four words of ray k of cell_dev: one 16-byte store where the buffer allows it
__device__ __forceinline__ void map_store_cells(int* cell_out, bool wide, int k, int ax, int ay, int bx, int by) {
  if (wide) {
    *reinterpret_cast<int4*>(cell_out + 4 * k) = make_int4(ax, ay, bx, by);
  } else {
    cell_out[4 * k] = ax; cell_out[4 * k + 1] = ay; cell_out[4 * k + 2] = bx; cell_out[4 * k + 3] = by;
  }
}

__global__ __launch_bounds__(MAP_THREADS) void smj_map_kernel(const MapArgs a) {
  __shared__ unsigned hits[SMJ_OCC_BAND_CELLS];
  __shared__ unsigned misses[SMJ_OCC_BAND_CELLS];
  __shared__ smj_occ_line_t rays[MAP_CHUNK];
  __shared__ int s_info[4];
  const int tid = threadIdx.x;
  const int env = blockIdx.x / a.bands, band = blockIdx.x - env * a.bands;
  const smj_hmap_band_t b = smj_hmap_band(a.nx, a.ny, SMJ_OCC_BAND_CELLS, band);
  const int ncell = b.rows * b.cols;   // <= SMJ_OCC_BAND_CELLS
  const long long g0 = (long long)env * a.nx * a.ny + (long long)b.r0 * a.nx + b.c0;   // the band's first cell in the outputs
  int* ho = a.hit + g0;
  int* mo = a.miss ? a.miss + g0 : nullptr;
  int* cell_out = band == 0 && a.cell_out ? a.cell_out + (long long)env * a.nlidar * 4 : nullptr;
  const bool wide = ((uintptr_t)a.cell_out & 15) == 0;   // then every ray's four words are a 16-byte group

  // (0) the status: the same for every thread of the workgroup
  const float x = a.pose[env], y = a.pose[a.num_envs + env], theta = a.pose[2 * a.num_envs + env];
  const int status = smj_map_status(x, y, theta, a.gate ? a.gate[(long long)env * a.gate_ld] : 0);
  if (status != SMJ_MAP_OK) {
    if (!a.accumulate) {
      smj_scan_store_band<MAP_THREADS, true>(ho, nullptr, ncell, tid);
      if (mo) smj_scan_store_band<MAP_THREADS, true>(mo, nullptr, ncell, tid);
    }
    if (band == 0 && tid < 4) a.info[4 * env + tid] = tid == SMJ_MAP_INFO_STATUS ? status : 0;
    if (cell_out)
      for (int k = tid; k < a.nlidar; k += MAP_THREADS) map_store_cells(cell_out, wide, k, SMJ_MAP_NO_CELL, SMJ_MAP_NO_CELL, SMJ_MAP_NO_CELL, SMJ_MAP_NO_CELL);
    return;
  }
  float sn, cs;
  sincosf(theta, &sn, &cs);

  // (1) start values
  if (a.accumulate) {
    for (int c = tid; c < ncell; c += MAP_THREADS) {
      hits[c] = (unsigned)ho[c];
      misses[c] = mo ? (unsigned)mo[c] : 0u;
    }
  } else {
    for (int c = tid; c < ncell; c += MAP_THREADS) {
      hits[c] = 0u;
      misses[c] = 0u;
    }
  }
  if (tid < 4) s_info[tid] = 0;
  int nret = 0, nclr = 0, ngrd = 0;   // this thread's rays by info word: returns kept, clearing rays kept, dropped by a guard

  for (int base = 0; base < a.nlidar; base += MAP_CHUNK) {
    const int count = min(MAP_CHUNK, a.nlidar - base);
    if (base) __syncthreads();   // the walk of the chunk before has read its records
    // ray records of the chunk
    for (int j = tid; j < count; j += MAP_THREADS) {
      const int k = base + j;
      const SmjScanSource& s = a.src;
      const int sid = s.lidar_site[k], sb = s.site_bodyid[sid];
      float bp[3], bm[9], fp[3], fm[9], o[2], d[2], len;
      for (int q = 0; q < 3; q++) bp[q] = s.xpose[(12 * sb + q) * s.ld + env];
      for (int q = 0; q < 9; q++) bm[q] = s.xpose[(12 * sb + 3 + q) * s.ld + env];
      for (int q = 0; q < 3; q++) fp[q] = s.xpose[(12 * a.body + q) * s.ld + env];
      for (int q = 0; q < 9; q++) fm[q] = s.xpose[(12 * a.body + 3 + q) * s.ld + env];
      const float lz[3] = {s.site_mat[9 * sid + 2], s.site_mat[9 * sid + 5], s.site_mat[9 * sid + 8]};
      smj_occ_ray(SMJ_OCC_BODY, bp, bm, s.site_pos + 3 * sid, lz, fp, fm, o, d);
      const int cls = smj_occ_classify(s.lidar[(long long)k * s.lidar_ld + env], a.r_min, a.r_max, a.no_return_clears, &len);
      smj_occ_line_t L = smj_map_line(cls, o, d, len, x, y, cs, sn, a.x0, a.y0, a.cell);
      const int word = smj_map_info_word(cls, L.kind);
      nret += word == SMJ_MAP_INFO_RETURNS; nclr += word == SMJ_MAP_INFO_CLEARS; ngrd += word == SMJ_MAP_INFO_GUARDED;
      if (cell_out) {
        const bool kept = L.kind != SMJ_OCC_DROP;
        map_store_cells(cell_out, wide, k, kept ? L.ax : SMJ_MAP_NO_CELL, kept ? L.ay : SMJ_MAP_NO_CELL, kept ? L.bx : SMJ_MAP_NO_CELL,
                        kept ? L.by : SMJ_MAP_NO_CELL);
      }
      // the line stays inside the box of its two ends: a ray whose box misses the band adds nothing here
      const int xl = min(L.ax, L.bx), xh = max(L.ax, L.bx), yl = min(L.ay, L.by), yh = max(L.ay, L.by);
      if (xh < b.c0 || xl >= b.c0 + b.cols || yh < b.r0 || yl >= b.r0 + b.rows) L.kind = SMJ_OCC_DROP;
      rays[j] = L;
    }
    __syncthreads();

    // (2) walk the rays of the chunk
    if (mo) {
      const int grp = tid / MAP_GROUP, lane = tid - grp * MAP_GROUP;
      for (int j = grp; j < count; j += MAP_THREADS / MAP_GROUP) {
        const smj_occ_line_t L = rays[j];
        if (L.kind == SMJ_OCC_DROP) continue;
        const int n = smj_occ_steps(L);
        int i_lo, i_hi;
        smj_map_range(L, n, b, &i_lo, &i_hi);   // the steps inside the band along the major axis
        for (int i = i_lo + lane; i <= i_hi; i += MAP_GROUP) {
          int ix, iy;
          smj_occ_cell(L, n, i, &ix, &iy);
          const int slot = smj_hmap_slot(b, ix, iy);   // -1 where the minor coordinate leaves the band
          if (slot >= 0) atomicAdd(smj_occ_layer(L, n, i) ? &hits[slot] : &misses[slot], 1u);   // result unused: no-return LDS atomic
        }
      }
    } else {
      // without a miss layer only the last cell of a return counts: a lane per ray
      for (int j = tid; j < count; j += MAP_THREADS) {
        const smj_occ_line_t L = rays[j];
        if (L.kind != SMJ_OCC_RETURN) continue;
        const int slot = smj_hmap_slot(b, L.bx, L.by);
        if (slot >= 0) atomicAdd(&hits[slot], 1u);
      }
    }
  }
  if (band == 0) {   // s_info was zeroed before the first barrier; LDS, commutative
    if (nret) atomicAdd(&s_info[SMJ_MAP_INFO_RETURNS], nret);
    if (nclr) atomicAdd(&s_info[SMJ_MAP_INFO_CLEARS], nclr);
    if (ngrd) atomicAdd(&s_info[SMJ_MAP_INFO_GUARDED], ngrd);
  }
  __syncthreads();

  // (3) store the band once
  smj_scan_store_band<MAP_THREADS, true>(ho, hits, ncell, tid);
  if (mo) smj_scan_store_band<MAP_THREADS, true>(mo, misses, ncell, tid);
  if (band == 0 && tid < 4) a.info[4 * env + tid] = tid == SMJ_MAP_INFO_STATUS ? SMJ_MAP_OK : s_info[tid];
}

void smj_launch_map(const SmjScanSource& src, int num_envs, int nlidar, int body, float r_min, float r_max, const float* pose, const int* gate,
                    long gate_ld, float x0, float y0, float cell, int nx, int ny, int no_return_clears, int accumulate, int* hit, int* miss, int* info,
                    int* cell_out, hipStream_t stream) {
  MapArgs a;
  a.src = src; a.pose = pose; a.gate = gate; a.gate_ld = gate_ld;
  a.hit = hit; a.miss = miss; a.info = info; a.cell_out = cell_out;
  a.num_envs = num_envs; a.nlidar = nlidar; a.body = body; a.nx = nx; a.ny = ny; a.no_return_clears = no_return_clears; a.accumulate = accumulate;
  a.bands = smj_hmap_bands(nx, ny, SMJ_OCC_BAND_CELLS);
  a.x0 = x0; a.y0 = y0; a.cell = cell; a.r_min = r_min; a.r_max = r_max;
  const dim3 grid((unsigned)((long long)num_envs * a.bands)), block(MAP_THREADS);
  hipLaunchKernelGGL(smj_map_kernel, grid, block, 0, stream, a);
}
