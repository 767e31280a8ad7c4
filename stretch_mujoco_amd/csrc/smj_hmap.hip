// smj_depth_to_heightmap: depth images -> per-cell highest point and hit count of a 2.5-D grid in the camera, world or a body
// frame (smj_hmap.h has the binning rule, the key and the bands; smj_points.h the point of a pixel).  One kernel, no global atomics,
// no workspace: both reductions (a max, an integer sum) are done in LDS and the band is stored once.
//
// Grid.  One workgroup per (env, band).  The band's cells live in LDS as two 32-bit arrays, the order-preserving key of z (0 =
// empty) and the count.  The workgroup (1) composes the env's 3x4 transform into LDS (thread 0, smj_points_transform) and sets its
// cells to zero, or with accumulate to what the outputs hold; (2) streams ALL kept pixels of the env's image -- 16-byte loads of four
// depths where stride is 1 and the address allows it, scalar loads for the few pixels before / after the aligned body and for every
// other case, the SAME arithmetic on both -- and scatters each kept point that falls into its band with a no-return LDS atomic max on
// the key and a no-return LDS atomic add on the count; (3) after a barrier decodes and stores the band, lane-contiguous (16 bytes
// per lane where the address allows it).  Nothing but the two outputs is written.
//
// Band size and workgroup size.  LDS costs 8 bytes per cell; a CU has 160 KiB.  A band of C cells is read by a workgroup that streams
// the whole image, so a call moves bands * 4 B * kept pixels + 8 B * cells (+ 8 B * cells with accumulate): C wants to be large so
// that the usual grids (64 x 64 at 5 cm = 3.2 m square) are ONE band, and small so that a CU still holds enough wavefronts to cover
// the latency of the depth loads, the only global traffic that matters (407 KB in, 32 KiB out per env at 424 x 240 / 64 x 64).
// C = 4096 (32 KiB exactly; the transform passes through the cells' own LDS) with 256 threads: five workgroups = 20 wavefronts per CU, five per SIMD, each with two 16-byte
// loads in flight per lane (the loop is unrolled by two) = 40 KiB outstanding per CU.  C = 8192 would halve the bands of a 128 x 128
// grid but leaves two workgroups per CU: at 256 threads only 8 wavefronts, at 512 threads 16 with barriers twice as wide.  C = 2048
// makes the 64 x 64 grid two bands, i.e. reads every image twice.  The kernel needs few registers (profiles/height_map_cost.txt), so
// LDS, not VGPRs, sets the occupancy.
//
// Contention.  Neighbouring pixels of a floor or a wall fall into one cell, so a wavefront sends many LDS atomics to one address and
// they serialise.  A pre-merge inside the wavefront (the lanes that share the first kept lane's cell reduce their keys with a
// butterfly max and count themselves with a popcount, one lane issues the two atomics) gives bit-identical arrays, was built and
// measured at 4096 envs, and lost: 2.90 ms against 2.49 ms per fused map of both cameras on a 64 x 64 grid, 9.50 against 8.10 ms on
// 128 x 128 (profiles/height_map_cost.txt).  The ballots and shuffles cost every pixel more than the serialised atomics cost the
// pixels that collide, so every kept lane issues its own two atomics.
#include "smj_hmap.h"

static constexpr int HM_THREADS = 256;

struct HmapArgs {
  const float* xpose;
  long ld;
  const int* cam_bodyid;
  const float* cam_pos;
  const float* cam_mat;
  const float* depth;
  float* zmax;
  int* count;
  int cam, width, height, stride, kind, body, nx, ny, accumulate, bands;
  float th, aspect, x0, y0, inv_cell, z_lo, z_hi;
};

__device__ __forceinline__ void hm_pixel(const HmapArgs& a, const smj_hmap_band_t& b, float d, int u, int v, const float* T, unsigned* keys,
                                         unsigned* cnt) {
  int ix = 0, iy = 0;
  float z;
  const bool in_grid = smj_hmap_pixel(d, u, v, a.width, a.height, a.th, a.aspect, T, a.x0, a.y0, a.inv_cell, a.nx, a.ny, a.z_lo, a.z_hi,
                                      &ix, &iy, &z);
  const int slot = in_grid ? smj_hmap_slot(b, ix, iy) : -1;
  if (slot >= 0) {   // results unused: no-return LDS atomics
    atomicMax(&keys[slot], smj_hmap_key(z));
    atomicAdd(&cnt[slot], 1u);
  }
}

__global__ __launch_bounds__(HM_THREADS) void smj_hmap_kernel(const HmapArgs a) {
  __shared__ unsigned keys[SMJ_HMAP_BAND_CELLS];
  __shared__ unsigned cnt[SMJ_HMAP_BAND_CELLS];
  float* Ts = reinterpret_cast<float*>(keys);   // the transform passes through the first cells before they are initialised: 12 floats
                                                // of their own would make the workgroup 32 KiB + 48 B, four per CU instead of five
  const int tid = threadIdx.x;
  const int env = blockIdx.x / a.bands, band = blockIdx.x - env * a.bands;
  const smj_hmap_band_t b = smj_hmap_band(a.nx, a.ny, SMJ_HMAP_BAND_CELLS, band);
  const int ncell = b.rows * b.cols;   // <= SMJ_HMAP_BAND_CELLS
  const long long g0 = (long long)env * a.nx * a.ny + (long long)b.r0 * a.nx + b.c0;   // the band's first cell in the outputs
  float* zo = a.zmax + g0;
  int* co = a.count ? a.count + g0 : nullptr;

  // (1) transform and start values
  if (tid == 0) {
    float T[12];
    smj_points_env_transform(a.kind, a.xpose, a.ld, env, a.cam_bodyid, a.cam_pos, a.cam_mat, a.cam, a.body, T);
    for (int k = 0; k < 12; k++) Ts[k] = T[k];
  }
  __syncthreads();
  float T[12];
  for (int k = 0; k < 12; k++) T[k] = Ts[k];
  __syncthreads();
  if (a.accumulate) {
    for (int c = tid; c < ncell; c += HM_THREADS) {
      keys[c] = smj_hmap_key_of_stored(zo[c]);
      cnt[c] = co ? (unsigned)co[c] : 0u;
    }
  } else {
    for (int c = tid; c < ncell; c += HM_THREADS) {
      keys[c] = 0u;
      cnt[c] = 0u;
    }
  }
  __syncthreads();

  // (2) stream the env's kept pixels
  const int W = a.width, H = a.height;
  const long long hw = (long long)W * H;   // < 2^31 (the entry checks)
  const float* img = a.depth + (long long)env * hw;
  if (a.stride == 1) {
    // flat pixels [0, hw): `lead` scalar ones up to the first 16-byte boundary, ng groups of four, then the tail
    const int n = (int)hw;
    int lead = (int)((16u - (unsigned)((uintptr_t)img & 15u)) & 15u) >> 2;
    if (lead > n) lead = n;
    const int ng = (n - lead) >> 2;
    const float4* img4 = reinterpret_cast<const float4*>(img + lead);
    for (int r = 0; r < ng; r += 2 * HM_THREADS) {
      const int gg[2] = {r + tid, r + HM_THREADS + tid};
      const bool have[2] = {gg[0] < ng, gg[1] < ng};
      const float4 none = make_float4(0.f, 0.f, 0.f, 0.f);   // depth 0 is invalid: dropped
      const float4 q0 = have[0] ? img4[gg[0]] : none, q1 = have[1] ? img4[gg[1]] : none;   // both loads in flight before the arithmetic
      const float d[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
      for (int h = 0; h < 2; h++) {
        const int p = have[h] ? lead + 4 * gg[h] : 0;
        int v = p / W, u = p - v * W;
        for (int k = 0; k < 4; k++) {
          hm_pixel(a, b, d[4 * h + k], u, v, T, keys, cnt);
          if (++u == W) { u = 0; ++v; }
        }
      }
    }
    const int tail0 = lead + 4 * ng, nrest = lead + (n - tail0);   // <= 6 pixels, first wavefront
    if (tid < 64) {
      const bool mine = tid < nrest;
      const int p = mine ? (tid < lead ? tid : tail0 + (tid - lead)) : 0;
      const int v = p / W, u = p - v * W;
      hm_pixel(a, b, mine ? img[p] : 0.f, u, v, T, keys, cnt);
    }
  } else {
    const int wp = smj_points_grid(W, a.stride), hp = smj_points_grid(H, a.stride);
    const int nq = wp * hp;
    for (int q0 = 0; q0 < nq; q0 += HM_THREADS) {
      const int q = q0 + tid;
      const bool mine = q < nq;
      const int i = mine ? q / wp : 0, j = mine ? q - i * wp : 0;
      int u, v;
      smj_points_pixel(i, j, a.stride, &u, &v);
      hm_pixel(a, b, mine ? img[(long long)v * W + u] : 0.f, u, v, T, keys, cnt);
    }
  }
  __syncthreads();

  // (3) decode and store the band once: scalar cells up to the first 16-byte boundary of the output, groups of four, the tail
  const smj_hmap_split_t s = smj_hmap_store_split((uintptr_t)zo, ncell);
  const bool cvec = co && (((uintptr_t)co ^ (uintptr_t)zo) & 15u) == 0;   // the counts share the heights' phase: wide stores for both
  for (int g = tid; g < s.groups; g += HM_THREADS) {
    const int c = s.lead + 4 * g;
    *reinterpret_cast<float4*>(zo + c) =
        make_float4(smj_hmap_unkey(keys[c]), smj_hmap_unkey(keys[c + 1]), smj_hmap_unkey(keys[c + 2]), smj_hmap_unkey(keys[c + 3]));
    if (cvec) *reinterpret_cast<int4*>(co + c) = make_int4((int)cnt[c], (int)cnt[c + 1], (int)cnt[c + 2], (int)cnt[c + 3]);
  }
  if (co && !cvec)
    for (int c = s.lead + tid; c < s.tail0; c += HM_THREADS) co[c] = (int)cnt[c];
  if (tid < s.rest) {
    const int c = smj_hmap_split_rest(s, tid);
    zo[c] = smj_hmap_unkey(keys[c]);
    if (co) co[c] = (int)cnt[c];
  }
}

void smj_launch_hmap(const float* xpose, long ld, int num_envs, const int* cam_bodyid, const float* cam_pos, const float* cam_mat,
                     int cam, int width, int height, float fovy_deg, const float* depth, int stride, int kind, int body, float x0,
                     float y0, float cell, int nx, int ny, float z_lo, float z_hi, int accumulate, float* zmax, int* count,
                     hipStream_t stream) {
  HmapArgs a;
  a.xpose = xpose; a.ld = ld; a.cam_bodyid = cam_bodyid; a.cam_pos = cam_pos; a.cam_mat = cam_mat; a.depth = depth;
  a.zmax = zmax; a.count = count;
  a.cam = cam; a.width = width; a.height = height; a.stride = stride; a.kind = kind; a.body = body; a.nx = nx; a.ny = ny;
  a.accumulate = accumulate;
  a.bands = smj_hmap_bands(nx, ny, SMJ_HMAP_BAND_CELLS);
  a.th = tanf(fovy_deg * 3.14159265358979323846f / 360.f);   // as smj_launch_depth and smj_launch_points
  a.aspect = (float)width / (float)height;
  a.x0 = x0; a.y0 = y0; a.inv_cell = 1.f / cell; a.z_lo = z_lo; a.z_hi = z_hi;
  const dim3 grid((unsigned)((long long)num_envs * a.bands)), block(HM_THREADS);
  hipLaunchKernelGGL(smj_hmap_kernel, grid, block, 0, stream, a);
}
