// smj_scan_to_particles: the lidar scan, a likelihood field and P particles of every env -> per particle the sum S of the field
// under the scan's returns laid out from that particle, the best particle, and (status OK, resample != 0) a systematic resampling of
// the particles by w = max(S - cut, 0) (smj_mcl.h has the weight of a point, cut and w, the threshold of a slot, the ancestor
// search, the effective sample size and the status; smj_match.h the point of a ray and its cell; smj_scan.h the source of the rays,
// the copy of (1) and the butterfly of (3), with smj_match.hip).  One kernel, no workspace, no global atomics.  Every output is
// defined without reference to an order -- integer sums, the first of a total order, a search on integer sums -- so two calls give
// identical bits.
//
// Grid.  One workgroup of 512 threads per env.
//   (1) the env's field goes into LDS once, bytes as they are, by the copy of smj_scan.h (the LDS offset takes the alignment of
//       the global address, so the middle moves in 16-byte loads whatever the pointer).  Thread k turns ray k into its point of the
//       robot's frame and, if it counts, appends it to a list in LDS (an LDS atomic hands out the slots; the order of the list does
//       not show in an integer sum): the sums run over the returns alone;
//   (2) thread t owns particles t, t + 512, ...: one sincosf per particle, then a walk over the list -- every lane reads the same
//       8 bytes of LDS, a broadcast -- with one byte of the field gathered per point.  S goes to weight_dev and to s_w in LDS; the
//       thread keeps the first of its particles in the (S, j) order;
//   (3) the first in the order: a butterfly over the wave's 64 lanes, then over the eight waves' results in LDS.  With it every
//       thread knows the status.  An env that is not OK, or a call without resampling, copies its particles and returns: no scan,
//       no search;
//   (4) the inclusive sums of w replace S in s_w, 512 at a time: within a wave on the DPP data path (row shifts by 1, 2, 4, 8, then
//       the row_bcast:15 / row_bcast:31 steps of smj_wave.h's reductions), across the waves through eight words of LDS and a running
//       carry.  A slot beyond P holds w = 0, so any P in [1, 4096] scans alike.  The squares go into one 64-bit LDS sum;
//   (5) thread t owns slots t, t + 512, ...: the threshold, a binary search over s_w (adjacent lanes hold adjacent thresholds: the
//       first probes are one address for the whole wave, a broadcast, the last fall into a few neighbouring words), the gather of
//       the ancestor and the add of the noise.  Slot k opens a new ancestor iff u_(k-1) lies below the sums before a_k.
// Three builds by the field: up to 16384 cells in LDS (128 x 128: 40 KiB with weights and points, three workgroups and 24 waves per
// CU), up to 65536 (88 KiB, one workgroup), and one that leaves the field in global memory (24 KiB).  Loops are bounded by the
// limits of smj_mcl.h: 2 rounds of rays, 8 rounds of particles, 1024 points, 12 steps of a search.
//
// Measured (profiles/localize_cost.txt, 4096 envs, 128 x 128, the scene's scan with 85 of 360 rays returning): 0.15 / 0.36 / 1.30 ms
// for 256 / 1024 / 4096 particles, 0.49 / 1.27 / 4.88 ms when every ray returns; resampling is 0.03 ms of the 0.36.  With the field
// left in global memory the same calls take 0.19 / 0.41 / 1.71 ms: the staged build is the default (smj_set_option
// "mcl_stage_field").  The walk is bound by the arithmetic of smj_match_cell, about 35 vector instructions per particle and point:
// 1.24 T look-ups/s; smj_scan_to_pose's default search (9261 lattice poses) takes 1.28 ms beside it.
#include "smj_mcl.h"
#include "smj_scan.h"

static constexpr int MCL_THREADS = 512;
static constexpr int MCL_WAVES = MCL_THREADS / 64;
static constexpr int MCL_SMALL_CELLS = 16384;

struct MclArgs {
  SmjScanSource src;   // smj_scan.h
  const uint8_t* field;
  const float* particle;
  const float* noise;
  const unsigned* draw;
  float* particle_out;
  int* weight;
  int* ancestor;
  int* stat;
  float* pose_out;
  int num_envs, nlidar, body, nx, ny, P, span, min_points, resample;
  float r_min, r_max, x0, y0, cell;
};

// t + (t of the lane the DPP control names), 0 where that lane does not exist or the row is masked: a move on the integer's bits
template <int CTRL, int ROWMASK>
__device__ __forceinline__ int mcl_dpp_add(int t) {
  return t + __builtin_amdgcn_update_dpp(0, t, CTRL, ROWMASK, 0xF, false);
}

// The inclusive sum over the wave's 64 lanes.  All lanes active.
__device__ __forceinline__ int mcl_wave_scan(int t) {
  t = mcl_dpp_add<0x111, 0xF>(t);   // row_shr:1
  t = mcl_dpp_add<0x112, 0xF>(t);   // row_shr:2
  t = mcl_dpp_add<0x114, 0xF>(t);   // row_shr:4
  t = mcl_dpp_add<0x118, 0xF>(t);   // row_shr:8: every row of 16 lanes holds its own inclusive sums
  t = mcl_dpp_add<0x142, 0xA>(t);   // row_bcast:15 into rows 1 and 3: the total of the row before
  t = mcl_dpp_add<0x143, 0xC>(t);   // row_bcast:31 into rows 2 and 3: the total of rows 0 and 1
  return t;
}

// CELLS: the bytes of field the build keeps in LDS; 0 leaves the field in global memory.
template <int CELLS>
__global__ __launch_bounds__(MCL_THREADS) void smj_mcl_kernel(const MclArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_raw[CELLS + 16];
  __shared__ float2 s_p[SMJ_MCL_MAX_POINTS];
  __shared__ int s_w[SMJ_MCL_MAX_PARTICLES];   // S of every particle, then the inclusive sums of w
  __shared__ int s_bestS[MCL_WAVES], s_bestj[MCL_WAVES], s_wave[MCL_WAVES];
  __shared__ unsigned long long s_sq;
  __shared__ int s_n, s_distinct;
  const int tid = threadIdx.x, env = blockIdx.x;
  const int nx = a.nx, ny = a.ny, ncell = nx * ny, K = a.nlidar, P = a.P;   // ncell <= CELLS (or CELLS = 0), K <= SMJ_MCL_MAX_POINTS, P <= SMJ_MCL_MAX_PARTICLES
  const long long row = (long long)a.num_envs * P, at0 = (long long)env * P;   // word j of row q of this env: q row + at0 + j

  // (1) the field: LDS byte sh + i holds field byte i, and sh + lead is a multiple of 16 in both address spaces
  const uint8_t* g = a.field + (long long)env * ncell;
  const uint8_t* field = g;
  if (CELLS > 0) field = smj_scan_stage_field<MCL_THREADS>(s_raw, g, ncell, tid);
  if (tid == 0) { s_n = 0; s_distinct = 0; s_sq = 0ull; }
  __syncthreads();
  // the points
  for (int k = tid; k < K; k += MCL_THREADS) {
    const SmjScanSource& s = a.src;
    const int sid = s.lidar_site[k], sb = s.site_bodyid[sid];
    float bp[3], bm[9], fp[3], fm[9], o[2], d[2], p[2], len;
    for (int j = 0; j < 3; j++) bp[j] = s.xpose[(12 * sb + j) * s.ld + env];
    for (int j = 0; j < 9; j++) bm[j] = s.xpose[(12 * sb + 3 + j) * s.ld + env];
    for (int j = 0; j < 3; j++) fp[j] = s.xpose[(12 * a.body + j) * s.ld + env];
    for (int j = 0; j < 9; j++) fm[j] = s.xpose[(12 * a.body + 3 + j) * s.ld + env];
    const float lz[3] = {s.site_mat[9 * sid + 2], s.site_mat[9 * sid + 5], s.site_mat[9 * sid + 8]};
    smj_occ_ray(SMJ_OCC_BODY, bp, bm, s.site_pos + 3 * sid, lz, fp, fm, o, d);
    const int cls = smj_occ_classify(s.lidar[(long long)k * s.lidar_ld + env], a.r_min, a.r_max, 0, &len);
    smj_match_point(o, d, len, p);
    if (cls == SMJ_OCC_RETURN && smj_drive_finite(p[0]) && smj_drive_finite(p[1])) s_p[atomicAdd(&s_n, 1)] = make_float2(p[0], p[1]);   // LDS, at most K slots
  }
  __syncthreads();
  const int n = s_n;

  // (2) the weights
  int mineS = -1, minej = 0x7fffffff;   // every S is >= 0: the first particle of a thread always takes over
  for (int j = tid; j < P; j += MCL_THREADS) {
    const float x = a.particle[at0 + j], y = a.particle[row + at0 + j], theta = a.particle[2 * row + at0 + j];
    int S = 0;
    if (smj_mcl_finite(x, y, theta)) {
      float s, c;
      sincosf(theta, &s, &c);
      for (int k = 0; k < n; k++) {
        const float2 p = s_p[k];
        S += smj_mcl_point_weight(x, y, c, s, p.x, p.y, a.x0, a.y0, a.cell, nx, ny, field);
      }
    }
    a.weight[at0 + j] = S;
    s_w[j] = S;
    if (smj_match_before(S, j, mineS, minej)) { mineS = S; minej = j; }
  }

  // (3) the first in the order: within the wave, then across the waves
  const int2 first = smj_scan_wave_first(mineS, minej);
  mineS = first.x; minej = first.y;
  if ((tid & 63) == 0) {
    s_bestS[tid >> 6] = mineS;
    s_bestj[tid >> 6] = minej;
  }
  __syncthreads();
  mineS = s_bestS[0]; minej = s_bestj[0];   // wave 0 holds particle 0: a real one
  for (int wv = 1; wv < MCL_WAVES; wv++)
    if (smj_match_before(s_bestS[wv], s_bestj[wv], mineS, minej)) { mineS = s_bestS[wv]; minej = s_bestj[wv]; }
  const int s_max = mineS, best = minej;
  const int status = smj_mcl_status(n, a.min_points, s_max);   // the same in every thread
  const bool ok = status == SMJ_MCL_OK;
  const int cut = smj_mcl_cut(s_max, a.span);

  const unsigned* pin = reinterpret_cast<const unsigned*>(a.particle);
  unsigned* pout = reinterpret_cast<unsigned*>(a.particle_out);
  if (tid == 0 && a.pose_out) {
    unsigned* po = reinterpret_cast<unsigned*>(a.pose_out);
    for (int q = 0; q < 3; q++) po[(long long)q * a.num_envs + env] = ok ? pin[q * row + at0 + best] : 0x7fc00000u;
  }
  const bool resampling = ok && a.resample != 0;
  if (!resampling) {   // the particles as they are, bit for bit
    for (int k = tid; k < P; k += MCL_THREADS) {
      for (int q = 0; q < 3; q++) pout[q * row + at0 + k] = pin[q * row + at0 + k];
      if (a.ancestor) a.ancestor[at0 + k] = k;
    }
  }
  if (!ok) {
    if (tid < SMJ_MCL_STAT_WORDS)
      a.stat[SMJ_MCL_STAT_WORDS * env + tid] = tid == SMJ_MCL_STAT_BEST ? -1 : tid == SMJ_MCL_STAT_SMAX ? s_max : tid == SMJ_MCL_STAT_N ? n
                                               : tid == SMJ_MCL_STAT_STATUS ? status : tid == SMJ_MCL_STAT_CUT ? cut : 0;
    return;
  }

  // (4) the inclusive sums of w, in place of S; every thread ends with the same carry
  int carry = 0;
  unsigned long long sq = 0ull;
  for (int base = 0; base < P; base += MCL_THREADS) {
    const int j = base + tid;
    const int w = j < P ? smj_mcl_w(s_w[j], cut) : 0;
    sq += (unsigned long long)w * (unsigned long long)w;
    const int t = mcl_wave_scan(w);
    if ((tid & 63) == 63) s_wave[tid >> 6] = t;
    __syncthreads();
    int before = carry, all = 0;
    for (int wv = 0; wv < MCL_WAVES; wv++) {
      const int v = s_wave[wv];
      before += wv < (tid >> 6) ? v : 0;
      all += v;
    }
    if (j < P) s_w[j] = before + t;
    carry += all;
    __syncthreads();   // s_wave is free for the next round; after the last one s_w holds every sum
  }
  const int total = carry;   // >= 1: the best particle has w = min(s_max, span) >= 1
  if (sq) atomicAdd(&s_sq, sq);   // LDS, commutative
  __syncthreads();

  // (5) the slots
  if (resampling) {
    const unsigned o = smj_mcl_offset(a.draw[env], total);
    int opened = 0;
    for (int k = tid; k < P; k += MCL_THREADS) {
      const int u = smj_mcl_threshold(k, total, o, P), anc = smj_mcl_ancestor(s_w, P, u);
      opened += k == 0 || (anc > 0 && smj_mcl_threshold(k - 1, total, o, P) < s_w[anc - 1]);   // a_(k-1) < a_k
      for (int q = 0; q < 3; q++) {
        if (a.noise) a.particle_out[q * row + at0 + k] = a.particle[q * row + at0 + anc] + a.noise[q * row + at0 + k];
        else pout[q * row + at0 + k] = pin[q * row + at0 + anc];
      }
      if (a.ancestor) a.ancestor[at0 + k] = anc;
    }
    if (opened) atomicAdd(&s_distinct, opened);   // LDS, commutative
    __syncthreads();
  }
  if (tid < SMJ_MCL_STAT_WORDS)
    a.stat[SMJ_MCL_STAT_WORDS * env + tid] = tid == SMJ_MCL_STAT_BEST ? best : tid == SMJ_MCL_STAT_SMAX ? s_max : tid == SMJ_MCL_STAT_N ? n
                                             : tid == SMJ_MCL_STAT_STATUS ? status : tid == SMJ_MCL_STAT_TOTAL ? total
                                             : tid == SMJ_MCL_STAT_ESS ? smj_mcl_ess(total, (uint64_t)s_sq) : tid == SMJ_MCL_STAT_CUT ? cut : s_distinct;
}

void smj_launch_mcl(const SmjScanSource& src, int num_envs, int nlidar, int body, float r_min, float r_max, const uint8_t* field, int nx, int ny,
                    float x0, float y0, float cell, const float* particle, int P, const float* noise, const unsigned* draw, int span, int min_points,
                    int resample, float* particle_out, int* weight, int* ancestor, int* stat, float* pose_out, int stage_field, hipStream_t stream) {
  MclArgs a;
  a.src = src; a.field = field; a.particle = particle; a.noise = noise; a.draw = draw;
  a.particle_out = particle_out; a.weight = weight; a.ancestor = ancestor; a.stat = stat; a.pose_out = pose_out;
  a.num_envs = num_envs; a.nlidar = nlidar; a.body = body; a.nx = nx; a.ny = ny; a.P = P; a.span = span; a.min_points = min_points;
  a.resample = resample;
  a.r_min = r_min; a.r_max = r_max; a.x0 = x0; a.y0 = y0; a.cell = cell;
  const dim3 grid((unsigned)num_envs), block(MCL_THREADS);
  if (!stage_field)
    hipLaunchKernelGGL(smj_mcl_kernel<0>, grid, block, 0, stream, a);
  else if (nx * ny <= MCL_SMALL_CELLS)
    hipLaunchKernelGGL(smj_mcl_kernel<MCL_SMALL_CELLS>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(smj_mcl_kernel<SMJ_MATCH_MAX_CELLS>, grid, block, 0, stream, a);
}
