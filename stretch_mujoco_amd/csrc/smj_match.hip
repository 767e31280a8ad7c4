// smj_scan_to_pose: the lidar scan, a likelihood field and a prior pose of every env, and one table of rotations shared by all of
// them -> per env the pose, out of T rotations x (2 wy + 1) x (2 wx + 1) whole-cell shifts, at which the scan's returns collect the
// largest sum of the field (smj_match.h has the point of a ray, the cell of a point, the score, the order, the status and the output
// pose; smj_scan.h what the scan entries share: the source of the rays, the copy of (1) and the butterfly of (3)).  One kernel, no
// workspace, no global atomics.  Every output is defined without reference to an order -- an integer sum over the points, the first
// of a total order over the candidates -- so two calls give identical bits.
//
// Grid.  One workgroup of 512 threads per env.
//   (1) the env's field goes into LDS once, bytes as they are: the copy starts at the LDS offset that has the alignment of the global
//       address, so the middle of the range moves in 16-byte loads and stores whatever the pointer, the few bytes before and after it
//       one by one.  Thread k turns ray k into its point of the robot's frame (all float arithmetic of a ray is done once, by one
//       lane; a ray without a return keeps NaN, which no rotation places); threads t < T take the sincosf of theta + angle[t];
//   (2) per rotation: thread k stores the cell of ray k to cell_dev and, if the point is placed, appends it as one packed word to a
//       list in LDS (an LDS atomic hands out the slots; the order of the list does not show in an integer sum), so that the sums run
//       over the placed points alone -- in the scenes at hand a quarter of the rays return; barrier; candidate
//       c = (dy + wy) (2 wx + 1) + (dx + wx) goes to thread c % 512, so the lanes of a wave hold adjacent dx: at every point they read
//       adjacent bytes of the field, a handful of LDS words, while the point's cell is one word broadcast to all lanes.  The thread
//       sums the field over the list, stores J and keeps the first of its candidates in the order; barrier;
//   (3) the first in the order: a butterfly over the wave's 64 lanes, then over the eight waves' results in LDS; thread 0 stores the
//       pose and `best`.
// Two builds by the size of the field in LDS: up to 16384 cells (128 x 128: 29 KiB with points and cells, four workgroups and so the
// full 32 waves per CU) and up to 65536 (77 KiB, two per CU, 32 waves again).  Loops are bounded by the limits of smj_match.h: 2
// rounds of rays, 64 rotations, 9 rounds of candidates, 1024 points.
//
// Measured (profiles/scanmatch_cost.txt, 4096 envs, 128 x 128, 21 x 21 x 21 candidates): 1.34 ms on the scene's scan (85 of 360 rays
// return), 5.0 ms when every ray returns; 5.4 ms before the list of placed points; 3.0 / 1.6 / 1.4 / 1.3 ms with 128 / 256 / 448 / 512
// threads (the sums wait on LDS: more waves hide more of it, and 441 candidates fill 512 threads in one round).
#include "smj_match.h"
#include "smj_scan.h"

static constexpr int MATCH_THREADS = 512;
static constexpr int MATCH_SMALL_CELLS = 16384;

struct MatchArgs {
  SmjScanSource src;   // smj_scan.h
  const uint8_t* field;
  const float* pose;
  const float* angle;
  const int* bias;
  float* pose_out;
  int* best;
  int* score;
  int* cell_out;
  int num_envs, nlidar, body, nx, ny, T, wx, wy, shift_weight, min_points;
  float r_min, r_max, x0, y0, cell;
};

template <int CELLS>
__global__ __launch_bounds__(MATCH_THREADS) void smj_match_kernel(const MatchArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t s_raw[CELLS + 16];
  __shared__ float s_px[SMJ_MATCH_MAX_POINTS], s_py[SMJ_MATCH_MAX_POINTS];
  __shared__ int s_cell[SMJ_MATCH_MAX_POINTS];
  __shared__ float s_cos[SMJ_MATCH_MAX_ANGLES], s_sin[SMJ_MATCH_MAX_ANGLES];
  __shared__ int s_n, s_m[2];
  __shared__ int s_bestJ[MATCH_THREADS / 64], s_besti[MATCH_THREADS / 64];
  const int tid = threadIdx.x, env = blockIdx.x;
  const int nx = a.nx, ny = a.ny, ncell = nx * ny, K = a.nlidar, T = a.T;   // ncell <= CELLS, K <= SMJ_MATCH_MAX_POINTS, T <= SMJ_MATCH_MAX_ANGLES
  const float x = a.pose[env], y = a.pose[a.num_envs + env], theta = a.pose[2 * a.num_envs + env];

  // (1) the field: LDS byte sh + i holds field byte i, and sh + lead is a multiple of 16 in both address spaces
  const uint8_t* field = smj_scan_stage_field<MATCH_THREADS>(s_raw, a.field + (long long)env * ncell, ncell, tid);
  if (tid == 0) { s_n = 0; s_m[0] = 0; }
  if (tid < T) {
    float s, c;
    sincosf(smj_match_pose_theta(theta, a.angle[tid]), &s, &c);
    s_cos[tid] = c;
    s_sin[tid] = s;
  }
  __syncthreads();
  // the points
  for (int k = tid; k < K; k += MATCH_THREADS) {
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
    const bool counts = cls == SMJ_OCC_RETURN && smj_drive_finite(p[0]) && smj_drive_finite(p[1]);
    s_px[k] = counts ? p[0] : __int_as_float(0x7fc00000);
    s_py[k] = counts ? p[1] : __int_as_float(0x7fc00000);
    if (counts) atomicAdd(&s_n, 1);   // LDS, commutative
  }
  __syncthreads();

  // (2) the rotations
  const int wx = a.wx, wy = a.wy, WX = 2 * wx + 1, C = WX * (2 * wy + 1);   // C <= 4225
  int mineJ = -0x7fffffff - 1, minei = 0x7fffffff;
  for (int t = 0; t < T; t++) {
    const float c = s_cos[t], s = s_sin[t];
    int* cell_out = a.cell_out ? a.cell_out + (((long long)env * T + t) * K) * 2 : nullptr;
    for (int k = tid; k < K; k += MATCH_THREADS) {
      int ix, iy;
      if (smj_match_cell(x, y, c, s, s_px[k], s_py[k], a.x0, a.y0, a.cell, nx, ny, &ix, &iy))
        s_cell[atomicAdd(&s_m[t & 1], 1)] = smj_match_pack(ix, iy);   // LDS; the order of the list does not show in an integer sum
      if (cell_out) {
        cell_out[2 * k] = ix;
        cell_out[2 * k + 1] = iy;
      }
    }
    __syncthreads();
    const int m = s_m[t & 1];                 // the placed points of this rotation
    if (tid == 0) s_m[(t + 1) & 1] = 0;       // the next rotation's count: nobody reads or adds to it before the barrier below
    const int bias = smj_match_bias(a.bias ? a.bias[t] : 0);
    int* score = a.score ? a.score + ((long long)env * T + t) * C : nullptr;
    for (int cand = tid; cand < C; cand += MATCH_THREADS) {
      const int dyi = cand / WX, dx = cand - dyi * WX - wx, dy = dyi - wy;
      int S = 0;
      for (int k = 0; k < m; k++) {
        const int w = s_cell[k];
        const int at = smj_match_shifted(smj_match_pack_x(w), smj_match_pack_y(w), dx, dy, nx, ny);
        S += at >= 0 ? (int)field[at] : 0;
      }
      const int J = smj_match_score(S, bias, a.shift_weight, dx, dy), i = smj_match_index(t, dy, dx, wx, wy);
      if (score) score[cand] = J;
      if (smj_match_before(J, i, mineJ, minei)) { mineJ = J; minei = i; }
    }
    __syncthreads();
  }

  // (3) the first in the order: within the wave, then across the waves
  const int2 first = smj_scan_wave_first(mineJ, minei);
  mineJ = first.x; minei = first.y;
  if ((tid & 63) == 0) {
    s_bestJ[tid >> 6] = mineJ;
    s_besti[tid >> 6] = minei;
  }
  __syncthreads();
  if (tid == 0) {
    for (int wv = 1; wv < MATCH_THREADS / 64; wv++)
      if (smj_match_before(s_bestJ[wv], s_besti[wv], mineJ, minei)) { mineJ = s_bestJ[wv]; minei = s_besti[wv]; }
    const int n = s_n;
    const int status = smj_match_status(smj_drive_finite(x) && smj_drive_finite(y) && smj_drive_finite(theta), n, a.min_points);
    const bool ok = status == SMJ_MATCH_OK;
    int t, dy, dx;
    smj_match_unindex(minei, wx, wy, &t, &dy, &dx);   // a candidate of the table in either case: thread 0 always has one
    a.pose_out[env] = ok ? smj_match_pose_xy(dx, a.cell, x) : x;
    a.pose_out[a.num_envs + env] = ok ? smj_match_pose_xy(dy, a.cell, y) : y;
    a.pose_out[2 * a.num_envs + env] = ok ? smj_match_pose_theta(theta, a.angle[t]) : theta;
    a.best[4 * env] = ok ? minei : -1;
    a.best[4 * env + 1] = ok ? mineJ : 0;
    a.best[4 * env + 2] = n;
    a.best[4 * env + 3] = status;
  }
}

void smj_launch_match(const SmjScanSource& src, int num_envs, int nlidar, int body, float r_min, float r_max, const uint8_t* field, int nx, int ny,
                      float x0, float y0, float cell, const float* pose, const float* angle, const int* bias, int T, int wx, int wy, int shift_weight,
                      int min_points, float* pose_out, int* best, int* score, int* cell_out, hipStream_t stream) {
  MatchArgs a;
  a.src = src; a.field = field; a.pose = pose; a.angle = angle; a.bias = bias;
  a.pose_out = pose_out; a.best = best; a.score = score; a.cell_out = cell_out;
  a.num_envs = num_envs; a.nlidar = nlidar; a.body = body; a.nx = nx; a.ny = ny; a.T = T; a.wx = wx; a.wy = wy;
  a.shift_weight = shift_weight; a.min_points = min_points;
  a.r_min = r_min; a.r_max = r_max; a.x0 = x0; a.y0 = y0; a.cell = cell;
  const dim3 grid((unsigned)num_envs), block(MATCH_THREADS);
  if (nx * ny <= MATCH_SMALL_CELLS)
    hipLaunchKernelGGL(smj_match_kernel<MATCH_SMALL_CELLS>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(smj_match_kernel<SMJ_MATCH_MAX_CELLS>, grid, block, 0, stream, a);
}
