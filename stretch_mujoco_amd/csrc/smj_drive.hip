// smj_navigation_to_velocity: pose, twist, costmap and navigation potential of every env, and one table of candidate arcs shared by
// all of them -> per env the best base command (smj_drive.h has the cell of a point, what a point contributes, the blocked
// predicate, the score, the order and the status).  One kernel, no workspace, no global atomics.  Every output is defined without
// reference to an order -- a maximum over a candidate's swept points, the minimum of a total order over the candidates -- so two
// calls give identical bits.
//
// Grid.  One workgroup of 256 threads per env.
//   (1) thread 0 reads the pose, takes ONE sincosf (the accurate one) and the robot's own cell and leaves them in LDS;
//   (2) the table pass: entry i = k P + p goes to thread i % 256 in round i / 256, so a wave reads 64 consecutive float2 of
//       point_dev (shared by all envs: it stays in L2) and stores 64 consecutive words of cell_dev.  A swept point's contribution
//       goes into its candidate's LDS word by an LDS atomic max (commutative, so the order does not show); the scoring point's
//       potential has one writer;
//   (3) the candidate pass: candidate k goes to thread k % 256, which evaluates the window and the score, stores score_dev and keeps
//       the first of its candidates in the (score, k) order;
//   (4) the arg-min: a butterfly over the wave's 64 lanes, then over the four waves' results in LDS; thread 0 stores cmd and best.
// Loops are bounded by K P <= 32768 entries: at most 128 rounds in (2), 4 in (3).
#include "smj_drive.h"

static constexpr int DRIVE_THREADS = 256;

struct DriveArgs {
  const float* pose;
  const float* twist;
  const uint8_t* cost;
  const int* potential;
  const float* command;
  const float* point;
  const int* bias;
  float* cmd;
  int* best;
  long long* score;
  int* cell_out;
  int num_envs, nx, ny, K, P, lethal, outside_is_free, goal_weight, obstacle_weight, arrive_potential;
  float x0, y0, cell, max_dv, max_dw;
};

__global__ __launch_bounds__(DRIVE_THREADS) void smj_drive_kernel(const DriveArgs a) {
  __shared__ int s_swept[SMJ_DRIVE_MAX_CANDIDATES], s_goal[SMJ_DRIVE_MAX_CANDIDATES];
  __shared__ float s_pose[5];   // x, y, cos, sin, and whether the pose is finite
  __shared__ int s_own;
  __shared__ long long s_best[DRIVE_THREADS / 64];
  __shared__ int s_bestk[DRIVE_THREADS / 64];
  const int tid = threadIdx.x, env = blockIdx.x;
  const int nx = a.nx, ny = a.ny, K = a.K, P = a.P, n = K * P;   // n <= SMJ_DRIVE_MAX_TABLE
  const long long e0 = (long long)env * nx * ny;
  const uint8_t* cost = a.cost ? a.cost + e0 : nullptr;
  const int* potential = a.potential + e0;

  // (1) the pose
  if (tid == 0) {
    const float x = a.pose[env], y = a.pose[a.num_envs + env], th = a.pose[2 * a.num_envs + env];
    float s, c;
    sincosf(th, &s, &c);
    s_pose[0] = x; s_pose[1] = y; s_pose[2] = c; s_pose[3] = s;
    s_pose[4] = smj_drive_finite(x) && smj_drive_finite(y) && smj_drive_finite(th) ? 1.0f : 0.0f;
    s_own = smj_drive_cell(x, y, a.x0, a.y0, a.cell, nx, ny);
  }
  for (int k = tid; k < K; k += DRIVE_THREADS) {
    s_swept[k] = 0;
    s_goal[k] = SMJ_DRIVE_NAV_NONE;
  }
  __syncthreads();
  const float x = s_pose[0], y = s_pose[1], c = s_pose[2], s = s_pose[3];

  // (2) the table
  int* cell_out = a.cell_out ? a.cell_out + (long long)env * n : nullptr;
  const int rounds = smj_drive_rounds(n, DRIVE_THREADS);
  for (int r = 0; r < rounds; r++) {
    const int i = r * DRIVE_THREADS + tid;
    if (i >= n) break;
    const int k = i / P, p = i - k * P;
    const float px = a.point[2 * i], py = a.point[2 * i + 1];
    const int at = smj_drive_cell(smj_drive_world_x(x, c, s, px, py), smj_drive_world_y(y, c, s, px, py), a.x0, a.y0, a.cell, nx, ny);
    if (cell_out) cell_out[i] = at;
    if (p < P - 1) {
      const int v = smj_drive_swept(at, at >= 0 && cost ? cost[at] : 0, a.lethal, a.outside_is_free);
      if (v) atomicMax(&s_swept[k], v);   // LDS
    } else if (at >= 0) {
      s_goal[k] = potential[at];
    }
  }
  __syncthreads();

  // (3) the candidates
  const bool window = a.twist != nullptr;
  const float v0 = window ? a.twist[env] : 0.0f, w0 = window ? a.twist[a.num_envs + env] : 0.0f;
  long long mine = SMJ_DRIVE_NO_SCORE;
  int minek = 0x7fffffff;
  for (int k = tid; k < K; k += DRIVE_THREADS) {
    const bool in = !window || smj_drive_in_window(a.command[2 * k], a.command[2 * k + 1], v0, w0, a.max_dv, a.max_dw);
    const long long sc = smj_drive_score(s_swept[k], s_goal[k], in, a.goal_weight, a.obstacle_weight, a.bias ? a.bias[k] : 0);
    if (a.score) a.score[(long long)env * K + k] = sc;
    if (smj_drive_before(sc, k, mine, minek)) { mine = sc; minek = k; }
  }

  // (4) the first in the order: within the wave, then across the waves
  for (int off = 32; off >= 1; off >>= 1) {
    const long long os = __shfl_xor(mine, off);
    const int ok = __shfl_xor(minek, off);
    if (smj_drive_before(os, ok, mine, minek)) { mine = os; minek = ok; }
  }
  if ((tid & 63) == 0) {
    s_best[tid >> 6] = mine;
    s_bestk[tid >> 6] = minek;
  }
  __syncthreads();
  if (tid == 0) {
    for (int wv = 1; wv < DRIVE_THREADS / 64; wv++)
      if (smj_drive_before(s_best[wv], s_bestk[wv], mine, minek)) { mine = s_best[wv]; minek = s_bestk[wv]; }
    const int own = s_own;
    const int status = smj_drive_status(s_pose[4] != 0.0f, own, own >= 0 ? potential[own] : 0, a.arrive_potential, mine);
    const bool go = status == SMJ_DRIVE_OK;
    const int row = go ? minek : 0;   // a row of the table in either case: no load from an index that is none
    const float v = a.command[2 * row], w = a.command[2 * row + 1];
    a.cmd[env] = go ? v : 0.0f;
    a.cmd[a.num_envs + env] = go ? w : 0.0f;
    a.best[2 * env] = go ? minek : -1;
    a.best[2 * env + 1] = status;
  }
}

void smj_launch_drive(int num_envs, const float* pose, const float* twist, const uint8_t* cost, const int* potential, int nx, int ny, float x0, float y0,
                      float cell, const float* command, const float* point, const int* bias, int K, int P, int lethal, int outside_is_free,
                      int goal_weight, int obstacle_weight, int arrive_potential, float max_dv, float max_dw, float* cmd, int* best, long long* score,
                      int* cell_out, hipStream_t stream) {
  DriveArgs a;
  a.pose = pose; a.twist = twist; a.cost = cost; a.potential = potential; a.command = command; a.point = point; a.bias = bias;
  a.cmd = cmd; a.best = best; a.score = score; a.cell_out = cell_out;
  a.num_envs = num_envs; a.nx = nx; a.ny = ny; a.K = K; a.P = P; a.lethal = lethal; a.outside_is_free = outside_is_free;
  a.goal_weight = goal_weight; a.obstacle_weight = obstacle_weight; a.arrive_potential = arrive_potential;
  a.x0 = x0; a.y0 = y0; a.cell = cell; a.max_dv = max_dv; a.max_dw = max_dw;
  hipLaunchKernelGGL(smj_drive_kernel, dim3((unsigned)num_envs), dim3(DRIVE_THREADS), 0, stream, a);
}
