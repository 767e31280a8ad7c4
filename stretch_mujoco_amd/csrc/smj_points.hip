// smj_depth_to_points: depth images -> organised point clouds in the camera, world or a body frame (smj_points.h has the
// arithmetic and the conventions).  Two kernels: a per-env pass that composes the 3x4 transform once per env into the workspace,
// and the streaming pass, bounded by memory traffic: 4 bytes of depth in, 12 bytes of point out per kept pixel.
//
// Streaming pass.  The cloud is one flat array of N points.  A thread takes FOUR consecutive points (with stride 1 those are
// four consecutive depth values: one 16-byte load), a workgroup of 256 threads 1024 points = 3072 floats.  The points go through
// LDS so that the stores are lane-contiguous: thread t writes the 16-byte words t, t + 256, t + 512 of the workgroup's 12 KiB,
// 1 KiB per wavefront instruction, instead of 16-byte pieces 48 bytes apart.  The tail of the array and pointers that are only
// 4-byte aligned take scalar loads / stores around the SAME arithmetic, so the values do not depend on the path.
#include "smj_points.h"

static constexpr int PT_THREADS = 256, PT_PER_THREAD = 4, PT_PER_BLOCK = PT_THREADS * PT_PER_THREAD;

__global__ __launch_bounds__(64) void smj_points_prepass(const float* __restrict__ xpose, long ld, int num_envs, const int* __restrict__ cam_bodyid,
                                                         const float* __restrict__ cam_pos, const float* __restrict__ cam_mat, int cam, int kind,
                                                         int body, float* __restrict__ ws) {
  const int env = blockIdx.x * 64 + threadIdx.x;   // lane = env: the batch-major pose reads are contiguous across the wavefront
  if (env >= num_envs) return;
  float T[12];
  smj_points_env_transform(kind, xpose, ld, env, cam_bodyid, cam_pos, cam_mat, cam, body, T);
  for (int k = 0; k < 12; k++) ws[12 * (long)env + k] = T[k];
}

__global__ __launch_bounds__(PT_THREADS) void smj_points_kernel(const float* __restrict__ depth, const float* __restrict__ ws, float* __restrict__ out,
                                                                long long N, int width, int height, int wp, int hp, int stride, float th,
                                                                float aspect, int vec_in, int vec_out) {
  __shared__ float4 stage4[3 * PT_THREADS];   // the workgroup's 1024 points, xyz interleaved as in the output
  float* stage = reinterpret_cast<float*>(stage4);
  const int tid = threadIdx.x;
  const long long base = (long long)blockIdx.x * PT_PER_BLOCK, p0 = base + PT_PER_THREAD * tid;
  if (p0 < N) {
    int env[4], gi[4], gj[4];
    smj_points_unflatten(p0, wp, hp, &env[0], &gi[0], &gj[0]);
    for (int k = 1; k < 4; k++) {
      env[k] = env[k - 1]; gi[k] = gi[k - 1]; gj[k] = gj[k - 1];
      smj_points_next(wp, hp, &env[k], &gi[k], &gj[k]);
    }
    const int n = N - p0 < 4 ? (int)(N - p0) : 4;   // points of this group inside the array
    float d[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec_in && n == 4) {   // stride 1: the flat depth index is the point index
      const float4 q = *reinterpret_cast<const float4*>(depth + p0);
      d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    } else {
      for (int k = 0; k < n; k++) {
        int u, v;
        smj_points_pixel(gi[k], gj[k], stride, &u, &v);
        d[k] = depth[((long long)env[k] * height + v) * width + u];
      }
    }
    float T[12], pt[12];
    int have = -1;
    for (int k = 0; k < 4; k++) {
      if (k < n) {
        if (env[k] != have) {   // once per thread; a second time only where the group straddles two envs
          const float4* Tp = reinterpret_cast<const float4*>(ws + 12 * (long)env[k]);
          const float4 a = Tp[0], b = Tp[1], c = Tp[2];
          T[0] = a.x; T[1] = a.y; T[2] = a.z; T[3] = a.w; T[4] = b.x; T[5] = b.y; T[6] = b.z; T[7] = b.w;
          T[8] = c.x; T[9] = c.y; T[10] = c.z; T[11] = c.w;
          have = env[k];
        }
        int u, v;
        float xn, yn;
        smj_points_pixel(gi[k], gj[k], stride, &u, &v);
        smj_points_dir(u, v, width, height, th, aspect, &xn, &yn);
        smj_points_point(d[k], xn, yn, T, pt + 3 * k);
      } else {
        pt[3 * k] = pt[3 * k + 1] = pt[3 * k + 2] = 0.f;   // past the end of the array: staged, never stored
      }
    }
    for (int m = 0; m < 3; m++) stage4[3 * tid + m] = make_float4(pt[4 * m], pt[4 * m + 1], pt[4 * m + 2], pt[4 * m + 3]);
  }
  __syncthreads();
  const long long left = 3 * (N - base);   // floats of the output from this workgroup's first one to the end of the array
  const int nf = left < 3 * PT_PER_BLOCK ? (int)left : 3 * PT_PER_BLOCK;
  float* o = out + 3 * base;
  if (vec_out) {
    for (int m = 0; m < 3; m++) {
      const int q = tid + PT_THREADS * m, f = 4 * q;
      if (f + 4 <= nf) *reinterpret_cast<float4*>(o + f) = stage4[q];
      else
        for (int c = 0; c < 4; c++)
          if (f + c < nf) o[f + c] = stage[f + c];
    }
  } else {
    for (int m = 0; m < 12; m++) {
      const int f = tid + PT_THREADS * m;
      if (f < nf) o[f] = stage[f];
    }
  }
}

size_t smj_points_workspace_bytes(int num_envs) { return sizeof(float) * 12 * (size_t)num_envs; }

void smj_launch_points(const float* xpose, long ld, int num_envs, const int* cam_bodyid, const float* cam_pos, const float* cam_mat,
                       int cam, int width, int height, float fovy_deg, const float* depth, int stride, int kind, int body,
                       float* points, float* workspace, hipStream_t stream) {
  const int wp = smj_points_grid(width, stride), hp = smj_points_grid(height, stride);
  const long long N = (long long)num_envs * wp * hp;
  const float th = tanf(fovy_deg * 3.14159265358979323846f / 360.f);   // as smj_launch_depth
  const float aspect = (float)width / (float)height;
  const int vec_in = stride == 1 && ((uintptr_t)depth & 15) == 0, vec_out = ((uintptr_t)points & 15) == 0;
  hipLaunchKernelGGL(smj_points_prepass, dim3((num_envs + 63) / 64), dim3(64), 0, stream, xpose, ld, num_envs, cam_bodyid, cam_pos, cam_mat,
                     cam, kind, body, workspace);
  hipLaunchKernelGGL(smj_points_kernel, dim3((unsigned)((N + PT_PER_BLOCK - 1) / PT_PER_BLOCK)), dim3(PT_THREADS), 0, stream, depth, workspace,
                     points, N, width, height, wp, hp, stride, th, aspect, vec_in, vec_out);
}
