// Organised point clouds from the depth images (smj_depth_to_points, include/smj_pointcloud.h): the per-pixel arithmetic, the index mapping
// and the per-env transform as plain inline functions.  The kernels of smj_points.hip call exactly these; the header also
// compiles under a host compiler, so tests/points/points_check.cpp checks the shipped code against long-hand fp64.
//
// Conventions.  The depth image is [num_envs][H][W], metres along the optical axis of a MuJoCo camera (x right, y up, looking
// down -z), row 0 at the top.  With stride s the cloud keeps the pixels (u, v) = (s j, s i): grid [H'][W'], H' = ceil(H / s),
// W' = ceil(W / s).  The cloud is one flat array of N = num_envs H' W' points of three floats; point p is (env, i, j) with
// p = (env H' + i) W' + j.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SMJ_PT_HD __host__ __device__ __forceinline__
#else
#define SMJ_PT_HD static inline
#endif

enum { SMJ_PT_CAMERA = 0, SMJ_PT_WORLD = 1, SMJ_PT_BODY = 2 };   // frame kinds of smj_points_transform

SMJ_PT_HD int smj_points_grid(int n, int stride) { return (n + stride - 1) / stride; }   // ceil(n / stride): kept pixels 0, s, 2s, ..

// point p -> (env, i, j).  per_env = H' W' fits 31 bits (the entry checks), p may not.
SMJ_PT_HD void smj_points_unflatten(long long p, int wp, int hp, int* env, int* i, int* j) {
  const long long per_env = (long long)wp * hp;
  const long long e = p / per_env;
  const unsigned rem = (unsigned)(p - e * per_env);
  const unsigned row = rem / (unsigned)wp;
  *env = (int)e;
  *i = (int)row;
  *j = (int)(rem - row * (unsigned)wp);
}

// (env, i, j) of point p -> that of point p + 1: what the kernel does for the second to fourth point of a group of four
// (a group may straddle a row or an env) instead of three more divisions
SMJ_PT_HD void smj_points_next(int wp, int hp, int* env, int* i, int* j) {
  if (++*j == wp) {
    *j = 0;
    if (++*i == hp) { *i = 0; ++*env; }
  }
}

// grid (i, j) -> image pixel (u, v) = (s j, s i); always inside the image because i < ceil(H / s)
SMJ_PT_HD void smj_points_pixel(int i, int j, int stride, int* u, int* v) { *u = stride * j; *v = stride * i; }

// Pixel centre -> direction (xn, yn, -1) in the MuJoCo camera frame: the ray caster's rule (smj_render.hip, non-raster form),
// th = tan(fovy / 2), aspect = (float)W / (float)H
SMJ_PT_HD void smj_points_dir(int u, int v, int width, int height, float th, float aspect, float* xn, float* yn) {
  *xn = ((u + 0.5f) / width * 2.f - 1.f) * th * aspect;
  *yn = (1.f - (v + 0.5f) / height * 2.f) * th;
}

// valid depth: finite and > 0 (0 is what limit_depth_distance leaves beyond the limit); a NaN fails the first compare
SMJ_PT_HD bool smj_points_valid(float d) { return d > 0.f && d <= 3.402823466e38f; }

// One point: T is the 3x4 transform [R | t] (row major, 12 floats) from the MuJoCo camera frame to the target frame.
// d (xn, yn, -1) in the camera frame, then R . + t.  An invalid depth gives three quiet NaNs (organised-cloud convention).
SMJ_PT_HD void smj_points_point(float d, float xn, float yn, const float* T, float* out) {
  if (!smj_points_valid(d)) {
    out[0] = out[1] = out[2] = __builtin_nanf("");
    return;
  }
  const float c[3] = {d * xn, d * yn, -d};
  out[0] = T[0] * c[0] + T[1] * c[1] + T[2] * c[2] + T[3];
  out[1] = T[4] * c[0] + T[5] * c[1] + T[6] * c[2] + T[7];
  out[2] = T[8] * c[0] + T[9] * c[1] + T[10] * c[2] + T[11];
}

// The per-env transform.  kind SMJ_PT_CAMERA: the constant diag(1, -1, -1) -- the optical frame (x right, y down, z forward):
// d (xn, -yn, 1); nothing else is read.  Otherwise the camera's world pose, composed as the depth renderer's staging pass does
// it (smj_depth_prepass) from the pose (cbp, cbm) of the camera's body and the model's cam_pos / cam_mat:
//   cpos = cbp + cbm cam_pos,  cmat = cbm cam_mat.
// SMJ_PT_WORLD: [cmat | cpos].  SMJ_PT_BODY: into the frame of the body with pose (bp, bm): [bm' cmat | bm' (cpos - bp)].
SMJ_PT_HD void smj_points_transform(int kind, const float* cbp, const float* cbm, const float* cam_pos, const float* cam_mat,
                                    const float* bp, const float* bm, float* T) {
  if (kind == SMJ_PT_CAMERA) {
    for (int k = 0; k < 12; k++) T[k] = 0.f;
    T[0] = 1.f; T[5] = -1.f; T[10] = -1.f;
    return;
  }
  float cpos[3], cmat[9];
  for (int i = 0; i < 3; i++) {
    cpos[i] = cbp[i] + (cbm[3 * i] * cam_pos[0] + cbm[3 * i + 1] * cam_pos[1] + cbm[3 * i + 2] * cam_pos[2]);
    for (int j = 0; j < 3; j++) cmat[3 * i + j] = cbm[3 * i] * cam_mat[j] + cbm[3 * i + 1] * cam_mat[3 + j] + cbm[3 * i + 2] * cam_mat[6 + j];
  }
  if (kind == SMJ_PT_WORLD) {
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) T[4 * i + j] = cmat[3 * i + j];
      T[4 * i + 3] = cpos[i];
    }
    return;
  }
  const float dp[3] = {cpos[0] - bp[0], cpos[1] - bp[1], cpos[2] - bp[2]};
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T[4 * i + j] = bm[i] * cmat[j] + bm[3 + i] * cmat[3 + j] + bm[6 + i] * cmat[6 + j];
    T[4 * i + 3] = bm[i] * dp[0] + bm[3 + i] * dp[1] + bm[6 + i] * dp[2];
  }
}

// Pose (p, m) of fused body `body` of env `env` from XPOSE, [nbody * 12][ld] batch-major: position, then the row-major 3x3
SMJ_PT_HD void smj_xpose_body(const float* xpose, long ld, int env, int body, float* p, float* m) {
  for (int k = 0; k < 3; k++) p[k] = xpose[(12 * body + k) * ld + env];
  for (int k = 0; k < 9; k++) m[k] = xpose[(12 * body + 3 + k) * ld + env];
}

// smj_points_transform for env `env` of camera `cam`, with the poses it needs read from XPOSE (none for SMJ_PT_CAMERA)
SMJ_PT_HD void smj_points_env_transform(int kind, const float* xpose, long ld, int env, const int* cam_bodyid, const float* cam_pos,
                                        const float* cam_mat, int cam, int body, float* T) {
  float cbp[3] = {}, cbm[9] = {}, bp[3] = {}, bm[9] = {};
  if (kind != SMJ_PT_CAMERA) {
    smj_xpose_body(xpose, ld, env, cam_bodyid[cam], cbp, cbm);
    if (kind == SMJ_PT_BODY) smj_xpose_body(xpose, ld, env, body, bp, bm);
  }
  smj_points_transform(kind, cbp, cbm, cam_pos + 3 * cam, cam_mat + 9 * cam, bp, bm, T);
}

#if defined(__HIPCC__)
// Launches (smj_points.hip).  workspace: smj_points_workspace_bytes(num_envs) of device memory, the per-env transforms.
// kind / body: SMJ_PT_* and, for SMJ_PT_BODY, the fused body; xpose [nbody*12][ld] batch-major (not read for SMJ_PT_CAMERA).
size_t smj_points_workspace_bytes(int num_envs);
void smj_launch_points(const float* xpose, long ld, int num_envs, const int* cam_bodyid, const float* cam_pos, const float* cam_mat,
                       int cam, int width, int height, float fovy_deg, const float* depth, int stride, int kind, int body,
                       float* points, float* workspace, hipStream_t stream);
#endif
