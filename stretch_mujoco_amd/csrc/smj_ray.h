// Ray against a primitive geom in the geom's own frame: what the lidar kernel (either side of a surface, [MJ] mj_rayGeom) and the
// depth cameras' per-pixel kernel (entering side only, from tnear on) of smj_render.hip share.  Host-and-device functions, so that
// a host compiler can evaluate the very arithmetic the kernels run (tests/ray/ray_check.cpp).
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SMJ_RAY_HD __host__ __device__ inline
#define SMJ_RAY_UNROLL _Pragma("unroll")
#else
#define SMJ_RAY_HD static inline
#define SMJ_RAY_UNROLL
#endif

enum { RT_PLANE = 0, RT_SPHERE = 2, RT_CAPSULE = 3, RT_ELLIPSOID = 4, RT_CYLINDER = 5, RT_BOX = 6, RT_MESH = 7 };

SMJ_RAY_HD float ray_dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// The two roots x0 <= x1 of |p + x v|^2 = r2, false when the line misses (or grazes within rounding).  Through the point of closest
// approach: t_c = -(v.p) / (v.v), q = p + t_c v, x = t_c -+ sqrt((r2 - |q|^2) / (v.v)).  The textbook discriminant
// (v.p)^2 - (v.v)(|p|^2 - r2) subtracts two numbers of the size |p|^2 to get one of the size r2: in fp32 a 2 cm leg 10 m away came
// out 2.4 mm off and a 1 cm one was missed by some rays; here the only cancellation is in q, whose error is an ulp of |p|, and the
// error of the root stays within a few ulp of the distance ("Lidar rays against an independent reference").
SMJ_RAY_HD bool ray_roots(const float* p, const float* v, float r2, float* x0, float* x1) {
  const float a = ray_dot3(v, v), tc = -ray_dot3(v, p) / a;
  const float q[3] = {p[0] + tc * v[0], p[1] + tc * v[1], p[2] + tc * v[2]};
  const float h = r2 - ray_dot3(q, q);
  if (h * a < 1e-15f) return false;
  const float s = sqrtf(h / a);
  *x0 = tc - s;
  *x1 = tc + s;
  return true;
}
// nearest root that is not behind the origin (either side of the surface), or -1
SMJ_RAY_HD float ray_quad(const float* p, const float* v, float r2) {
  float x0, x1;
  if (!ray_roots(p, v, r2, &x0, &x1)) return -1.f;
  if (x0 >= 0) return x0;
  if (x1 >= 0) return x1;
  return -1.f;
}

// entering intersection of the ray with a primitive in its own frame (outside faces only), or -1
SMJ_RAY_HD float ray_prim(int type, const float* size, const float* lp, const float* lv, float tnear) {
  if (type == RT_PLANE) {
    if (lv[2] > -1e-15f) return -1.f;
    const float x = -lp[2] / lv[2];
    if (x < tnear) return -1.f;
    const float px = lp[0] + x * lv[0], py = lp[1] + x * lv[1];
    if ((size[0] <= 0 || fabsf(px) <= size[0]) && (size[1] <= 0 || fabsf(py) <= size[1])) return x;
    return -1.f;
  }
  if (type == RT_SPHERE) {
    float x0, x1;
    if (!ray_roots(lp, lv, size[0] * size[0], &x0, &x1)) return -1.f;
    return x0 >= tnear ? x0 : -1.f;
  }
  if (type == RT_CYLINDER) {
    float best = -1.f;
    const float p2[3] = {lp[0], lp[1], 0.f}, v2[3] = {lv[0], lv[1], 0.f};
    float x0, x1;
    if (ray_dot3(v2, v2) > 1e-15f && ray_roots(p2, v2, size[0] * size[0], &x0, &x1)) {
      if (x0 >= tnear && fabsf(lp[2] + x0 * lv[2]) <= size[1]) best = x0;
    }
    if (fabsf(lv[2]) > 1e-15f) {
      const float sg = lv[2] < 0 ? 1.f : -1.f;   // the cap facing the ray
      const float x = (sg * size[1] - lp[2]) / lv[2];
      if (x >= tnear) {
        const float px = lp[0] + x * lv[0], py = lp[1] + x * lv[1];
        if (px * px + py * py <= size[0] * size[0] && (best < 0 || x < best)) best = x;
      }
    }
    return best;
  }
  if (type == RT_BOX) {
    float best = -1.f;
    SMJ_RAY_UNROLL
    for (int ax = 0; ax < 3; ax++) {
      if (fabsf(lv[ax]) < 1e-15f) continue;
      const float sg = lv[ax] < 0 ? 1.f : -1.f;   // the face of this axis that faces the ray
      const float x = (sg * size[ax] - lp[ax]) / lv[ax];
      if (x < tnear) continue;
      const int a1 = (ax + 1) % 3, a2 = (ax + 2) % 3;
      if (fabsf(lp[a1] + x * lv[a1]) <= size[a1] && fabsf(lp[a2] + x * lv[a2]) <= size[a2] && (best < 0 || x < best)) best = x;
    }
    return best;
  }
  if (type == RT_CAPSULE) {
    float best = -1.f;
    const float p2[3] = {lp[0], lp[1], 0.f}, v2[3] = {lv[0], lv[1], 0.f};
    float x0, x1;
    if (ray_dot3(v2, v2) > 1e-15f && ray_roots(p2, v2, size[0] * size[0], &x0, &x1)) {
      if (x0 >= tnear && fabsf(lp[2] + x0 * lv[2]) <= size[1]) best = x0;
    }
    for (int sg = -1; sg <= 1; sg += 2) {
      const float q[3] = {lp[0], lp[1], lp[2] - sg * size[1]};
      if (!ray_roots(q, lv, size[0] * size[0], &x0, &x1)) continue;
      if (x0 >= tnear && sg * (lp[2] + x0 * lv[2]) >= size[1] && (best < 0 || x0 < best)) best = x0;
    }
    return best;
  }
  if (type == RT_ELLIPSOID) {
    const float s[3] = {1.f / size[0], 1.f / size[1], 1.f / size[2]};
    const float v[3] = {lv[0] * s[0], lv[1] * s[1], lv[2] * s[2]}, p[3] = {lp[0] * s[0], lp[1] * s[1], lp[2] * s[2]};
    float x0, x1;
    if (!ray_roots(p, v, 1.f, &x0, &x1)) return -1.f;
    return x0 >= tnear ? x0 : -1.f;
  }
  return -1.f;
}

// nearest intersection (either side) of a ray with a primitive in its own frame, or -1.  [MJ] mj_rayGeom
SMJ_RAY_HD float ray_prim_any(int type, const float* size, const float* lp, const float* lv) {
  if (type == RT_PLANE) {
    if (lv[2] > -1e-15f) return -1.f;
    const float x = -lp[2] / lv[2];
    if (x < 0) return -1.f;
    const float px = lp[0] + x * lv[0], py = lp[1] + x * lv[1];
    if ((size[0] <= 0 || fabsf(px) <= size[0]) && (size[1] <= 0 || fabsf(py) <= size[1])) return x;
    return -1.f;
  }
  if (type == RT_SPHERE) return ray_quad(lp, lv, size[0] * size[0]);
  if (type == RT_CYLINDER) {
    float best = -1.f;
    const float p2[3] = {lp[0], lp[1], 0.f}, v2[3] = {lv[0], lv[1], 0.f};
    if (ray_dot3(v2, v2) > 1e-15f) {
      const float x = ray_quad(p2, v2, size[0] * size[0]);
      if (x >= 0 && fabsf(lp[2] + x * lv[2]) <= size[1]) best = x;
    }
    if (fabsf(lv[2]) > 1e-15f)
      for (int sg = -1; sg <= 1; sg += 2) {
        const float x = (sg * size[1] - lp[2]) / lv[2];
        if (x >= 0) {
          const float px = lp[0] + x * lv[0], py = lp[1] + x * lv[1];
          if (px * px + py * py <= size[0] * size[0] && (best < 0 || x < best)) best = x;
        }
      }
    return best;
  }
  if (type == RT_BOX) {
    float best = -1.f;
    SMJ_RAY_UNROLL
    for (int ax = 0; ax < 3; ax++) {
      if (fabsf(lv[ax]) < 1e-15f) continue;
      for (int sg = -1; sg <= 1; sg += 2) {
        const float x = (sg * size[ax] - lp[ax]) / lv[ax];
        if (x < 0) continue;
        const int a1 = (ax + 1) % 3, a2 = (ax + 2) % 3;
        if (fabsf(lp[a1] + x * lv[a1]) <= size[a1] && fabsf(lp[a2] + x * lv[a2]) <= size[a2] && (best < 0 || x < best)) best = x;
      }
    }
    return best;
  }
  if (type == RT_CAPSULE) {   // the cylinder's side between the caps, then the two end spheres beyond them
    float best = -1.f;
    const float p2[3] = {lp[0], lp[1], 0.f}, v2[3] = {lv[0], lv[1], 0.f};
    float x[2];
    if (ray_dot3(v2, v2) > 1e-15f && ray_roots(p2, v2, size[0] * size[0], &x[0], &x[1])) {
      for (int k = 0; k < 2; k++)
        if (x[k] >= 0 && fabsf(lp[2] + x[k] * lv[2]) <= size[1] && (best < 0 || x[k] < best)) best = x[k];
    }
    for (int sg = -1; sg <= 1; sg += 2) {
      const float q[3] = {lp[0], lp[1], lp[2] - sg * size[1]};
      if (!ray_roots(q, lv, size[0] * size[0], &x[0], &x[1])) continue;
      for (int k = 0; k < 2; k++)
        if (x[k] >= 0 && sg * (lp[2] + x[k] * lv[2]) >= size[1] && (best < 0 || x[k] < best)) best = x[k];
    }
    return best;
  }
  if (type == RT_ELLIPSOID) {
    const float sc[3] = {1.f / size[0], 1.f / size[1], 1.f / size[2]};
    const float v[3] = {lv[0] * sc[0], lv[1] * sc[1], lv[2] * sc[2]}, q[3] = {lp[0] * sc[0], lp[1] * sc[1], lp[2] * sc[2]};
    return ray_quad(q, v, 1.f);
  }
  return -1.f;
}
