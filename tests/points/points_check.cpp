// Host harness of the point-cloud arithmetic (stretch_mujoco_amd/csrc/smj_points.h): the inline functions the HIP kernels call,
// compiled for the host and checked against long-hand fp64 -- the index mapping (every grid cell of every env hit exactly once,
// nothing out of range), the per-pixel point in the three frame kinds, the NaN rule.  Prints "ok" at the end.
#include "smj_points.h"
#include "host_check.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

static void check_mapping(int W, int H, int s, int num_envs) {
  const int wp = smj_points_grid(W, s), hp = smj_points_grid(H, s);
  CHECK(wp == (int)std::ceil((double)W / s) && hp == (int)std::ceil((double)H / s), "grid %d %d %d", W, H, s);
  const long long N = (long long)num_envs * wp * hp;
  std::vector<int> hits((size_t)N, 0);
  std::vector<int> pix((size_t)W * H, 0);
  int ce = 0, ci = 0, cj = 0;   // the chain of smj_points_next from point 0
  for (long long p = 0; p < N; p++) {
    int env, i, j, u, v;
    smj_points_unflatten(p, wp, hp, &env, &i, &j);
    CHECK(env >= 0 && env < num_envs && i >= 0 && i < hp && j >= 0 && j < wp, "point %lld -> (%d, %d, %d) out of range", p, env, i, j);
    CHECK(((long long)env * hp + i) * wp + j == p, "point %lld -> (%d, %d, %d) is not its own index", p, env, i, j);
    CHECK(env == ce && i == ci && j == cj, "point %lld: next() chain (%d, %d, %d) != unflatten (%d, %d, %d)", p, ce, ci, cj, env, i, j);
    smj_points_next(wp, hp, &ce, &ci, &cj);
    smj_points_pixel(i, j, s, &u, &v);
    CHECK(u == s * j && v == s * i && u >= 0 && u < W && v >= 0 && v < H, "grid (%d, %d) -> pixel (%d, %d) of %d x %d", i, j, u, v, W, H);
    if (env >= 0 && env < num_envs && i >= 0 && i < hp && j >= 0 && j < wp) hits[(size_t)(((long long)env * hp + i) * wp + j)]++;
    if (env == 0 && u >= 0 && u < W && v >= 0 && v < H) pix[(size_t)v * W + u]++;
  }
  for (long long p = 0; p < N; p++) CHECK(hits[(size_t)p] == 1, "cell %lld hit %d times", p, hits[(size_t)p]);
  for (int v = 0; v < H; v++)
    for (int u = 0; u < W; u++) CHECK(pix[(size_t)v * W + u] == ((u % s == 0 && v % s == 0) ? 1 : 0), "pixel (%d, %d) kept %d times at stride %d", u, v, pix[(size_t)v * W + u], s);
  // the kernel's groups of four: unflatten the first point, step to the next three (a group may straddle a row or an env)
  for (long long p0 = 0; p0 < N; p0 += 4) {
    int env, i, j;
    smj_points_unflatten(p0, wp, hp, &env, &i, &j);
    for (int k = 1; k < 4 && p0 + k < N; k++) {
      int e2, i2, j2;
      smj_points_next(wp, hp, &env, &i, &j);
      smj_points_unflatten(p0 + k, wp, hp, &e2, &i2, &j2);
      CHECK(env == e2 && i == i2 && j == j2, "group at %lld, point %d", p0, k);
    }
  }
}

// long-hand fp64 of one point from the same fp32 inputs
static void reference(int kind, const Pose& cb, const Pose& cam, const Pose& body, int u, int v, int W, int H, double fovy_deg, double d,
                      double* out, double* S) {
  const double th = std::tan(fovy_deg * M_PI / 360.0);
  const double xn = ((u + 0.5) / W * 2 - 1) * th * W / H, yn = (1 - (v + 0.5) / H * 2) * th;
  const double c[3] = {d * xn, d * yn, -d};
  *S = d * (std::fabs(xn) + std::fabs(yn) + 1);
  if (kind == SMJ_PT_CAMERA) {
    out[0] = d * xn; out[1] = -d * yn; out[2] = d;
    return;
  }
  double cpos[3], cmat[9], w[3];
  for (int i = 0; i < 3; i++) {
    cpos[i] = cb.p[i];
    for (int k = 0; k < 3; k++) cpos[i] += (double)cb.m[3 * i + k] * cam.p[k];
    for (int j = 0; j < 3; j++) {
      cmat[3 * i + j] = 0;
      for (int k = 0; k < 3; k++) cmat[3 * i + j] += (double)cb.m[3 * i + k] * cam.m[3 * k + j];
    }
  }
  for (int i = 0; i < 3; i++) w[i] = cpos[i] + cmat[3 * i] * c[0] + cmat[3 * i + 1] * c[1] + cmat[3 * i + 2] * c[2];
  for (int k = 0; k < 3; k++) *S += std::fabs((double)cb.p[k]) + std::fabs((double)cam.p[k]);
  if (kind == SMJ_PT_WORLD) {
    for (int i = 0; i < 3; i++) out[i] = w[i];
    return;
  }
  for (int k = 0; k < 3; k++) *S += std::fabs((double)body.p[k]);
  for (int i = 0; i < 3; i++) {
    out[i] = 0;
    for (int k = 0; k < 3; k++) out[i] += (double)body.m[3 * k + i] * (w[k] - body.p[k]);
  }
}

static void check_points() {
  std::mt19937 g(12345);
  std::uniform_real_distribution<double> U(0, 1);
  double worst = 0;
  for (int trial = 0; trial < 20000; trial++) {
    // image shapes between 1:2 and 2:1 (the cameras are 16:9, one of them on its side): the subtraction in xn rounds at
    // 2^-24 th W / H, which the bound below -- built from the size of the final terms -- covers only for moderate aspect ratios
    const int H = 1 + (int)(U(g) * 300), W = std::max(1, (int)(H * (0.5 + 1.5 * U(g))));
    const int u = (int)(U(g) * W), v = (int)(U(g) * H);
    const float fovy = (float)(20 + 80 * U(g));
    const float d = (float)(trial % 7 == 0 ? 50 * U(g) : 0.05 + 10 * U(g));
    const Pose cb = random_pose(g, 10), body = random_pose(g, 10);
    Pose cam = random_pose(g, 0.5);
    const float th = tanf(fovy * 3.14159265358979323846f / 360.f), aspect = (float)W / (float)H;
    float xn, yn;
    smj_points_dir(u, v, W, H, th, aspect, &xn, &yn);
    for (int kind : {SMJ_PT_CAMERA, SMJ_PT_WORLD, SMJ_PT_BODY}) {
      float T[12], got[3];
      if (kind == SMJ_PT_CAMERA) smj_points_transform(kind, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, T);   // nothing may be read
      else smj_points_transform(kind, cb.p, cb.m, cam.p, cam.m, kind == SMJ_PT_BODY ? body.p : nullptr, kind == SMJ_PT_BODY ? body.m : nullptr, T);
      smj_points_point(d, xn, yn, T, got);
      double want[3], S;
      if (d <= 0) continue;
      reference(kind, cb, cam, body, u, v, W, H, fovy, d, want, &S);
      const double tol = 32 * std::ldexp(1.0, -24) * S;   // the bound of the GPU test (tests/test_gpu_point_cloud.py has the derivation)
      for (int k = 0; k < 3; k++) {
        const double e = std::fabs(got[k] - want[k]);
        worst = std::max(worst, e / tol);
        CHECK(e <= tol, "kind %d comp %d: got %.9g want %.9g (err %.3g, tol %.3g)", kind, k, got[k], want[k], e, tol);
      }
      if (kind == SMJ_PT_CAMERA) {   // the optical frame is exact: d (xn, -yn, 1) in fp32
        CHECK(got[0] == d * xn && got[1] == -(d * yn) && got[2] == d, "camera frame is not d (xn, -yn, 1)");
      }
      const float inf = std::numeric_limits<float>::infinity();
      for (float bad : {0.f, -1.f, inf, -inf, std::numeric_limits<float>::quiet_NaN()}) {
        float o[3] = {1.f, 2.f, 3.f};
        smj_points_point(bad, xn, yn, T, o);
        CHECK(std::isnan(o[0]) && std::isnan(o[1]) && std::isnan(o[2]), "depth %g in kind %d is not three NaNs", bad, kind);
      }
    }
  }
  printf("worst error / tolerance %.3f\n", worst);
}

int main() {
  const int cases[][3] = {{37, 23, 1}, {37, 23, 3}, {5, 4, 7}, {1, 1, 1}, {424, 240, 5}};
  for (const auto& c : cases) check_mapping(c[0], c[1], c[2], 3);
  {   // (5, 4, 7): a stride larger than the image keeps pixel (0, 0) alone
    CHECK(smj_points_grid(5, 7) == 1 && smj_points_grid(4, 7) == 1, "stride beyond the image");
  }
  check_points();
  CHECK(smj_points_valid(1e-30f) && smj_points_valid(3.4e38f), "small / large finite depths are valid");
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
