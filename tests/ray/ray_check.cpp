// Host harness of the ray-primitive arithmetic (stretch_mujoco_amd/csrc/smj_ray.h): ray_prim_any (the lidar kernel: either side of a
// surface), ray_prim (the depth cameras: entering side, from tnear on) and ray_quad, evaluated in fp32 on the host against fp64 closed
// forms written here in another way -- every closed shape as the INTERVAL of the line inside it (slabs for the box, a disc interval cut
// by a slab for the cylinder, the hull of three intervals for the capsule), the answer being the interval's first end that is not
// behind the origin.  Rays are generated in the geom's frame, in fp64, and rounded to fp32 for both sides of the comparison:
//   (a) general poses, hits aimed at a point well inside the shape and misses aimed well outside;   (b) the origin inside;
//   (c) exact alignments: components that are exactly 0, rays in the plane of a box face, along a cylinder's axis;
//   (d) far and thin: r = 1, 2, 5 cm at 3, 6, 9.9 m, aimed within 0.9 r;
//   (e) ray_prim with a near plane: tnear below and beyond the entry, the origin inside, unnormalised directions, planes of every bound.
// The bound of each group is 16 x its input-rounding floor, the largest change of the fp64 answer when the ray and the sizes are
// rounded to fp32 ("Lidar rays against an independent reference"); hit or miss must agree on every ray.  Prints "ok".
#include "smj_ray.h"
#include "host_check.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

struct Ray { double p[3], v[3]; };
struct Span { double t0, t1; bool any; };   // the part of the line inside a closed convex shape

static Span none() { return {0, 0, false}; }
static Span all() { return {-1e300, 1e300, true}; }
static Span cut(Span a, Span b) {
  if (!a.any || !b.any) return none();
  const Span s = {std::max(a.t0, b.t0), std::min(a.t1, b.t1), true};
  return s.t0 <= s.t1 ? s : none();
}
static Span hull(Span a, Span b) {
  if (!a.any) return b;
  if (!b.any) return a;
  return {std::min(a.t0, b.t0), std::max(a.t1, b.t1), true};
}
static Span slab(double p, double v, double h) {   // |p + t v| <= h
  if (v == 0) return std::fabs(p) <= h ? all() : none();
  const double a = (-h - p) / v, b = (h - p) / v;
  return {std::min(a, b), std::max(a, b), true};
}
static Span ball(const double* p, const double* v, int n, double r) {   // |p + t v| <= r over the first n components
  double a = 0, b = 0, c = -r * r;
  for (int k = 0; k < n; k++) { a += v[k] * v[k]; b += v[k] * p[k]; c += p[k] * p[k]; }
  if (a == 0) return c <= 0 ? all() : none();
  const double disc = b * b - a * c;
  if (disc < 0) return none();
  const double s = std::sqrt(disc);
  return {(-b - s) / a, (-b + s) / a, true};
}
static Span inside(int type, const double* size, const Ray& r) {
  if (type == RT_SPHERE) return ball(r.p, r.v, 3, size[0]);
  if (type == RT_BOX) return cut(cut(slab(r.p[0], r.v[0], size[0]), slab(r.p[1], r.v[1], size[1])), slab(r.p[2], r.v[2], size[2]));
  if (type == RT_CYLINDER) return cut(ball(r.p, r.v, 2, size[0]), slab(r.p[2], r.v[2], size[1]));
  if (type == RT_CAPSULE) {
    Span s = cut(ball(r.p, r.v, 2, size[0]), slab(r.p[2], r.v[2], size[1]));
    for (int sg = -1; sg <= 1; sg += 2) {
      const double q[3] = {r.p[0], r.p[1], r.p[2] - sg * size[1]};
      s = hull(s, ball(q, r.v, 3, size[0]));
    }
    return s;
  }
  if (type == RT_ELLIPSOID) {
    const double q[3] = {r.p[0] / size[0], r.p[1] / size[1], r.p[2] / size[2]}, w[3] = {r.v[0] / size[0], r.v[1] / size[1], r.v[2] / size[2]};
    return ball(q, w, 3, 1.0);
  }
  return none();
}
// either side: the first end of the span that is not behind the origin.  front: the entering end, from tnear on
static double ref_any(int type, const double* size, const Ray& r) {
  if (type == RT_PLANE) {
    if (!(r.v[2] < 0) || r.p[2] < 0) return -1;
    const double t = r.p[2] / -r.v[2], x = r.p[0] + t * r.v[0], y = r.p[1] + t * r.v[1];
    return ((size[0] <= 0 || std::fabs(x) <= size[0]) && (size[1] <= 0 || std::fabs(y) <= size[1])) ? t : -1;
  }
  const Span s = inside(type, size, r);
  if (!s.any) return -1;
  return s.t0 >= 0 ? s.t0 : (s.t1 >= 0 ? s.t1 : -1);
}
static double ref_front(int type, const double* size, const Ray& r, double tnear) {
  if (type == RT_PLANE) { const double t = ref_any(type, size, r); return t >= tnear ? t : -1; }
  const Span s = inside(type, size, r);
  return (s.any && s.t0 >= tnear) ? s.t0 : -1;
}

static Ray rounded(const Ray& r) {
  Ray o;
  for (int k = 0; k < 3; k++) { o.p[k] = (double)(float)r.p[k]; o.v[k] = (double)(float)r.v[k]; }
  return o;
}

struct Group {
  const char* name;
  double floor = 0, err = 0;
  int rays = 0, hits = 0;
};

// one ray through the three evaluations: fp64 on the fp64 ray (the floor), fp64 and fp32 on the rounded ray (the error)
static void probe(Group& g, int type, const double* size64, const Ray& r, int want_hit) {
  float size[3], lp[3], lv[3];
  double sized[3];
  for (int k = 0; k < 3; k++) { size[k] = (float)size64[k]; sized[k] = size[k]; }
  const Ray rr = rounded(r);
  for (int k = 0; k < 3; k++) { lp[k] = (float)r.p[k]; lv[k] = (float)r.v[k]; }
  const double exact = ref_any(type, size64, r), ref = ref_any(type, sized, rr);
  const float got = ray_prim_any(type, size, lp, lv);
  g.rays++;
  CHECK((exact >= 0) == (want_hit != 0), "%s: type %d: the fp64 form says %g where the case was built to %s", g.name, type, exact, want_hit ? "hit" : "miss");
  CHECK((got >= 0) == (ref >= 0), "%s: type %d size %g %g %g: fp32 %g against fp64 %g (from %g %g %g along %g %g %g)", g.name, type, size64[0], size64[1], size64[2], got, ref,
        r.p[0], r.p[1], r.p[2], r.v[0], r.v[1], r.v[2]);
  if (exact >= 0 && ref >= 0) g.floor = std::max(g.floor, std::fabs(exact - ref));
  if (got >= 0 && ref >= 0) { g.err = std::max(g.err, std::fabs((double)got - ref)); g.hits++; }
  // the depth cameras' form: the entering side only, from tnear on
  const double front = ref_front(type, sized, rr, 0.0);
  const float gf = ray_prim(type, size, lp, lv, 0.f);
  CHECK((gf >= 0) == (front >= 0), "%s: type %d: ray_prim %g against fp64 %g", g.name, type, gf, front);
  if (gf >= 0 && front >= 0) {
    g.err = std::max(g.err, std::fabs((double)gf - front));
    CHECK(ray_prim(type, size, lp, lv, gf + 0.01f) < 0, "%s: type %d: ray_prim past tnear", g.name, type);
  }
}

static void finish(const Group& g) {
  printf("%-22s rays %5d hits %5d floor %.3e fp32 error %.3e ratio %.2f\n", g.name, g.rays, g.hits, g.floor, g.err, g.floor > 0 ? g.err / g.floor : 0.0);
  CHECK(g.hits > 0 && g.floor > 0 && g.err <= 16 * g.floor && g.err <= 1e-3, "%s: fp32 error %g above 16 x the floor %g", g.name, g.err, g.floor);
}

static const int TYPES[] = {RT_SPHERE, RT_CAPSULE, RT_ELLIPSOID, RT_CYLINDER, RT_BOX};
static void sizes_of(int type, double* s) {
  const double table[7][3] = {{0, 0, 0}, {0, 0, 0}, {0.35, 0, 0}, {0.2, 0.4, 0}, {0.5, 0.3, 0.2}, {0.3, 0.35, 0}, {0.4, 0.3, 0.25}};
  for (int k = 0; k < 3; k++) s[k] = table[type][k];
}
// a point of the shape's frame: `f` x the way from the centre to the surface along a random direction (f < 1: inside, f > 1: outside)
static void point_at(int type, const double* s, std::mt19937& g, double f, double* out) {
  std::normal_distribution<double> n(0, 1);
  double d[3] = {n(g), n(g), n(g)};
  const double l = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  for (double& x : d) x /= l;
  const Ray r = {{0, 0, 0}, {d[0], d[1], d[2]}};
  const double reach = inside(type, s, r).t1;
  for (int k = 0; k < 3; k++) out[k] = f * reach * d[k];
}
static Ray towards(const double* from, const double* to) {
  Ray r;
  double l = 0;
  for (int k = 0; k < 3; k++) { r.p[k] = from[k]; r.v[k] = to[k] - from[k]; l += r.v[k] * r.v[k]; }
  for (double& x : r.v) x /= std::sqrt(l);
  return r;
}

static void check_general_poses() {   // (a)
  Group g{"(a) general poses"};
  std::mt19937 gen(11);
  std::uniform_real_distribution<double> far(1.0, 5.0);
  for (int type : TYPES) {
    double s[3];
    sizes_of(type, s);
    for (int i = 0; i < 2000; i++) {
      double from[3], to[3];
      point_at(type, s, gen, 1.0, from);
      const double l = std::sqrt(from[0] * from[0] + from[1] * from[1] + from[2] * from[2]), d = far(gen);
      for (double& x : from) x *= (l + d) / l;
      point_at(type, s, gen, 0.9, to);
      probe(g, type, s, towards(from, to), 1);
      // a miss: aimed at a point of a sphere of twice the bounding radius, across the line of sight
      const double R = 2.0 * (s[0] + s[1] + s[2]);
      double side[3] = {from[1], -from[0], 0.3 * from[2] + 0.1};
      const double along = (side[0] * from[0] + side[1] * from[1] + side[2] * from[2]) / ((l + d) * (l + d));
      for (int k = 0; k < 3; k++) side[k] -= along * from[k];
      const double lt = std::sqrt(side[0] * side[0] + side[1] * side[1] + side[2] * side[2]);
      for (int k = 0; k < 3; k++) to[k] = R * side[k] / lt;
      probe(g, type, s, towards(from, to), 0);
    }
  }
  // planes: infinite and finite, from the front at general incidence; from behind; outside the half sizes
  std::uniform_real_distribution<double> u(-1, 1);
  for (int i = 0; i < 2000; i++) {
    const double inf[3] = {0, 0, 1}, fin[3] = {1.5, 1.0, 1};
    const double from[3] = {3 * u(gen), 3 * u(gen), 0.2 + 2 * std::fabs(u(gen))}, in[3] = {1.3 * u(gen), 0.9 * u(gen), 0}, out[3] = {1.7 + std::fabs(u(gen)), 3 * u(gen), 0};
    probe(g, RT_PLANE, inf, towards(from, in), 1);
    probe(g, RT_PLANE, fin, towards(from, in), 1);
    probe(g, RT_PLANE, fin, towards(from, out), 0);
    const double below[3] = {from[0], from[1], -from[2]};
    probe(g, RT_PLANE, inf, towards(below, in), 0);
  }
  finish(g);
}

static void check_origin_inside() {   // (b)
  Group g{"(b) origin inside"};
  std::mt19937 gen(12);
  for (int type : TYPES) {
    double s[3];
    sizes_of(type, s);
    for (int i = 0; i < 2000; i++) {
      double from[3], to[3];
      point_at(type, s, gen, 0.8 * (i % 10) / 9.0, from);
      point_at(type, s, gen, 3.0, to);
      probe(g, type, s, towards(from, to), 1);
    }
  }
  const double cap[3] = {0.2, 0.4, 0};   // the capsule: inside the cylindrical part and inside a cap
  for (int i = 0; i < 500; i++) {
    double to[3];
    point_at(RT_CAPSULE, cap, gen, 3.0, to);
    const double side[3] = {0.05, 0.04, 0.1}, end[3] = {0.03, -0.02, 0.47};
    probe(g, RT_CAPSULE, cap, towards(side, to), 1);
    probe(g, RT_CAPSULE, cap, towards(end, to), 1);
  }
  finish(g);
}

static void check_exact_alignments() {   // (c)
  Group g{"(c) exact alignments"};
  std::mt19937 gen(13);
  std::uniform_real_distribution<double> u(-1, 1);
  for (int type : TYPES) {
    double s[3];
    sizes_of(type, s);
    for (int ax = 0; ax < 3; ax++)
      for (int sg = -1; sg <= 1; sg += 2)
        for (int i = 0; i < 200; i++) {
          // along an axis (two components exactly 0) through a point well inside, from outside; one in four from the axis itself
          double through[3];
          point_at(type, s, gen, 0.7, through);
          if (i % 4 == 0) through[0] = through[1] = through[2] = 0;
          Ray r = {{through[0], through[1], through[2]}, {0, 0, 0}};
          r.p[ax] = -sg * (2.0 + u(gen));
          r.v[ax] = sg;
          probe(g, type, s, r, 1);
          // in a coordinate plane (one component exactly 0)
          double start[3] = {r.p[0], r.p[1], r.p[2]};
          start[(ax + 1) % 3] += 0.3 * u(gen);
          const Ray q = towards(start, through);   // (the third component of start and through is the same number)
          probe(g, type, s, q, 1);
        }
  }
  // rays in the plane of a box face that pass beside the face, and over a cylinder's cap in the cap's plane: clean misses
  const double box[3] = {0.4, 0.3, 0.25}, cyl[3] = {0.3, 0.35, 0};
  for (int i = 0; i < 200; i++) {
    const Ray a = {{-2.0, 0.3, 0.25 + 0.2 + std::fabs(u(gen))}, {1, 0, 0}}, b = {{0.4, -3.0, 0.5 + std::fabs(u(gen))}, {0, 1, 0}}, c = {{-2.0, 0.5 + std::fabs(u(gen)), 0.35}, {1, 0, 0}};
    probe(g, RT_BOX, box, a, 0);
    probe(g, RT_BOX, box, b, 0);
    probe(g, RT_CYLINDER, cyl, c, 0);
  }
  // along a cylinder's and a capsule's axis: the side has no quadratic at all
  const double capsule[3] = {0.2, 0.4, 0};
  for (int sg = -1; sg <= 1; sg += 2) {
    const Ray a = {{0, 0, -sg * 2.5}, {0, 0, (double)sg}}, b = {{0.1, -0.05, -sg * 1.7}, {0, 0, (double)sg}}, c = {{0.05, 0.02, 0.1}, {0, 0, (double)sg}};
    for (const Ray& r : {a, b, c}) { probe(g, RT_CYLINDER, cyl, r, 1); probe(g, RT_CAPSULE, capsule, r, 1); }
  }
  finish(g);
}

static void check_far_and_thin() {   // (d)
  std::mt19937 gen(14);
  std::uniform_real_distribution<double> u(-1, 1);
  for (double dist : {3.0, 6.0, 9.9}) {
    char name[64];
    snprintf(name, sizeof name, "(d) thin at %.1f m", dist);
    Group g{name};
    for (double r : {0.01, 0.02, 0.05})
      for (int type : {RT_SPHERE, RT_CAPSULE, RT_CYLINDER})
        for (int i = 0; i < 2000; i++) {
          const double s[3] = {r, 0.2, 0};
          // from `dist` away in a random direction across the axis, aimed at a point within 0.9 r of the axis
          const double a = 3.14159265358979 * u(gen), h = 0.15 * u(gen), off = 0.9 * r * u(gen);
          const double from[3] = {dist * std::cos(a), dist * std::sin(a), h + 0.5 * u(gen)}, to[3] = {-off * std::sin(a), off * std::cos(a), type == RT_SPHERE ? 0.0 : h};
          probe(g, type, s, towards(from, to), 1);
        }
    finish(g);
  }
}

// (e) the depth cameras' form with a near plane and an unnormalised direction (pixel rays are (x, y, -1) turned into the geom's frame):
// with tnear below the entry the entry comes back, within the bound; with tnear beyond it -1 -- never the far side; from inside -1
static void probe_front(Group& g, int type, const double* size64, const Ray& r, int want_hit) {
  float size[3], lp[3], lv[3];
  double sized[3];
  for (int k = 0; k < 3; k++) { size[k] = (float)size64[k]; sized[k] = size[k]; lp[k] = (float)r.p[k]; lv[k] = (float)r.v[k]; }
  const Ray rr = rounded(r);
  const double exact = ref_front(type, size64, r, 0.0), ref = ref_front(type, sized, rr, 0.0);
  g.rays++;
  CHECK((exact >= 0) == (want_hit != 0), "%s: type %d: the fp64 form says %g where the case was built to %s", g.name, type, exact, want_hit ? "hit" : "miss");
  if (ref < 0) {
    for (float tn : {0.f, 0.02f, 1.f}) CHECK(ray_prim(type, size, lp, lv, tn) < 0, "%s: type %d: a hit at tnear %g where fp64 has none", g.name, type, tn);
    return;
  }
  if (exact >= 0) g.floor = std::max(g.floor, std::fabs(exact - ref));
  for (double f : {0.0, 0.5, 0.999}) {
    const float got = ray_prim(type, size, lp, lv, (float)(f * ref));
    CHECK(got >= 0, "%s: type %d: entry %g lost at tnear %g", g.name, type, ref, f * ref);
    if (got >= 0) { g.err = std::max(g.err, std::fabs((double)got - ref)); g.hits++; }
  }
  for (double tn : {ref * 1.001 + 1e-4, ref * 1.5, ref * 4.0})
    CHECK(ray_prim(type, size, lp, lv, (float)tn) < 0, "%s: type %d: entry %g, tnear %g: something came back", g.name, type, ref, tn);
}

static void check_near_plane() {   // (e)
  Group g{"(e) entering, tnear"};
  std::mt19937 gen(15);
  std::uniform_real_distribution<double> far(0.05, 5.0), stretch(1.0, 1.6), u(-1, 1);
  for (int type : TYPES) {
    double s[3];
    sizes_of(type, s);
    for (int i = 0; i < 2000; i++) {
      double from[3], to[3];
      point_at(type, s, gen, 1.0, from);
      const double l = std::sqrt(from[0] * from[0] + from[1] * from[1] + from[2] * from[2]), d = far(gen), k = stretch(gen);
      for (double& x : from) x *= (l + d) / l;
      point_at(type, s, gen, 0.9, to);
      Ray r = towards(from, to);
      for (double& x : r.v) x *= k;
      probe_front(g, type, s, r, 1);
      // from inside: nothing, whatever tnear
      point_at(type, s, gen, 0.8 * (i % 10) / 9.0, from);
      point_at(type, s, gen, 3.0, to);
      Ray q = towards(from, to);
      for (double& x : q.v) x *= k;
      probe_front(g, type, s, q, 0);
    }
  }
  for (int i = 0; i < 2000; i++) {
    const double inf[3] = {0, 0, 1}, fin[3] = {1.5, 1.0, 1}, half[3] = {0, 1.0, 1};
    const double from[3] = {3 * u(gen), 3 * u(gen), 0.2 + 2 * std::fabs(u(gen))}, in[3] = {1.3 * u(gen), 0.9 * u(gen), 0}, out[3] = {3 * u(gen), 1.2 + std::fabs(u(gen)), 0};
    Ray a = towards(from, in), b = towards(from, out);
    const double k = stretch(gen);
    for (double& x : a.v) x *= k;
    for (double& x : b.v) x *= k;
    probe_front(g, RT_PLANE, inf, a, 1);
    probe_front(g, RT_PLANE, fin, a, 1);
    probe_front(g, RT_PLANE, half, a, 1);
    probe_front(g, RT_PLANE, half, b, 0);
    probe_front(g, RT_PLANE, fin, b, 0);
  }
  finish(g);
}

static void check_quad_rule() {
  // the nearest root that is not behind the origin, -1 when the line misses or the sphere lies behind
  const float v[3] = {1, 0, 0}, ahead[3] = {-3, 0, 0}, in[3] = {0.25f, 0, 0}, behind[3] = {3, 0, 0}, beside[3] = {-3, 0.75f, 0};
  CHECK(ray_quad(ahead, v, 0.25f) == 2.5f && ray_quad(in, v, 0.25f) == 0.25f && ray_quad(behind, v, 0.25f) == -1.f && ray_quad(beside, v, 0.25f) == -1.f, "ray_quad's rule");
  float x0 = 0, x1 = 0;
  CHECK(ray_roots(ahead, v, 0.25f, &x0, &x1) && x0 == 2.5f && x1 == 3.5f && !ray_roots(beside, v, 0.25f, &x0, &x1), "ray_roots");
  const float size[3] = {0.5f, 0, 0};
  CHECK(ray_prim_any(RT_MESH, size, ahead, v) == -1.f && ray_prim(RT_MESH, size, ahead, v, 0.f) == -1.f, "a mesh is not a primitive");
}

int main() {
  check_quad_rule();
  check_general_poses();
  check_origin_inside();
  check_exact_alignments();
  check_far_and_thin();
  check_near_plane();
  if (failures) { printf("%d failures\n", failures); return 1; }
  printf("ok\n");
  return 0;
}
