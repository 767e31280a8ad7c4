// C-ABI (include/smj.h) of the batched Stretch physics path for gfx950.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>
#include <stdarg.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/smj.h"
#include "../../include/smj_build.h"
#include "smj_kernels.h"
#include "smj_step_plan.h"
#include "smj_model_load.h"
#include "smj_bvh.h"
#include "smj_meshlet.h"
#include "smj_render.h"
#include "smj_points.h"
#include "smj_hmap.h"
#include "smj_occ.h"
#include "smj_edt.h"
#include "smj_nav.h"
#include "smj_front.h"
#include "smj_drive.h"
#include "smj_match.h"
#include "smj_map.h"
#include "smj_mcl.h"
#include "smj_scan.h"
#include "smj_comm.h"
static_assert(SMJ_READ_CR == SMJ_READ_CONTACTS && SMJ_CR_WORDS == SMJ_CONTACT_WORDS && SMJ_CR_DIST == SMJ_CON_DIST && SMJ_CR_POS == SMJ_CON_POS &&
                  SMJ_CR_FRAME == SMJ_CON_FRAME && SMJ_CR_FORCE == SMJ_CON_FORCE && SMJ_CR_GEOM1 == SMJ_CON_GEOM1 && SMJ_CR_GEOM2 == SMJ_CON_GEOM2 &&
                  SMJ_CR_DIM == SMJ_CON_CONDIM && SMJ_CR_EFC == SMJ_CON_EFC_ADR,
              "contact record: the kernel's word offsets (smj_model.h) and the header's (include/smj.h)");

struct smj_ctx {
  int device = 0;
  int num_envs = 0;
  DevModel model{};
  DevState state{};
  std::vector<void*> allocs;
  std::string err;
  float* qpos0_dev = nullptr;
  float* stage = nullptr;      // env-major staging copy of the state, [num_envs][layout.stride] (DevState::stage)
  int variant = 0;             // row of smj_variants (smj_variants.h)
  // capacity escalation: the model once more with the records of the variant's escalation target, and the list of parked envs
  DevModel model_esc{};
  bool has_esc = false;
  int* redo = nullptr;
  SmjStepOptions opt;      // the host-side scheduling options (smj_step_plan.h)
  // launch order: per-env shader time of the last launch and the permutation sorted by it (DevState::order / cost)
  int* cost = nullptr;
  int* order = nullptr;
  int lidar_cull = 1;      // lidar: drop, per env, the geoms that cannot reach the scan plane (smj_render.h lidar_plane_*)
  int mcl_stage_field = 1; // smj_scan_to_particles: the env's field is copied into LDS (0: gathered through L2; the weights must not change)
  bool prof_warned = false;    // the one-time warning of smj_step: profiling slot bound, the PGS kernel launched has no counters
  const SmjBuildDesc* last_primary = nullptr;   // the primary build of the last smj_step (smj_last_build)
  int* progress = nullptr;    // [B] progress, [B] done_steps, [SMJ_SCHED_WORDS] sched (DevState)
  size_t redo_cap = 0;         // entries the escalation list holds
  hipStream_t aux = nullptr;   // the pollers' stream
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  SmjCaps caps{};              // capacities of the variant in use
  SmjStageLayout layout{};     // staging-row layout of the variant in use
  int debug_floats = 0;
  DevRender render{};
  bool has_render = false;
  float* pose_ws = nullptr;
  // camera-static depth layers: geoms welded to a camera's body always look the same from that camera, so they are
  // rendered once per (camera, image size, field of view) and every later render starts its rays from that layer
  struct Layer { int cam = -1, w = 0, h = 0; float fovy = 0; float* buf = nullptr; };
  std::vector<Layer> layers;
  float* depth_ws = nullptr;   // scratch of the depth renderer's per-env staging pass (allocated at the first render)   // internal [nbody*12][num_envs] body poses when the caller has not bound SMJ_SLOT_XPOSE
  float* points_ws = nullptr;  // per-env transforms of smj_depth_to_points (allocated at the first call)
  void* slot_ptr[SMJ_SLOT_COUNT] = {};
  long slot_ld[SMJ_SLOT_COUNT] = {};
  // RCCL communicator of the env-sharded job (smj_comm_init); null in a single-GPU run
  SmjComm comm;
};

static_assert(sizeof(ncclUniqueId) == sizeof(SmjNcclId) && (int)ncclFloat == SMJ_NCCL_FLOAT32 && (int)ncclSuccess == SMJ_NCCL_SUCCESS && sizeof(ncclComm_t) == sizeof(void*),
              "smj_comm.h spells out RCCL's ABI by hand");

static int fail(smj_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

#define HIPCHK(c, call)                                                                     \
  do {                                                                                      \
    hipError_t e_ = (call);                                                                 \
    if (e_ != hipSuccess) return fail(c, -2, "%s failed: %s", #call, hipGetErrorString(e_)); \
  } while (0)

// the builds linked into this library, by SmjBuildId (each translation unit describes itself: smj_step_tu.h)
static const SmjBuildDesc* const smj_builds[SMJ_B_COUNT] = {
#define X(tag) &smj_build_##tag,
    SMJ_BUILDS(X)
#undef X
};

// device memory owned by the context (freed in smj_destroy), zeroed
template <class T>
static int alloc_zeroed(smj_ctx* c, size_t count, T** out) {
  void* d = nullptr;
  HIPCHK(c, hipMalloc(&d, sizeof(T) * count));
  c->allocs.push_back(d);
  HIPCHK(c, hipMemset(d, 0, sizeof(T) * count));
  *out = (T*)d;
  return 0;
}

// ---- argument checks shared by the render and perception entries.  Each returns 0 or what fail() returned; an entry is a list of
// them followed by a launch.  Order within an entry: -6 (the model has no tables) before every -1 (a bad argument) before -5 (a slot
// is not bound), and nothing is allocated or launched before the last check has passed.
#define TRY(call)             \
  do {                        \
    const int rc_ = (call);   \
    if (rc_) return rc_;      \
  } while (0)

static int check_render_tables(smj_ctx* c, const char* consequence) {
  return c->has_render ? 0 : fail(c, -6, "the model blob carries no render tables (k_rgeom / rmesh_*)%s", consequence);
}

static int check_camera_id(smj_ctx* c, int cam) {
  return cam >= 0 && cam < c->render.ncam ? 0 : fail(c, -1, "camera id %d out of range (ncam %d)", cam, c->render.ncam);
}

// `what` names the arguments: the render entries have no stride (they pass 1)
static int check_image(smj_ctx* c, int width, int height, int stride, float fovy_deg, const char* what) {
  return width >= 1 && height >= 1 && stride >= 1 && fovy_deg > 0.f && fovy_deg < 180.f ? 0 : fail(c, -1, "bad %s", what);
}

// a frame argument (include/smj_pointcloud.h): SMJ_FRAME_CAMERA where the entry has a camera, SMJ_FRAME_WORLD, or a body id.  The
// entries map the answer onto their kernels' own SMJ_PT_* / SMJ_OCC_* values.
enum FrameKind { FRAME_IS_CAMERA, FRAME_IS_WORLD, FRAME_IS_BODY };
static int check_frame(smj_ctx* c, int frame, bool camera_ok, FrameKind* kind) {
  if (frame < SMJ_FRAME_WORLD || (frame == SMJ_FRAME_CAMERA && !camera_ok))
    return fail(c, -1, "bad frame %d (%sSMJ_FRAME_WORLD or a body id)", frame, camera_ok ? "SMJ_FRAME_CAMERA, " : "");
  if (frame >= c->model.nbody_all) return fail(c, -1, "frame: body id %d out of range (nbody %d)", frame, c->model.nbody_all);
  *kind = frame == SMJ_FRAME_CAMERA ? FRAME_IS_CAMERA : frame == SMJ_FRAME_WORLD ? FRAME_IS_WORLD : FRAME_IS_BODY;
  return 0;
}

// the metric placement of a grid: the side of a cell, then the origin
static int check_origin_cell(smj_ctx* c, float x0, float y0, float cell) {
  if (!(cell > 0.f && cell <= 3.402823466e38f)) return fail(c, -1, "cell must be finite and > 0");
  if (!(fabsf(x0) <= 3.402823466e38f && fabsf(y0) <= 3.402823466e38f)) return fail(c, -1, "origin not finite");
  return 0;
}

static int check_grid(smj_ctx* c, int nx, int ny, int max_cells, float cell, float x0, float y0) {
  if (nx < 1 || ny < 1 || (long long)nx * ny > max_cells) return fail(c, -1, "bad grid %d x %d (nx, ny >= 1, nx * ny <= %d)", nx, ny, max_cells);
  return check_origin_cell(c, x0, y0, cell);
}

// a grid of integer cells (the distance and navigation entries: no cell size, no origin), within its kernel's limits
static int check_cell_grid(smj_ctx* c, int nx, int ny, int max_side, int max_cells) {
  return nx >= 1 && ny >= 1 && nx <= max_side && ny <= max_side && (long long)nx * ny <= max_cells
             ? 0 : fail(c, -1, "bad grid %d x %d (1 <= nx, ny <= %d, nx * ny <= %d)", nx, ny, max_side, max_cells);
}

// a kernel whose workgroups read an env's inputs while they (or others) store: no output may share a byte with an input or with
// another output (null pointers pass: an optional buffer left out)
struct ByteRange { const void* p; uintptr_t bytes; const char* name; };
static int check_disjoint(smj_ctx* c, std::initializer_list<ByteRange> inputs, std::initializer_list<ByteRange> outputs) {
  const auto meet = [](const ByteRange& a, const ByteRange& b) { return a.p && b.p && (uintptr_t)a.p < (uintptr_t)b.p + b.bytes && (uintptr_t)b.p < (uintptr_t)a.p + a.bytes; };
  for (const ByteRange& o : outputs)
    for (const ByteRange& i : inputs)
      if (meet(o, i)) return fail(c, -1, "the %s range overlaps the %s range", o.name, i.name);
  for (const ByteRange* o = outputs.begin(); o != outputs.end(); o++)
    for (const ByteRange* q = o + 1; q != outputs.end(); q++)
      if (meet(*o, *q)) return fail(c, -1, "the %s and %s ranges overlap", o->name, q->name);
  return 0;
}

// every buffer of an entry is read and written in 4-byte words (null pointers pass: whether one may be null is the entry's business)
static int check_aligned(smj_ctx* c, std::initializer_list<const void*> ptrs, const char* what) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  return bits & 3 ? fail(c, -1, "%s not aligned to 4 bytes", what) : 0;
}

static int check_xpose(smj_ctx* c) {
  return c->state.xpose ? 0 : fail(c, -5, "XPOSE slot is not bound (step with SMJ_READ_POSES first)");
}

// ---- the entries that read the lidar scan (smj_scan.h).  Each helper stands where its checks stood in every entry, so the order in
// which an entry's checks fire is the order of its lines.
// The model has a lidar (`what` ends the refusal: what the entry would have done with the scan) of at most max_rays rays.
static int check_scan(smj_ctx* c, int max_rays, const char* what) {
  if (!c->has_render || c->render.nlidar < 1) return fail(c, -6, "the model blob carries no lidar / ray-casting tables (sensor_lidar_site, k_lgeom): no scan to %s", what);
  return c->render.nlidar <= max_rays ? 0 : fail(c, -1, "the model has %d lidar rays, above %d", c->render.nlidar, max_rays);
}

static int check_lidar_ld(smj_ctx* c, long lidar_ld) {
  return lidar_ld >= c->num_envs ? 0 : fail(c, -1, "lidar_ld %ld below num_envs %d", lidar_ld, c->num_envs);
}

// `tail` ends the refusal of a ray longer than the line arithmetic of smj_occ.h takes
static int check_range_limits(smj_ctx* c, float r_min, float r_max, float cell, const char* tail) {
  if (!(r_min >= 0.f && r_min <= r_max && r_max <= 3.402823466e38f)) return fail(c, -1, "bad range limits (finite, 0 <= r_min <= r_max)");
  return r_max / cell <= (float)SMJ_OCC_MAX_STEPS ? 0 : fail(c, -1, "r_max / cell above %d%s", (int)SMJ_OCC_MAX_STEPS, tail);
}
static const char* const RAY_TOO_LONG = ": a ray would cross more cells than the line arithmetic takes";
static const char* const RAY_BOUND_OF_OCC = ", the bound of smj_lidar_to_occupancy";

// the frame of the entries that work in the robot's frame: a body id
static int check_robot_frame(smj_ctx* c, int frame) {
  FrameKind fk;
  if (frame < 0) return fail(c, -1, "bad frame %d (a body id: the robot's frame)", frame);
  return check_frame(c, frame, false, &fk);
}

// The bytes of the scan and of the XPOSE slot that a kernel reads, for check_disjoint.  Either ends with the last env of its last
// row: the columns beyond num_envs are the caller's, an output may live there.
static uintptr_t scan_extent(smj_ctx* c, long lidar_ld) {
  return ((uintptr_t)(c->render.nlidar - 1) * (uintptr_t)lidar_ld + (uintptr_t)c->num_envs) * 4u;
}
static uintptr_t xpose_extent(smj_ctx* c) {
  return ((12u * (uintptr_t)c->model.nbody_all - 1) * (uintptr_t)c->slot_ld[SMJ_SLOT_XPOSE] + (uintptr_t)c->num_envs) * 4u;
}

static SmjScanSource scan_source(smj_ctx* c, const void* lidar_dev, long lidar_ld) {
  return {c->state.xpose, c->slot_ld[SMJ_SLOT_XPOSE], c->render.lidar_site, c->render.site_bodyid, c->render.site_pos, c->render.site_mat,
          (const float*)lidar_dev, lidar_ld};
}

// device memory the context allocates at the first call that needs it and keeps (freed in smj_destroy)
template <class T>
static int ensure_alloc(smj_ctx* c, T** ptr, size_t bytes) {
  if (*ptr) return 0;
  void* d = nullptr;
  HIPCHK(c, hipMalloc(&d, bytes));
  c->allocs.push_back(d);
  *ptr = (T*)d;
  return 0;
}

struct DeviceUploader {
  smj_ctx* c;
  template <class T>
  const T* put(const std::vector<T>& h) {
    void* d = nullptr;
    if (hipMalloc(&d, h.size() * sizeof(T)) != hipSuccess) return nullptr;
    c->allocs.push_back(d);
    if (hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return static_cast<const T*>(d);
  }
  const float* f32(const std::vector<float>& h) { return put(h); }
  const int* i32(const std::vector<int>& h) { return put(h); }
};

// Depth-camera tables: visible-geom list, camera frames and one BVH per render mesh (built here, uploaded once).
static int setup_render(smj_ctx* c, const void* blob, size_t nbytes) {
  SmjBlob b{static_cast<const uint8_t*>(blob), nbytes};
  const SmjBlobEntry* rg = b.find("k_rgeom");
  const SmjBlobEntry* rv = b.find("rmesh_vert");
  const SmjBlobEntry* rf = b.find("rmesh_face");
  const SmjBlobEntry* va = b.find("rmesh_vertadr");
  const SmjBlobEntry* vn = b.find("rmesh_vertnum");
  const SmjBlobEntry* fa = b.find("rmesh_faceadr");
  const SmjBlobEntry* fn = b.find("rmesh_facenum");
  const SmjBlobEntry* gm = b.find("geom_rmeshid");
  const SmjBlobEntry* cb = b.find("cam_bodyid");
  const SmjBlobEntry* cp = b.find("cam_pos");
  const SmjBlobEntry* cm = b.find("k_cam_mat");
  const SmjBlobEntry* vz = b.find("vis_znear_zfar_extent");
  const SmjBlobEntry* nr = b.find("k_nrgeom");
  const SmjBlobEntry* lg = b.find("k_lgeom");
  const SmjBlobEntry* nl = b.find("k_nlgeom");
  const SmjBlobEntry* ls = b.find("sensor_lidar_site");
  const SmjBlobEntry* lt = b.find("sensor_lidar_static");
  if (!rg || !rv || !rf || !va || !vn || !fa || !fn || !gm || !cb || !cp || !cm || !vz || !nr || !lg || !nl || !ls || !lt)
    return 0;   // model without ray-casting tables: smj_render_depth / lidar readout report that
  if (rv->dtype != 3 || rf->dtype != 1 || vz->dtype != 0 || cp->dtype != 0 || cm->dtype != 0)
    return fail(c, -3, "model blob: render tables have unexpected types");
  DeviceUploader up{c};
  DevRender& r = c->render;
  int nrgeom = 0;
  memcpy(&nrgeom, b.p + nr->offset, 4);
  if (nrgeom > SMJ_RGEOM_MAX) return fail(c, -4, "model has %d camera-visible geoms, renderer capacity is %d", nrgeom, SMJ_RGEOM_MAX);
  r.nrgeom = nrgeom;
  r.ncam = (int)(cb->nbytes / 4);
  r.nbody = c->model.nbody_all;
  double z[3];
  memcpy(z, b.p + vz->offset, 24);
  r.znear = (float)(z[0] * z[2]);
  r.zfar = (float)(z[1] * z[2]);
  auto geti = [&](const SmjBlobEntry* e) { std::vector<int> h(e->nbytes / 4 ? e->nbytes / 4 : 1, 0); memcpy(h.data(), b.p + e->offset, e->nbytes); return h; };
  auto getd = [&](const SmjBlobEntry* e) {
    std::vector<float> h(e->nbytes / 8 ? e->nbytes / 8 : 1, 0.f);
    const double* src = reinterpret_cast<const double*>(b.p + e->offset);
    for (size_t i = 0; i < e->nbytes / 8; i++) h[i] = (float)src[i];
    return h;
  };
  r.rgeom = up.i32(geti(rg));
  r.geom_rmeshid = up.i32(geti(gm));
  r.cam_bodyid = up.i32(geti(cb));
  r.cam_pos = up.f32(getd(cp));
  r.cam_mat = up.f32(getd(cm));
  memcpy(&r.nlgeom, b.p + nl->offset, 4);
  r.nlidar = c->model.nlidar;
  r.lidar_cutoff = c->model.lidar_cutoff;
  if (r.nlidar > 384) return fail(c, -4, "model has %d lidar rays, kernel capacity is 384", r.nlidar);
  r.lgeom = up.i32(geti(lg));
  r.lidar_site = up.i32(geti(ls));
  r.lidar_static = up.f32(getd(lt));
  r.site_bodyid = c->model.site_bodyid; r.site_pos = c->model.site_pos; r.site_mat = c->model.k_site_mat;
  if (!r.lgeom || !r.lidar_site || !r.lidar_static) return fail(c, -2, "device allocation failed for the lidar tables");
  {   // the scan plane of the rangefinders (smj_render.h lidar_plane_*): all sites on one body, all rays within 1e-5 of one plane
    r.lidar_plane_body = -1;
    const SmjBlobEntry* sp = b.find("site_pos");
    const SmjBlobEntry* sm = b.find("k_site_mat");
    const SmjBlobEntry* sb = b.find("site_bodyid");
    if (sp && sm && sb && sp->dtype == 0 && sm->dtype == 0 && r.nlidar >= 3) {
      const std::vector<int> sites = geti(ls), sbody = geti(sb);
      const double* P = reinterpret_cast<const double*>(b.p + sp->offset);
      const double* Mx = reinterpret_cast<const double*>(b.p + sm->offset);
      auto dir = [&](int i, double* d) { const double* m9 = Mx + 9 * (size_t)sites[i]; d[0] = m9[2]; d[1] = m9[5]; d[2] = m9[8]; };
      double d0[3], n[3] = {0, 0, 0}, best = 0;
      dir(0, d0);
      for (int i = 1; i < r.nlidar; i++) {   // the normal from the pair of rays closest to a right angle
        double d[3];
        dir(i, d);
        const double cx = d0[1] * d[2] - d0[2] * d[1], cy = d0[2] * d[0] - d0[0] * d[2], cz = d0[0] * d[1] - d0[1] * d[0], l = sqrt(cx * cx + cy * cy + cz * cz);
        if (l > best) { best = l; n[0] = cx / l; n[1] = cy / l; n[2] = cz / l; }
      }
      bool ok = best > 0.5;
      double p0[3] = {0, 0, 0}, slack = 0, slope = 0;
      for (int i = 0; i < r.nlidar; i++) for (int k = 0; k < 3; k++) p0[k] += P[3 * (size_t)sites[i] + k] / r.nlidar;
      for (int i = 0; ok && i < r.nlidar; i++) {
        double d[3];
        dir(i, d);
        ok = sbody[sites[i]] == sbody[sites[0]];
        const double* q = P + 3 * (size_t)sites[i];
        slack = fmax(slack, fabs((q[0] - p0[0]) * n[0] + (q[1] - p0[1]) * n[1] + (q[2] - p0[2]) * n[2]));
        slope = fmax(slope, fabs(d[0] * n[0] + d[1] * n[1] + d[2] * n[2]));
      }
      if (ok && slope < 1e-5) {
        r.lidar_plane_body = sbody[sites[0]];
        for (int k = 0; k < 3; k++) { r.lidar_plane_p[k] = (float)p0[k]; r.lidar_plane_n[k] = (float)n[k]; }
        r.lidar_plane_slack = (float)slack + 1e-4f;          // + fp32 rounding of metre-scale coordinates
        r.lidar_plane_slope = (float)fmax(slope, 2e-6);       // per metre along the ray (fp32 directions)
      }
    }
  }
  r.geom_type = c->model.geom_type; r.geom_bodyid = c->model.geom_bodyid; r.geom_pos = c->model.geom_pos;
  r.geom_mat = c->model.k_geom_mat; r.geom_size = c->model.geom_size; r.geom_rbound = c->model.geom_rbound;
  r.geom_bcenter = c->model.k_geom_bcenter; r.geom_aabb = c->model.geom_aabb;
  {
    const SmjBlobEntry* gc = b.find("geom_rgba");   // colours of the RGB stand-in (smj_render_rgb); older blobs may lack them
    r.geom_rgba = (gc && gc->dtype == 0) ? up.f32(getd(gc)) : nullptr;
  }
  // BVHs
  const std::vector<int> vadr = geti(va), vnum = geti(vn), fadr = geti(fa), fnum = geti(fn);
  const float* verts = reinterpret_cast<const float*>(b.p + rv->offset);
  const int* faces = reinterpret_cast<const int*>(b.p + rf->offset);
  const size_t nmesh = va->nbytes / 4;
  SmjBvhSet set;
  for (size_t i = 0; i < nmesh; i++) {
    // faces index the vertices of their own mesh
    smj_bvh_add_mesh(set, verts + 3 * (size_t)vadr[i], vnum[i], faces + 3 * (size_t)fadr[i], fnum[i]);
  }
  std::vector<int> meshtab(4 * (nmesh ? nmesh : 1), 0);
  for (size_t i = 0; i < nmesh; i++) {
    meshtab[4 * i] = set.mesh[i].nodebase; meshtab[4 * i + 1] = set.mesh[i].tribase; meshtab[4 * i + 2] = set.mesh[i].leaf0;
    meshtab[4 * i + 3] = set.mesh[i].ntri;
  }
  if (set.node.empty()) set.node.assign(16, 0.f);
  if (set.tri.empty()) set.tri.assign(12, 0.f);
  r.node = reinterpret_cast<const float4*>(up.f32(set.node));
  r.tri = reinterpret_cast<const float4*>(up.f32(set.tri));
  r.mesh = reinterpret_cast<const int4*>(up.i32(meshtab));
  if (!r.rgeom || !r.geom_rmeshid || !r.cam_bodyid || !r.cam_pos || !r.cam_mat || !r.node || !r.tri || !r.mesh)
    return fail(c, -2, "device allocation failed for the render tables");
  {   // the mesh rasteriser's tables: meshlets of every render mesh and the work list over the mesh geoms a camera can see
    const SmjBlobEntry* gt = b.find("geom_type");
    std::vector<int> rgh = geti(rg), gmh = geti(gm), gth = gt ? geti(gt) : std::vector<int>();
    SmjMeshletSet ml;
    for (size_t i = 0; i < nmesh; i++) smj_meshlets_add_mesh(ml, verts + 3 * (size_t)vadr[i], faces + 3 * (size_t)fadr[i], set.order[i]);
    const SmjBlobEntry* gs = b.find("geom_size");
    std::vector<float> gsh = (gs && gs->dtype == 0) ? getd(gs) : std::vector<float>();
    std::vector<int> boxlet(nrgeom > 0 ? nrgeom : 1, -1);
    for (int i = 0; i < nrgeom && gt && !gsh.empty(); i++)   // box geoms: one meshlet each, appended after the meshes'
      if (gth[rgh[i]] == 6) boxlet[i] = smj_meshlets_add_box(ml, gsh.data() + 3 * (size_t)rgh[i]);
    std::vector<int> rec(12 * (ml.let.size() ? ml.let.size() : 1), 0), work;
    for (size_t i = 0; i < ml.let.size(); i++) {
      const SmjMeshlet& m = ml.let[i];
      int* q = rec.data() + 12 * i;
      q[0] = m.vbase; q[1] = m.nvert; q[2] = m.tbase; q[3] = m.ntri;
      const float f[8] = {m.cen[0], m.cen[1], m.cen[2], m.rad, m.axis[0], m.axis[1], m.axis[2], m.cosc};
      memcpy(q + 4, f, sizeof f);
    }
    for (int i = 0; i < nrgeom && gt; i++) {   // the work list: one (geom entry, meshlet) item per meshlet, mesh after mesh
      const int g = rgh[i];
      if (boxlet[i] >= 0) { work.push_back(i); work.push_back(boxlet[i]); continue; }
      if (gth[g] != 7 || gmh[g] < 0) continue;
      for (int k = 0; k < ml.mesh_count[gmh[g]]; k++) { work.push_back(i); work.push_back(ml.mesh_first[gmh[g]] + k); }
    }
    r.raster_boxes = gsh.empty() ? 0 : 1;
    r.nmlist = (int)(work.size() / 2);
    if (work.empty()) work.assign(2, 0);
    if (ml.vert.empty()) ml.vert.assign(4, 0.f);
    std::vector<int> tri(ml.tri.begin(), ml.tri.end());
    if (tri.empty()) tri.assign(1, 0);
    r.mlvert = reinterpret_cast<const float4*>(up.f32(ml.vert));
    r.mltri = reinterpret_cast<const unsigned*>(up.i32(tri));
    r.mlrec = reinterpret_cast<const int4*>(up.i32(rec));
    r.mlitem = reinterpret_cast<const int2*>(up.i32(work));
    if (!r.mlvert || !r.mltri || !r.mlrec || !r.mlitem) return fail(c, -2, "device allocation failed for the meshlet tables");
    r.raster = 1;
    r.raster_splits = 8;
  }
  c->has_render = true;
  return 0;
}

extern "C" {

const char* smj_version(void) { return "smj 0.1 (gfx950)"; }

const char* smj_last_error(const smj_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

const char* smj_last_build(const smj_ctx* ctx) { return ctx && ctx->last_primary ? ctx->last_primary->tag : ""; }   // include/smj_build.h

int smj_create(const void* blob, size_t nbytes, int num_envs, int device, smj_ctx** out) {
  if (!out) return -1;
  *out = nullptr;
  if (!blob || nbytes < 16 || memcmp(blob, "SMJB0001", 8) != 0) return -1;
  if (num_envs <= 0) return -1;
  smj_ctx* c = new smj_ctx();
  *out = c;  // returned even on failure so that smj_last_error() can be read; caller must smj_destroy()
  c->device = device;
  c->num_envs = num_envs;
  HIPCHK(c, hipSetDevice(device));
  hipDeviceProp_t prop;
  smj_step_options_for_arch(c->opt, hipGetDeviceProperties(&prop, device) == hipSuccess ? prop.gcnArchName : nullptr);
  DeviceUploader up{c};
  SmjCaps caps[SMJ_NVARIANTS];   // a variant's capacities are those of its Newton build
  for (int v = 0; v < SMJ_NVARIANTS; v++) caps[v] = smj_builds[smj_variants[v].newton]->caps;
  int rc = smj_load_model(blob, nbytes, c->model, up, c->err, caps, SMJ_NVARIANTS, &c->variant);
  if (rc) return rc;
  c->caps = caps[c->variant];
  c->layout = smj_stage_layout(c->caps.nvp, c->caps.nbp + c->caps.nsat, c->caps.nsat);
  const SmjVariant& V = smj_variants[c->variant];
  c->debug_floats = smj_builds[V.newton]->debug_floats;
  c->state.con_cap = c->caps.ncon;
  if (V.escalates()) {
    // escalation target: the same model loaded for the 160-row tall build (standard, 128-row tall) / the 64-column big build (38 / 50 columns) / the 32-satellite build
    int dummy = 0;
    const SmjCaps* esc_caps = V.esc_variant != SMJ_NO_VARIANT ? caps + V.esc_variant : &smj_builds[V.esc_build]->caps;
    rc = smj_load_model(blob, nbytes, c->model_esc, up, c->err, esc_caps, 1, &dummy);
    if (rc) return rc;
    c->has_esc = true;
    if (esc_caps->ncon > c->state.con_cap) c->state.con_cap = esc_caps->ncon;   // a handed-over step ends in the larger build
    void* d = nullptr;
    c->redo_cap = smj_redo_initial_cap(num_envs);   // longer calls re-allocate (smj_step)
    HIPCHK(c, hipMalloc(&d, sizeof(int) * c->redo_cap));
    c->redo = (int*)d;   // freed in smj_destroy (it can be re-allocated by smj_step)
    HIPCHK(c, hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
  }
  DevModel& m = c->model;
  c->qpos0_dev = const_cast<float*>(m.qpos0);
  c->state.B = num_envs;
  c->state.ld = num_envs;
  const size_t B = (size_t)num_envs;
  if ((rc = alloc_zeroed(c, 2 * B, &c->cost))) return rc;
  c->order = c->cost + num_envs;
  if ((rc = alloc_zeroed(c, 2 * B + SMJ_SCHED_WORDS + 1, &c->progress))) return rc;   // + the `hot` word behind sched, which the per-launch memset leaves alone
  if ((rc = alloc_zeroed(c, (size_t)c->layout.stride * B, &c->stage))) return rc;
  if ((rc = alloc_zeroed(c, 4 * SMJ_SEP_SLOTS * B, &c->state.sepcache))) return rc;           // separating directions of convex pairs, kept between steps
  if ((rc = alloc_zeroed(c, (size_t)SMJ_MC_SLOTS * SMJ_MC_WORDS * B, &c->state.mcache))) return rc;   // contact manifolds of convex pairs, kept between steps
  if ((rc = alloc_zeroed(c, SMJ_PGSPREV_STRIDE * B, &c->state.pgsprev))) return rc;           // PGS: the previous step's rows and forces, 2.6 KB per env
  return setup_render(c, blob, nbytes);
}

int smj_comm_init(smj_ctx* c, int rank, int world, const char* id_path, double timeout_s) {
  if (!c) return -1;
  HIPCHK(c, hipSetDevice(c->device));
  return smj_comm_open(c->comm, rank, world, id_path, timeout_s, c->err);   // binding, id-file rendezvous, ncclCommInitRank: smj_comm.h
}

int smj_allgather_returns(smj_ctx* c, const float* send_dev, float* recv_dev, int count, void* stream) {
  if (!c) return -1;
  if (!send_dev || !recv_dev || count <= 0) return fail(c, -1, "bad buffers / count");
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->comm.comm) {   // single-GPU job: the gather is a copy
    if (send_dev != recv_dev)
      HIPCHK(c, hipMemcpyAsync(recv_dev, send_dev, sizeof(float) * (size_t)count, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
  }
  return smj_comm_allgather(c->comm, send_dev, recv_dev, count, stream, c->err);
}

int smj_comm_destroy(smj_ctx* c) {
  if (!c) return -1;
  smj_comm_close(c->comm);
  return 0;
}

int smj_destroy(smj_ctx* c) {
  if (!c) return -1;
  smj_comm_destroy(c);
  if (c->aux) { (void)hipStreamSynchronize(c->aux); (void)hipStreamDestroy(c->aux); }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->redo) (void)hipFree(c->redo);
  for (void* p : c->allocs) (void)hipFree(p);
  delete c;
  return 0;
}

int smj_dims(const smj_ctx* c, int* out) {
  if (!c || !out) return -1;
  out[SMJ_DIM_NQ] = c->model.nq_all; out[SMJ_DIM_NV] = c->model.nv_all; out[SMJ_DIM_NU] = c->model.nu;
  out[SMJ_DIM_NSAT_MAX] = c->caps.nsat;
  out[SMJ_DIM_NBODY] = c->model.nbody_all; out[SMJ_DIM_NLIDAR] = c->model.nlidar; out[SMJ_DIM_NKEY] = c->model.nkey;
  out[SMJ_DIM_NUM_ENVS] = c->num_envs; out[SMJ_DIM_DEBUG_FLOATS] = c->debug_floats; out[SMJ_DIM_NEFC_MAX] = c->caps.nefc;
  out[SMJ_DIM_NCON_MAX] = c->caps.ncon; out[SMJ_DIM_NV_MAX] = c->caps.nvp; out[SMJ_DIM_NCAM] = c->has_render ? c->render.ncam : 0;
  out[SMJ_DIM_CONTACT_CAP] = c->state.con_cap;
  return 0;
}

int smj_bind(smj_ctx* c, int slot, void* p, long ld) {
  if (!c) return -1;
  if (slot < 0 || slot >= SMJ_SLOT_COUNT) return fail(c, -1, "bad slot %d", slot);
  if (p && ld < c->num_envs) return fail(c, -1, "slot %d: ld %ld < num_envs %d", slot, ld, c->num_envs);
  c->slot_ptr[slot] = p;
  c->slot_ld[slot] = ld;
  smj_bind_slot(c->state, slot, p);   // (false for SMJ_SLOT_CONTACTS alone: kept in slot_ptr until a call reads it)
  return 0;
}

static int check_bound(smj_ctx* c) {
  static const int need[] = {SMJ_SLOT_QPOS, SMJ_SLOT_QVEL, SMJ_SLOT_CTRL, SMJ_SLOT_WARMSTART, SMJ_SLOT_NSTEP,
                             SMJ_SLOT_ACT_LENGTH, SMJ_SLOT_ACT_VELOCITY, SMJ_SLOT_BASE_POSE, SMJ_SLOT_INFO};
  long ld = -1;
  for (int s : need) {
    if (!c->slot_ptr[s]) return fail(c, -5, "slot %d is not bound", s);
    if (s == SMJ_SLOT_NSTEP) continue;
    if (ld < 0) ld = c->slot_ld[s];
    if (c->slot_ld[s] != ld) return fail(c, -5, "all batch-major slots must share one leading dimension");
  }
  for (int s : {SMJ_SLOT_GYRO, SMJ_SLOT_ACCEL, SMJ_SLOT_LIDAR, SMJ_SLOT_DEBUG, SMJ_SLOT_PROF, SMJ_SLOT_XPOSE, SMJ_SLOT_BASECTL})
    if (c->slot_ptr[s] && c->slot_ld[s] != ld) return fail(c, -5, "slot %d: leading dimension differs", s);
  c->state.ld = ld;
  return 0;
}

int smj_reset(smj_ctx* c, const uint8_t* mask_dev, void* stream) {
  if (!c) return -1;
  int rc = check_bound(c);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  smj_launch_reset(c->model, c->state, mask_dev, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int smj_step(smj_ctx* c, int nsteps, unsigned read_flags, void* stream) {
  if (!c) return -1;
  if (nsteps <= 0) return fail(c, -1, "nsteps must be positive");
  int rc = check_bound(c);
  if (rc) return rc;
  if ((read_flags & SMJ_READ_IMU) && (!c->state.gyro || !c->state.accel)) return fail(c, -5, "IMU readout requested but GYRO/ACCEL not bound");
  if ((read_flags & SMJ_READ_LIDAR) && !c->state.lidar) return fail(c, -5, "lidar readout requested but LIDAR not bound");
  if ((read_flags & SMJ_READ_POSES) && !c->state.xpose) return fail(c, -5, "pose readout requested but XPOSE not bound");
  if ((read_flags & SMJ_READ_CONTACTS) && !c->slot_ptr[SMJ_SLOT_CONTACTS]) return fail(c, -5, "contact readout requested but CONTACTS not bound");
  HIPCHK(c, hipSetDevice(c->device));
  DevState st = c->state;
  st.contacts = (read_flags & SMJ_READ_CONTACTS) ? (float*)c->slot_ptr[SMJ_SLOT_CONTACTS] : nullptr;
  long pose_ld = c->slot_ld[SMJ_SLOT_XPOSE];
  if (read_flags & SMJ_READ_LIDAR) {
    // the lidar is ray-cast by its own kernel from the body poses of the last step
    if (!c->has_render) return fail(c, -6, "the model blob carries no ray-casting tables (k_lgeom / rmesh_*): no lidar");
    if (!st.xpose) {
      if (!c->pose_ws) {
        void* d = nullptr;
        HIPCHK(c, hipMalloc(&d, sizeof(float) * 12 * (size_t)c->model.nbody_all * (size_t)c->num_envs));
        c->allocs.push_back(d);
        c->pose_ws = (float*)d;
      }
      st.xpose = c->pose_ws;
      pose_ld = c->num_envs;
      // the step kernel indexes every batch-major array with one leading dimension
      if (st.ld != pose_ld) return fail(c, -5, "bind SMJ_SLOT_XPOSE when the leading dimension differs from num_envs");
    }
    read_flags |= SMJ_READ_POSES;
  }
  // batch-major slots -> env-major staging rows, the step kernel on contiguous rows, and back (smj_model.h, DevState::stage)
  const DevModel& m = c->model;
  StagePlan in, out;
  const SmjStageLayout& Y = c->layout;
  in.add(st.qpos, m.nq_all, Y.qpos); in.add(st.qvel, m.nv_all, Y.qvel); in.add(st.warm, m.nv_all, Y.warm);
  in.add(st.ctrl, m.nu, Y.ctrl); in.add(st.bctl, SMJ_BC_ROWS, Y.bctl); in.add(st.nstep, 1, Y.nstep);
  in.add(st.info, 4, Y.info);
  out = in;
  out.add(st.act_len, m.nu, Y.actlen); out.add(st.act_vel, m.nu, Y.actvel); out.add(st.base, 3, Y.base);
  if (read_flags & SMJ_READ_IMU) { out.add(st.gyro, 3, Y.gyro); out.add(st.accel, 3, Y.accel); }
  if (read_flags & SMJ_READ_POSES) out.add(st.xpose, 12 * m.nbody_all, Y.xpose);
  st.stage = c->stage;
  st.lay = Y;
  st.cost = c->cost;
  // what the call is, which builds it launches (the escalation model runs with the primary's options: one routing for both; the lean
  // twin of the standard Newton build in its place when this call can execute none of what that twin leaves out) and how every one of
  // them is launched (smj_step_plan.h).  The rest of this function carries the plan out: each `if` below tests one of its fields.
  const SmjVariant& V = smj_variants[c->variant];
  const SmjCallFacts facts{c->num_envs, nsteps, st.debug != nullptr, st.prof != nullptr, c->has_esc};
  const SmjRoute route = smj_route_lean(smj_route(c->variant, c->model.solver, facts.prof_bound, c->opt.newton_two_waves, c->opt.pgs_two_waves, smj_builds),
                                        smj_lean_facts(c->model, st, c->opt.lean_build), smj_builds[SMJ_B_step], smj_lean_pick(c->opt.lean_build, &smj_build_lean, &smj_build_lean2));
  const SmjStepPlan plan = smj_plan_step(V, route, c->opt, facts);
  c->last_primary = route.primary;
  if (plan.esc) {   // the escalation target runs with the same options
#define X(name, field, type) c->model_esc.field = c->model.field;
    SMJ_SOLVER_OPTIONS(X)
#undef X
  }
  hipStream_t sm = (hipStream_t)stream;
  smj_launch_stage(in, c->stage, Y.stride, c->num_envs, st.ld, false, sm);
  st.progress = st.done_steps = st.sched = st.hot = nullptr;
  if (plan.clear_sched) {
    st.progress = c->progress;
    st.done_steps = c->progress + c->num_envs;
    st.sched = c->progress + 2 * (size_t)c->num_envs;
    st.hot = st.sched + SMJ_SCHED_WORDS;
    HIPCHK(c, hipMemsetAsync(c->progress, 0, sizeof(int) * (2 * (size_t)c->num_envs + SMJ_SCHED_WORDS), sm));
  }
  if ((size_t)plan.redo_need > c->redo_cap) {   // the list grows, never shrinks
    HIPCHK(c, hipDeviceSynchronize());
    (void)hipFree(c->redo);
    c->redo = nullptr;
    c->redo_cap = (size_t)plan.redo_need;
    void* d = nullptr;
    HIPCHK(c, hipMalloc(&d, sizeof(int) * c->redo_cap));
    c->redo = (int*)d;
  }
  // -1 = entry not published yet: only the pollers read entries while the list grows (the sweep runs after the kernel, the count is final)
  if (plan.mark_unpublished) HIPCHK(c, hipMemsetAsync(c->redo, 0xff, sizeof(int) * (size_t)plan.pipe_total, sm));
  st.redo = plan.esc ? c->redo : nullptr;
  st.redo_worker = 0;
  st.pipe_len = plan.pipe_len;
  st.pipe_total = plan.pipe_total;
  st.pollers = 0;
  st.order = nullptr;
  if (plan.ordered) {
    smj_launch_order(c->cost, c->order, c->num_envs, sm);
    st.order = c->order;
  }
  int lrc = 0;
  if (plan.poll) {
    // pollers first, on their own stream, so that they are resident when the standard kernel fills the device; should they
    // not be (nothing guarantees it), parked envs are given up to the sweep, as without pollers
    DevState sp = st;
    sp.redo_worker = 2;
    sp.pollers = plan.poller_arg;
    sp.order = nullptr;
    HIPCHK(c, hipEventRecord(c->ev_fork, sm));
    HIPCHK(c, hipStreamWaitEvent(c->aux, c->ev_fork, 0));
    lrc = route.poller->launch(c->model_esc, sp, nsteps, read_flags, plan.poller_wgs, c->aux);
    HIPCHK(c, hipEventRecord(c->ev_join, c->aux));
  }
  // The primary builds exist once per solver (smj_step_impl.h newton()); smj_route has picked the one that carries this call's
  // solver by what the builds say of themselves -- a launcher's refusal (its own guard) is an error here, not a question.
  if (!lrc) lrc = route.primary->launch(c->model, st, nsteps, read_flags, 0, sm);
  if (lrc == SMJ_LAUNCH_REFUSED_SOLVER) return fail(c, -2, "build `%s` does not carry solver %d (variant %s)", route.primary->tag, c->model.solver, V.name);
  if (route.no_counters && !c->prof_warned) {   // (once: the caller asked for stage cycles and gets zeros -- say so instead of returning them silently)
    c->prof_warned = true;
    fprintf(stderr, "libsmj: the profiling slot is bound but the PGS kernel of this build has no cycle counters (build `make bigprof` and load it through SMJ_LIB_PATH); the counters stay zero\n");
  }
  if (plan.poll) HIPCHK(c, hipStreamWaitEvent(sm, c->ev_join, 0));
  if (!lrc && plan.sweep) {
    // the sweep: whatever is left of the envs that ran out of constraint rows / contact slots (parked at the start of the
    // offending step) is finished by the tall variant (160 rows / 48 contacts); an empty list returns at once
    st.redo_worker = 1;
    st.pipe_len = 0;
    lrc = route.sweep->launch(c->model_esc, st, nsteps, read_flags, plan.sweep_wgs, sm);
  }
  if (lrc) return fail(c, -2, "step kernel launch failed: %s", hipGetErrorString((hipError_t)lrc));
  smj_launch_stage(out, c->stage, Y.stride, c->num_envs, st.ld, true, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  if (read_flags & SMJ_READ_LIDAR) {
    DevRender rl = c->render;
    if (!c->lidar_cull) rl.lidar_plane_body = -1;   // option "lidar_cull" = 0: every run-time geom staged for every env (the ranges must not change)
    smj_launch_lidar(rl, st.xpose, pose_ld, c->num_envs, st.lidar, st.ld, (hipStream_t)stream);
    HIPCHK(c, hipGetLastError());
  }
  return 0;
}

int smj_base_controller_tick(smj_ctx* c, void* stream) {
  if (!c) return -1;
  int rc = check_bound(c);
  if (rc) return rc;
  if (!c->state.bctl) return fail(c, -5, "BASECTL slot is not bound");
  HIPCHK(c, hipSetDevice(c->device));
  smj_launch_base_tick(c->state, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int smj_render_depth(smj_ctx* c, int cam, int width, int height, float fovy_deg, float max_depth, void* out_dev, void* stream) {
  if (!c) return -1;
  TRY(check_render_tables(c, ""));
  TRY(check_camera_id(c, cam));
  TRY(check_image(c, width, height, 1, fovy_deg, "image size / field of view"));
  if (!out_dev) return fail(c, -1, "null output image");
  TRY(check_xpose(c));
  HIPCHK(c, hipSetDevice(c->device));
  TRY(ensure_alloc(c, &c->depth_ws, smj_depth_workspace_bytes(c->num_envs)));
  smj_ctx::Layer* L = nullptr;
  for (auto& l : c->layers)
    if (l.cam == cam && l.w == width && l.h == height && l.fovy == fovy_deg) L = &l;
  if (!L) {
    smj_ctx::Layer l;
    l.cam = cam; l.w = width; l.h = height; l.fovy = fovy_deg;
    TRY(ensure_alloc(c, &l.buf, sizeof(float) * (size_t)width * (size_t)height));
    smj_launch_depth(c->render, c->state.xpose, c->slot_ld[SMJ_SLOT_XPOSE], c->num_envs, cam, width, height, fovy_deg, 0.f, l.buf,
                     nullptr, 1, c->depth_ws, (hipStream_t)stream);
    HIPCHK(c, hipGetLastError());
    c->layers.push_back(l);
    L = &c->layers.back();
  }
  smj_launch_depth(c->render, c->state.xpose, c->slot_ld[SMJ_SLOT_XPOSE], c->num_envs, cam, width, height, fovy_deg, max_depth,
                   (float*)out_dev, L->buf, 2, c->depth_ws, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int smj_render_rgb(smj_ctx* c, int cam, int width, int height, float fovy_deg, void* rgb_dev, void* gid_dev, void* stream) {
  if (!c) return -1;
  TRY(check_render_tables(c, ""));
  if (!c->render.geom_rgba) return fail(c, -6, "the model blob carries no geom colours (geom_rgba)");
  TRY(check_camera_id(c, cam));
  TRY(check_image(c, width, height, 1, fovy_deg, "image size / field of view"));
  if (!rgb_dev) return fail(c, -1, "null output image");
  TRY(check_xpose(c));
  HIPCHK(c, hipSetDevice(c->device));
  TRY(ensure_alloc(c, &c->depth_ws, smj_depth_workspace_bytes(c->num_envs)));
  smj_launch_rgb(c->render, c->state.xpose, c->slot_ld[SMJ_SLOT_XPOSE], c->num_envs, cam, width, height, fovy_deg,
                 (unsigned char*)rgb_dev, (int*)gid_dev, c->depth_ws, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int smj_depth_to_points(smj_ctx* c, int cam, int width, int height, float fovy_deg, const void* depth_dev, int stride, int frame,
                        void* points_dev, void* stream) {
  if (!c) return -1;
  FrameKind fk;
  TRY(check_render_tables(c, ": no cameras"));
  TRY(check_camera_id(c, cam));
  TRY(check_image(c, width, height, stride, fovy_deg, "image size / stride / field of view"));
  if (!depth_dev || !points_dev) return fail(c, -1, "null depth image / point buffer");
  TRY(check_aligned(c, {depth_dev, points_dev}, "depth image / point buffer"));
  TRY(check_frame(c, frame, true, &fk));
  const long long per_env = (long long)smj_points_grid(width, stride) * smj_points_grid(height, stride);
  if (per_env > 0x7fffffffLL || per_env * c->num_envs > 0x7fffffffLL * 1024) return fail(c, -1, "point grid too large");
  if (fk != FRAME_IS_CAMERA) TRY(check_xpose(c));
  HIPCHK(c, hipSetDevice(c->device));
  TRY(ensure_alloc(c, &c->points_ws, smj_points_workspace_bytes(c->num_envs)));
  const int kind = fk == FRAME_IS_CAMERA ? SMJ_PT_CAMERA : fk == FRAME_IS_WORLD ? SMJ_PT_WORLD : SMJ_PT_BODY;
  smj_launch_points(c->state.xpose, c->slot_ld[SMJ_SLOT_XPOSE], c->num_envs, c->render.cam_bodyid, c->render.cam_pos, c->render.cam_mat, cam,
                    width, height, fovy_deg, (const float*)depth_dev, stride, kind, kind == SMJ_PT_BODY ? frame : 0, (float*)points_dev,
                    c->points_ws, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int smj_depth_to_heightmap(smj_ctx* c, int cam, int width, int height, float fovy_deg, const void* depth_dev, int stride, int frame,
                           float x0, float y0, float cell, int nx, int ny, float z_lo, float z_hi, int accumulate, void* zmax_dev,
                           void* count_dev, void* stream) {
  if (!c) return -1;
  FrameKind fk;
  TRY(check_render_tables(c, ": no cameras"));
  TRY(check_camera_id(c, cam));
  TRY(check_image(c, width, height, stride, fovy_deg, "image size / stride / field of view"));
  if ((long long)width * height > 0x7fffffffLL) return fail(c, -1, "image too large");
  TRY(check_grid(c, nx, ny, SMJ_HMAP_MAX_CELLS, cell, x0, y0));
  if (!(z_lo <= z_hi)) return fail(c, -1, "bad height band (NaN, or z_lo > z_hi)");
  if (!depth_dev || !zmax_dev) return fail(c, -1, "null depth image / height buffer");
  TRY(check_aligned(c, {depth_dev, zmax_dev, count_dev}, "depth image / height / count buffer"));
  TRY(check_frame(c, frame, true, &fk));
  if (fk != FRAME_IS_CAMERA) TRY(check_xpose(c));
  HIPCHK(c, hipSetDevice(c->device));
  const int kind = fk == FRAME_IS_CAMERA ? SMJ_PT_CAMERA : fk == FRAME_IS_WORLD ? SMJ_PT_WORLD : SMJ_PT_BODY;
  smj_launch_hmap(c->state.xpose, c->slot_ld[SMJ_SLOT_XPOSE], c->num_envs, c->render.cam_bodyid, c->render.cam_pos, c->render.cam_mat, cam, width,
                  height, fovy_deg, (const float*)depth_dev, stride, kind, kind == SMJ_PT_BODY ? frame : 0, x0, y0, cell, nx, ny, z_lo, z_hi,
                  accumulate != 0, (float*)zmax_dev, (int*)count_dev, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int smj_lidar_to_occupancy(smj_ctx* c, const void* lidar_dev, long lidar_ld, int frame, float x0, float y0, float cell, int nx, int ny,
                           float r_min, float r_max, int no_return_clears, int accumulate, void* hit_dev, void* miss_dev, void* stream) {
  if (!c) return -1;
  FrameKind fk;
  TRY(check_scan(c, 384, "map"));   // (the capacity of the ray cast: smj_create has refused a model with more)
  if (!lidar_dev || !hit_dev) return fail(c, -1, "null scan / hit buffer");
  TRY(check_aligned(c, {lidar_dev, hit_dev, miss_dev}, "scan / hit / miss buffer"));
  TRY(check_lidar_ld(c, lidar_ld));
  TRY(check_grid(c, nx, ny, SMJ_OCC_MAX_CELLS, cell, x0, y0));
  TRY(check_range_limits(c, r_min, r_max, cell, RAY_TOO_LONG));
  TRY(check_frame(c, frame, false, &fk));
  TRY(check_xpose(c));
  HIPCHK(c, hipSetDevice(c->device));
  const int kind = fk == FRAME_IS_WORLD ? SMJ_OCC_WORLD : SMJ_OCC_BODY;
  smj_launch_occ(scan_source(c, lidar_dev, lidar_ld), c->num_envs, c->render.nlidar, kind, kind == SMJ_OCC_BODY ? frame : 0, x0, y0, cell, nx, ny, r_min,
                 r_max, no_return_clears != 0, accumulate != 0, (int*)hit_dev, (int*)miss_dev, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int smj_occupancy_to_distance(smj_ctx* c, const void* hit_dev, const void* miss_dev, int nx, int ny, int min_hits, int unknown_is_obstacle,
                              int max_dist_cells, void* dist2_dev, void* nearest_dev, void* stream) {
  if (!c) return -1;
  if (!hit_dev || !dist2_dev) return fail(c, -1, "null hit / dist2 buffer");
  TRY(check_aligned(c, {hit_dev, miss_dev, dist2_dev, nearest_dev}, "hit / miss / dist2 / nearest buffer"));
  TRY(check_cell_grid(c, nx, ny, SMJ_EDT_MAX_SIDE, SMJ_EDT_MAX_CELLS));
  if (min_hits < 1) return fail(c, -1, "min_hits %d below 1: every cell would be an obstacle", min_hits);
  if (max_dist_cells < 0) return fail(c, -1, "max_dist_cells %d is negative (0 = no bound)", max_dist_cells);
  if (unknown_is_obstacle && !miss_dev) return fail(c, -1, "unknown_is_obstacle needs the miss layer");
  // several workgroups of an env read the grid while others store
  const uintptr_t bytes = (uintptr_t)c->num_envs * (uintptr_t)nx * (uintptr_t)ny * 4u;
  TRY(check_disjoint(c, {{hit_dev, bytes, "hit"}, {miss_dev, bytes, "miss"}}, {{dist2_dev, bytes, "dist2"}, {nearest_dev, bytes, "nearest"}}));
  HIPCHK(c, hipSetDevice(c->device));
  // no cell pair is further apart than sqrt(2) 4095 cells: a larger bound is no bound (and R * R stays an int)
  const int R = max_dist_cells >= 2 * SMJ_EDT_MAX_SIDE ? 0 : max_dist_cells;
  smj_launch_edt(c->num_envs, (const int*)hit_dev, (const int*)miss_dev, nx, ny, min_hits, unknown_is_obstacle != 0, R, (int*)dist2_dev,
                 (int*)nearest_dev, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int smj_costmap_to_navigation(smj_ctx* c, const void* cost_dev, const void* goal_dev, int num_goals, int nx, int ny, int lethal, int neutral,
                              void* potential_dev, void* next_dev, void* stream) {
  if (!c) return -1;
  if (!goal_dev || !potential_dev) return fail(c, -1, "null goal / potential buffer");
  TRY(check_aligned(c, {goal_dev, potential_dev, next_dev}, "goal / potential / next buffer"));
  TRY(check_cell_grid(c, nx, ny, SMJ_NAV_MAX_SIDE, SMJ_NAV_MAX_CELLS));
  if (num_goals < 1 || num_goals > SMJ_NAV_MAX_GOALS) return fail(c, -1, "num_goals %d outside [1, %d]", num_goals, (int)SMJ_NAV_MAX_GOALS);
  if (lethal < 1 || lethal > 256) return fail(c, -1, "lethal %d outside [1, 256]: below 1 no cell is passable, above 256 means 256", lethal);
  if (neutral < 1 || neutral > 255) return fail(c, -1, "neutral %d outside [1, 255]: a free step must cost something, and the potential must stay below 2^30", neutral);
  // the workgroup of an env reads its inputs while it stores (the potential of a large grid is relaxed in place)
  const uintptr_t cells = (uintptr_t)c->num_envs * (uintptr_t)nx * (uintptr_t)ny;
  TRY(check_disjoint(c, {{cost_dev, cells, "cost"}, {goal_dev, (uintptr_t)c->num_envs * (uintptr_t)num_goals * 4u, "goal"}},
                     {{potential_dev, cells * 4u, "potential"}, {next_dev, cells * 4u, "next"}}));
  HIPCHK(c, hipSetDevice(c->device));
  smj_launch_nav(c->num_envs, (const uint8_t*)cost_dev, (const int*)goal_dev, num_goals, nx, ny, lethal, neutral, (int*)potential_dev,
                 (int*)next_dev, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int smj_occupancy_to_frontiers(smj_ctx* c, const void* hit_dev, const void* miss_dev, const void* cost_dev, int nx, int ny, int min_hits, int lethal,
                               int min_size, int max_regions, void* label_dev, void* goal_dev, void* region_dev, void* count_dev, void* stream) {
  if (!c) return -1;
  if (!hit_dev || !miss_dev || !label_dev || !goal_dev) return fail(c, -1, "null hit / miss / label / goal buffer");
  TRY(check_aligned(c, {hit_dev, miss_dev, label_dev, goal_dev, region_dev, count_dev}, "hit / miss / label / goal / region / count buffer"));
  TRY(check_cell_grid(c, nx, ny, SMJ_FRONT_MAX_SIDE, SMJ_FRONT_MAX_CELLS));
  if (min_hits < 1) return fail(c, -1, "min_hits %d below 1: every cell would be occupied", min_hits);
  if (lethal < 1 || lethal > 256) return fail(c, -1, "lethal %d outside [1, 256]: below 1 no cell is passable, above 256 means 256", lethal);
  if (min_size < 1) return fail(c, -1, "min_size %d below 1: a region has at least one cell", min_size);
  if (max_regions < 1 || max_regions > SMJ_FRONT_MAX_REGIONS) return fail(c, -1, "max_regions %d outside [1, %d]", max_regions, (int)SMJ_FRONT_MAX_REGIONS);
  // the workgroup of an env reads its inputs while it stores (the labels of a large grid are built in place)
  const uintptr_t cells = (uintptr_t)c->num_envs * (uintptr_t)nx * (uintptr_t)ny, rows = (uintptr_t)c->num_envs * (uintptr_t)max_regions;
  TRY(check_disjoint(c, {{hit_dev, cells * 4u, "hit"}, {miss_dev, cells * 4u, "miss"}, {cost_dev, cells, "cost"}},
                     {{label_dev, cells * 4u, "label"}, {goal_dev, rows * 4u, "goal"}, {region_dev, rows * 16u, "region"},
                      {count_dev, (uintptr_t)c->num_envs * 8u, "count"}}));
  HIPCHK(c, hipSetDevice(c->device));
  smj_launch_front(c->num_envs, (const int*)hit_dev, (const int*)miss_dev, (const uint8_t*)cost_dev, nx, ny, min_hits, lethal, min_size, max_regions,
                   (int*)label_dev, (int*)goal_dev, (int*)region_dev, (int*)count_dev, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return 0;
}

static_assert((int)SMJ_DRIVE_NAV_NONE == SMJ_NAV_NONE && (int)SMJ_DRIVE_MAX_CELLS == (int)SMJ_NAV_MAX_CELLS && (int)SMJ_DRIVE_MAX_SIDE == (int)SMJ_NAV_MAX_SIDE,
              "smj_drive.h reads the potential of smj_costmap_to_navigation");

int smj_navigation_to_velocity(smj_ctx* c, const void* pose_dev, const void* twist_dev, const void* cost_dev, const void* potential_dev, int nx, int ny,
                               float x0, float y0, float cell, const void* command_dev, const void* point_dev, const void* bias_dev, int num_candidates,
                               int num_points, int lethal, int outside_is_free, int goal_weight, int obstacle_weight, int arrive_potential, float max_dv,
                               float max_dw, void* cmd_dev, void* best_dev, void* score_dev, void* cell_dev, void* stream) {
  if (!c) return -1;
  if (!pose_dev || !potential_dev || !command_dev || !point_dev || !cmd_dev || !best_dev)
    return fail(c, -1, "null pose / potential / command / point / cmd / best buffer");
  TRY(check_aligned(c, {pose_dev, twist_dev, potential_dev, command_dev, point_dev, bias_dev, cmd_dev, best_dev, score_dev, cell_dev},
                    "pose / twist / potential / command / point / bias / cmd / best / score / cell buffer"));
  if ((uintptr_t)score_dev & 7) return fail(c, -1, "score buffer not aligned to 8 bytes");
  TRY(check_cell_grid(c, nx, ny, SMJ_DRIVE_MAX_SIDE, SMJ_DRIVE_MAX_CELLS));
  TRY(check_origin_cell(c, x0, y0, cell));
  if (num_candidates < 1 || num_candidates > SMJ_DRIVE_MAX_CANDIDATES || num_points < 1 || num_points > SMJ_DRIVE_MAX_POINTS ||
      num_candidates * num_points > SMJ_DRIVE_MAX_TABLE)
    return fail(c, -1, "bad table %d x %d (1 <= num_candidates <= %d, 1 <= num_points <= %d, their product <= %d)", num_candidates, num_points,
                (int)SMJ_DRIVE_MAX_CANDIDATES, (int)SMJ_DRIVE_MAX_POINTS, (int)SMJ_DRIVE_MAX_TABLE);
  if (lethal < 1 || lethal > 256) return fail(c, -1, "lethal %d outside [1, 256]: below 1 every cell blocks, above 256 means 256", lethal);
  if (goal_weight < 0 || goal_weight > SMJ_DRIVE_MAX_WEIGHT || obstacle_weight < 0 || obstacle_weight > SMJ_DRIVE_MAX_WEIGHT)
    return fail(c, -1, "goal_weight %d or obstacle_weight %d outside [0, %d]", goal_weight, obstacle_weight, (int)SMJ_DRIVE_MAX_WEIGHT);
  if (arrive_potential < 0 || arrive_potential >= SMJ_NAV_NONE) return fail(c, -1, "arrive_potential %d outside [0, SMJ_NAV_NONE)", arrive_potential);
  if (!(max_dv >= 0.f && max_dw >= 0.f)) return fail(c, -1, "max_dv and max_dw must be >= 0 (+inf: no limit)");
  const uintptr_t envs = (uintptr_t)c->num_envs, cells = envs * (uintptr_t)nx * (uintptr_t)ny, K = (uintptr_t)num_candidates, P = (uintptr_t)num_points;
  TRY(check_disjoint(c, {{pose_dev, envs * 12u, "pose"}, {twist_dev, envs * 8u, "twist"}, {cost_dev, cells, "cost"}, {potential_dev, cells * 4u, "potential"},
                         {command_dev, K * 8u, "command"}, {point_dev, K * P * 8u, "point"}, {bias_dev, K * 4u, "bias"}},
                     {{cmd_dev, envs * 8u, "cmd"}, {best_dev, envs * 8u, "best"}, {score_dev, envs * K * 8u, "score"}, {cell_dev, envs * K * P * 4u, "cell"}}));
  HIPCHK(c, hipSetDevice(c->device));
  smj_launch_drive(c->num_envs, (const float*)pose_dev, (const float*)twist_dev, (const uint8_t*)cost_dev, (const int*)potential_dev, nx, ny, x0, y0, cell,
                   (const float*)command_dev, (const float*)point_dev, (const int*)bias_dev, num_candidates, num_points, lethal, outside_is_free != 0,
                   goal_weight, obstacle_weight, arrive_potential, max_dv, max_dw, (float*)cmd_dev, (int*)best_dev, (long long*)score_dev, (int*)cell_dev,
                   (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return 0;
}

static_assert((int)SMJ_MATCH_MAX_CELLS == (int)SMJ_OCC_MAX_CELLS && (int)SMJ_MATCH_MAX_CELLS == (int)SMJ_EDT_MAX_CELLS && (int)SMJ_MATCH_MAX_SIDE == (int)SMJ_EDT_MAX_SIDE,
              "smj_match.h matches scans against the maps of smj_lidar_to_occupancy and smj_occupancy_to_distance");

int smj_scan_to_pose(smj_ctx* c, const void* lidar_dev, long lidar_ld, int frame, float r_min, float r_max, const void* field_dev, int nx, int ny, float x0,
                     float y0, float cell, const void* pose_dev, const void* angle_dev, const void* angle_bias_dev, int num_angles, int wx, int wy,
                     int shift_weight, int min_points, void* pose_out_dev, void* best_dev, void* score_dev, void* cell_dev, void* stream) {
  if (!c) return -1;
  TRY(check_scan(c, SMJ_MATCH_MAX_POINTS, "match"));
  if (!lidar_dev || !field_dev || !pose_dev || !angle_dev || !pose_out_dev || !best_dev)
    return fail(c, -1, "null scan / field / pose / angle / pose_out / best buffer");
  TRY(check_aligned(c, {lidar_dev, pose_dev, angle_dev, angle_bias_dev, pose_out_dev, best_dev, score_dev, cell_dev},
                    "scan / pose / angle / angle_bias / pose_out / best / score / cell buffer"));
  const int nlidar = c->render.nlidar;
  TRY(check_lidar_ld(c, lidar_ld));
  TRY(check_cell_grid(c, nx, ny, SMJ_MATCH_MAX_SIDE, SMJ_MATCH_MAX_CELLS));
  TRY(check_origin_cell(c, x0, y0, cell));
  TRY(check_range_limits(c, r_min, r_max, cell, RAY_BOUND_OF_OCC));
  TRY(check_robot_frame(c, frame));
  if (num_angles < 1 || num_angles > SMJ_MATCH_MAX_ANGLES) return fail(c, -1, "num_angles %d outside [1, %d]", num_angles, (int)SMJ_MATCH_MAX_ANGLES);
  if (wx < 0 || wx > SMJ_MATCH_MAX_WINDOW || wy < 0 || wy > SMJ_MATCH_MAX_WINDOW)
    return fail(c, -1, "window %d x %d outside [0, %d]", wx, wy, (int)SMJ_MATCH_MAX_WINDOW);
  if (shift_weight < 0 || shift_weight > SMJ_MATCH_MAX_SHIFT_WEIGHT) return fail(c, -1, "shift_weight %d outside [0, %d]", shift_weight, (int)SMJ_MATCH_MAX_SHIFT_WEIGHT);
  if (min_points < 1 || min_points > SMJ_MATCH_MAX_POINTS) return fail(c, -1, "min_points %d outside [1, %d]", min_points, (int)SMJ_MATCH_MAX_POINTS);
  // the workgroup of an env reads its inputs while others store
  const uintptr_t envs = (uintptr_t)c->num_envs, T = (uintptr_t)num_angles, cand = T * (uintptr_t)(2 * wy + 1) * (uintptr_t)(2 * wx + 1);
  TRY(check_disjoint(c, {{lidar_dev, scan_extent(c, lidar_ld), "scan"}, {field_dev, envs * (uintptr_t)nx * (uintptr_t)ny, "field"},
                         {pose_dev, envs * 12u, "pose"}, {angle_dev, T * 4u, "angle"}, {angle_bias_dev, T * 4u, "angle_bias"},
                         {c->state.xpose, xpose_extent(c), "XPOSE slot's"}},
                     {{pose_out_dev, envs * 12u, "pose_out"}, {best_dev, envs * 16u, "best"}, {score_dev, envs * cand * 4u, "score"},
                      {cell_dev, envs * T * (uintptr_t)nlidar * 8u, "cell"}}));
  TRY(check_xpose(c));
  HIPCHK(c, hipSetDevice(c->device));
  smj_launch_match(scan_source(c, lidar_dev, lidar_ld), c->num_envs, nlidar, frame, r_min, r_max, (const uint8_t*)field_dev, nx, ny, x0, y0, cell,
                   (const float*)pose_dev, (const float*)angle_dev, (const int*)angle_bias_dev, num_angles, wx, wy, shift_weight, min_points,
                   (float*)pose_out_dev, (int*)best_dev, (int*)score_dev, (int*)cell_dev, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return 0;
}

static_assert((int)SMJ_MAP_MAX_RAYS == (int)SMJ_MATCH_MAX_POINTS, "smj_map.h integrates the scans smj_match.h matches, at the poses it finds");

int smj_scan_to_map(smj_ctx* c, const void* lidar_dev, long lidar_ld, int frame, float r_min, float r_max, const void* pose_dev, const void* gate_dev, long gate_ld,
                    float x0, float y0, float cell, int nx, int ny, int no_return_clears, int accumulate, void* hit_dev, void* miss_dev, void* info_dev,
                    void* cell_dev, void* stream) {
  if (!c) return -1;
  TRY(check_scan(c, SMJ_MAP_MAX_RAYS, "map"));
  if (!lidar_dev || !pose_dev || !hit_dev || !info_dev) return fail(c, -1, "null scan / pose / hit / info buffer");
  TRY(check_aligned(c, {lidar_dev, pose_dev, gate_dev, hit_dev, miss_dev, info_dev, cell_dev}, "scan / pose / gate / hit / miss / info / cell buffer"));
  const int nlidar = c->render.nlidar;
  TRY(check_lidar_ld(c, lidar_ld));
  if (gate_ld < 1) return fail(c, -1, "gate_ld %ld below 1", gate_ld);
  TRY(check_cell_grid(c, nx, ny, SMJ_OCC_MAX_CELLS, SMJ_OCC_MAX_CELLS));   // the grids of smj_lidar_to_occupancy: no bound on a side but the cell count
  TRY(check_origin_cell(c, x0, y0, cell));
  TRY(check_range_limits(c, r_min, r_max, cell, RAY_TOO_LONG));
  TRY(check_robot_frame(c, frame));
  // the workgroups of an env read its inputs while others store
  const uintptr_t envs = (uintptr_t)c->num_envs, cells = envs * (uintptr_t)nx * (uintptr_t)ny;
  TRY(check_disjoint(c, {{lidar_dev, scan_extent(c, lidar_ld), "scan"}, {pose_dev, envs * 12u, "pose"},
                         {gate_dev, ((envs - 1) * (uintptr_t)gate_ld + 1) * 4u, "gate"}, {c->state.xpose, xpose_extent(c), "XPOSE slot's"}},
                     {{hit_dev, cells * 4u, "hit"}, {miss_dev, cells * 4u, "miss"}, {info_dev, envs * 16u, "info"}, {cell_dev, envs * (uintptr_t)nlidar * 16u, "cell"}}));
  TRY(check_xpose(c));
  HIPCHK(c, hipSetDevice(c->device));
  smj_launch_map(scan_source(c, lidar_dev, lidar_ld), c->num_envs, nlidar, frame, r_min, r_max, (const float*)pose_dev, (const int*)gate_dev, gate_ld, x0, y0, cell,
                 nx, ny, no_return_clears != 0, accumulate != 0, (int*)hit_dev, (int*)miss_dev, (int*)info_dev, (int*)cell_dev, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return 0;
}

static_assert((int)SMJ_MCL_MAX_POINTS == (int)SMJ_MATCH_MAX_POINTS, "smj_mcl.h weighs particles by the scans and fields smj_match.h matches");

int smj_scan_to_particles(smj_ctx* c, const void* lidar_dev, long lidar_ld, int frame, float r_min, float r_max, const void* field_dev, int nx, int ny,
                          float x0, float y0, float cell, const void* particle_dev, int num_particles, const void* noise_dev, const void* draw_dev, int span,
                          int min_points, int resample, void* particle_out_dev, void* weight_dev, void* ancestor_dev, void* stat_dev, void* pose_out_dev,
                          void* stream) {
  if (!c) return -1;
  TRY(check_scan(c, SMJ_MCL_MAX_POINTS, "weigh particles by"));
  if (!lidar_dev || !field_dev || !particle_dev || !particle_out_dev || !weight_dev || !stat_dev)
    return fail(c, -1, "null scan / field / particle / particle_out / weight / stat buffer");
  if (resample != 0 && resample != 1) return fail(c, -1, "resample %d is neither 0 nor 1", resample);
  if (resample && !draw_dev) return fail(c, -1, "null draw buffer with resample = 1");
  TRY(check_aligned(c, {lidar_dev, particle_dev, noise_dev, draw_dev, particle_out_dev, weight_dev, ancestor_dev, stat_dev, pose_out_dev},
                    "scan / particle / noise / draw / particle_out / weight / ancestor / stat / pose_out buffer"));
  const int nlidar = c->render.nlidar;
  TRY(check_lidar_ld(c, lidar_ld));
  TRY(check_cell_grid(c, nx, ny, SMJ_MATCH_MAX_SIDE, SMJ_MATCH_MAX_CELLS));
  TRY(check_origin_cell(c, x0, y0, cell));
  TRY(check_range_limits(c, r_min, r_max, cell, RAY_BOUND_OF_OCC));
  TRY(check_robot_frame(c, frame));
  if (num_particles < 1 || num_particles > SMJ_MCL_MAX_PARTICLES) return fail(c, -1, "num_particles %d outside [1, %d]", num_particles, (int)SMJ_MCL_MAX_PARTICLES);
  if (span < 1 || span > SMJ_MCL_MAX_SPAN) return fail(c, -1, "span %d outside [1, %d]", span, (int)SMJ_MCL_MAX_SPAN);
  if (min_points < 1 || min_points > SMJ_MCL_MAX_POINTS) return fail(c, -1, "min_points %d outside [1, %d]", min_points, (int)SMJ_MCL_MAX_POINTS);
  // the workgroup of an env reads its inputs while others store
  const uintptr_t envs = (uintptr_t)c->num_envs, words = envs * (uintptr_t)num_particles;
  TRY(check_disjoint(c, {{lidar_dev, scan_extent(c, lidar_ld), "scan"}, {field_dev, envs * (uintptr_t)nx * (uintptr_t)ny, "field"},
                         {particle_dev, words * 12u, "particle"}, {noise_dev, words * 12u, "noise"}, {draw_dev, envs * 4u, "draw"},
                         {c->state.xpose, xpose_extent(c), "XPOSE slot's"}},
                     {{particle_out_dev, words * 12u, "particle_out"}, {weight_dev, words * 4u, "weight"}, {ancestor_dev, words * 4u, "ancestor"},
                      {stat_dev, envs * 4u * (uintptr_t)SMJ_MCL_STAT_WORDS, "stat"}, {pose_out_dev, envs * 12u, "pose_out"}}));
  TRY(check_xpose(c));
  HIPCHK(c, hipSetDevice(c->device));
  smj_launch_mcl(scan_source(c, lidar_dev, lidar_ld), c->num_envs, nlidar, frame, r_min, r_max, (const uint8_t*)field_dev, nx, ny, x0, y0, cell,
                 (const float*)particle_dev, num_particles, (const float*)noise_dev, (const unsigned*)draw_dev, span, min_points, resample,
                 (float*)particle_out_dev, (int*)weight_dev, (int*)ancestor_dev, (int*)stat_dev, (float*)pose_out_dev, c->mcl_stage_field, (hipStream_t)stream);
  HIPCHK(c, hipGetLastError());
  return 0;
}

int smj_set_option(smj_ctx* c, const char* name, double v) {
  if (!c || !name) return -1;
  DevModel& m = c->model;
  if (!strcmp(name, "lidar_cull")) c->lidar_cull = (int)v;                  // 1 (default): per env, only the geoms whose bounding sphere reaches the rangefinders' scan plane are staged
  else if (!strcmp(name, "mcl_stage_field")) c->mcl_stage_field = (int)v != 0;   // 1 (default): smj_scan_to_particles keeps the env's field in LDS; 0: it stays in global memory (profiles/localize_cost.txt has both)
  else if (!strcmp(name, "depth_raster")) c->render.raster = (int)v;           // 0: ray cast the meshes through their BVHs (the round-2 path)
  else if (!strcmp(name, "depth_raster_splits")) c->render.raster_splits = (int)(v < 1 ? 1 : v > 256 ? 256 : v);
  else if (!strcmp(name, "primary_rows")) m.row_limit = (int)v;   // the escalation variant keeps its full capacity (model_esc is not touched)
  else if (smj_set_step_option(c->opt, name, v)) {}   // the scheduling options, by the list of smj_step_plan.h
  else if (!smj_set_solver_option(m, name, v)) return fail(c, -1, "unknown option '%s'", name);   // the solver options of DevModel, by the list smj_step copies onto the escalation model
  return 0;
}

}  // extern "C"
